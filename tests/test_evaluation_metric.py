"""dig_amd.evaluation_metric: normalised strings, edit distance, lexicon search and confidence on the device, the reference's metric functions
on top of them and the edit-distance meter of evaluate().

Expected values come from `wagner_fischer` below (Levenshtein distance with unit costs is a definition), `oracle.decode_oracle.str_list`
for the normalised strings and a literal restatement of evaluation_metric/metrics.py:67-73, 103-202 with `wagner_fischer` in place of
`editdistance.eval`.  Everything is compared exactly except the confidence.  Operator tests run through the HIP library on the MI355X and
through the plain-C++ build in the GPU-less container (`abi_dev`)."""
import math
import string
import types

import numpy as np
import pytest
import torch

import decode_oracle as D

VOC = D.vocabulary()
EOS, PAD, UNK = VOC.index("EOS"), VOC.index("PADDING"), VOC.index("UNKNOWN")


def wagner_fischer(a, b):
    row = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, cb in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (ca != cb))
    return row[len(b)]


def test_wagner_fischer_is_levenshtein():
    assert [wagner_fischer(*p) for p in (("", ""), ("", "abc"), ("kitten", "sitting"), ("flaw", "lawn"), ("abc", "abc"), ("ab", "ba"))] == [0, 3, 3, 2, 0, 2]


def _strings(rows, dev, ld=None):
    """Device strings (int32 code points [n][ld], int32 lengths [n]) of Python strings."""
    ld = ld or max([len(r) for r in rows] + [1])
    a, n = np.zeros((len(rows), ld), np.int32), np.zeros(len(rows), np.int32)
    for i, r in enumerate(rows):
        a[i, :len(r)] = [ord(c) for c in r]
        n[i] = len(r)
    return torch.from_numpy(a).to(dev), torch.from_numpy(n).to(dev)


def _encode(word, T=25, eos=True):
    ids = [VOC.index(c) for c in word]
    ids = ids + ([EOS] if eos and len(ids) < T else [])
    return ids + [PAD] * (T - len(ids))


# ---------------------------------------------------------------------------------------------- dig_tokens_to_text
def test_tokens_to_text_matches_get_str_list(abi_dev):
    from dig_amd import evaluation_metric as EM
    B, T = 7, 25
    rng = np.random.RandomState(1)
    tok = rng.randint(0, 94, size=(B, T)).astype(np.int64)
    tok[0, 0] = EOS                                                      # EOS at position 0
    tok[1] = rng.randint(0, 62, size=T)                                  # no EOS at all (digits and letters only: full length)
    tok[2, 3], tok[2, 5], tok[2, 9] = UNK, PAD, EOS                      # UNKNOWN and PADDING inside
    tok[3, :8] = [VOC.index(c) for c in "!a-B.c?~"]; tok[3, 8] = EOS     # punctuation classes
    tok[4, :6] = [VOC.index(c) for c in "HeLLo9"]; tok[4, 6] = EOS       # upper case
    tok[5, 2], tok[5, 4], tok[5, 12] = -1, len(VOC), EOS                 # ids outside [0, n_classes)
    tok[6, 20] = EOS
    text, length = EM.tokens_to_text(torch.from_numpy(tok).to(abi_dev), VOC)
    text, length = text.cpu().numpy(), length.cpu().numpy()
    safe = tok.copy()
    safe[5, 2] = safe[5, 4] = UNK                                        # the oracle indexes the vocabulary: an outside id is dropped like UNKNOWN
    want = D.str_list(safe, VOC)
    got = ["".join(chr(c) for c in text[b, :length[b]]) for b in range(B)]
    assert got == want
    assert want[0] == "" and len(want[1]) == T and want[4] == "hello9" and want[3] == "abc"
    assert all((text[b, length[b]:] == 0).all() for b in range(B))


# ---------------------------------------------------------------------------------------------- dig_edit_distance
def _edit_cases():
    rng = np.random.RandomState(2)
    word = lambda n: "".join(rng.choice(list("abcd"), size=n))
    lens = (0, 1, 2, 25, 127, 128)
    a, b = [], []
    for la in lens:
        for lb in lens:
            a.append(word(la)); b.append(word(lb))
    for n in lens[1:]:                                                   # equal strings; strings that differ only in the last cell
        w = word(n)
        a += [w, w]; b += [w, w[:-1] + "z"]
    while len(a) < 67:
        a.append(word(rng.randint(0, 40))); b.append(word(rng.randint(0, 40)))
    return a, b


def test_edit_distance_pairs(abi_dev):
    from dig_amd import evaluation_metric as EM
    a, b = _edit_cases()
    assert len(a) == 67
    ta, la = _strings(a, abi_dev, 128)
    tb, lb = _strings(b, abi_dev, 128)
    got = EM.edit_distance(ta, la, tb, lb).cpu().tolist()
    assert got == [wagner_fischer(x, y) for x, y in zip(a, b)]
    # a_index: repeated and descending rows of `a`, and the "no word" index of an empty search
    idx = [66 - i for i in range(67)]
    idx[10] = idx[11] = idx[12] = 5
    idx[20] = -1
    got = EM.edit_distance(ta, la, tb, lb, a_index=torch.tensor(idx, dtype=torch.int32, device=abi_dev)).cpu().tolist()
    assert got == [wagner_fischer(a[j] if j >= 0 else "", y) for j, y in zip(idx, b)]


def test_edit_distance_rejects_long_rows(abi_dev):
    from dig_amd import _lib as L
    from dig_amd import evaluation_metric as EM
    ta, la = _strings(["ab"], abi_dev, 129)
    tb, lb = _strings(["ab"], abi_dev, 128)
    with pytest.raises(L.DigHipError, match="rc=-4"):
        EM.edit_distance(ta, la, tb, lb)
    with pytest.raises(L.DigHipError, match="rc=-4"):
        EM.edit_distance(tb, lb, ta, la)


# ---------------------------------------------------------------------------------------------- dig_lexicon_search
def _search_want(queries, pool, begin, count):
    idx, dist = [], []
    for q, b, c in zip(queries, begin, count):
        ds = [wagner_fischer(w, q) for w in pool[b:b + c]]
        idx.append(b + int(np.argmin(ds)) if ds else -1)
        dist.append(min(ds) if ds else -1)
    return idx, dist


def _search(dev, queries, pool, begin, count, T=25):
    from dig_amd import evaluation_metric as EM
    q, ql = _strings(queries, dev, T)
    w, wl = _strings(pool, dev)
    bi, bd = EM.lexicon_search(q, ql, w, wl, begin, count)
    return bi.cpu().tolist(), bd.cpu().tolist()


def _random_words(rng, n, lo=1, hi=12, alphabet="abcdefgh"):
    return ["".join(rng.choice(list(alphabet), size=rng.randint(lo, hi + 1))) for _ in range(n)]


def test_lexicon_search_range_sizes(abi_dev):
    """B = 5 queries against disjoint ranges of 0, 1, 50, 64 and 65 words, then all five against ranges of 1 000 that overlap."""
    rng = np.random.RandomState(3)
    pool = _random_words(rng, 1300)
    queries = ["abcabc", "hgfed", "", "aaaaaaaaaaaaaaaaaaaaaaaaa", "cdcdcdcd"]                  # (an empty query, one of the full T = 25)
    begin, count = [7, 7, 8, 58, 122], [0, 1, 50, 64, 65]
    assert _search(abi_dev, queries, pool, begin, count) == _search_want(queries, pool, begin, count)
    begin, count = [0, 100, 150, 300, 299], [1000] * 5
    assert _search(abi_dev, queries, pool, begin, count) == _search_want(queries, pool, begin, count)


def test_lexicon_search_shared_range_is_split_and_ties_take_the_first(abi_dev):
    """A shared range of 3 001 words: more than one chunk per query (asserted through the workspace size: 8 bytes per (query, chunk)), with the
    same word on both sides of chunk boundaries, at positions 0 and last, and two different words at equal distance."""
    from dig_amd import evaluation_metric as EM
    rng = np.random.RandomState(4)
    W, B, chunk = 3001, 5, EM.CHUNK
    assert EM.lexicon_search_workspace_bytes(B, W) == B * math.ceil(W / chunk) * 8 and math.ceil(W / chunk) > 1
    assert EM.lexicon_search_workspace_bytes(B, 0) == B * 8 and EM.lexicon_search_workspace_bytes(B, chunk + 1) == B * 2 * 8
    pool = _random_words(rng, W, lo=6, hi=12)                            # (random words over a-h: none is within 1 of the planted ones)
    pool[0] = pool[W - 1] = "zzzzyyyy"                                   # query 0: positions 0 and last
    pool[63] = pool[64] = "xxxxwwww"                                     # query 1: either side of the first chunk boundary
    pool[chunk * 20 - 1] = pool[chunk * 20] = pool[chunk * 33] = "vvvvuuuu"   # query 2: either side of a later boundary, and a third copy
    pool[1500], pool[1400] = "ttttsssr", "ttttsssq"                      # query 3: two different words at distance 1, the later one planted first
    pool[2000], pool[2500] = "", "p" * 128                               # a word of length 0 and one of length 128
    queries = ["zzzzyyyy", "xxxxwwww", "vvvvuuuu", "ttttssss", ""]
    got = _search(abi_dev, queries, pool, [0] * B, [W] * B)
    assert got == _search_want(queries, pool, [0] * B, [W] * B)
    assert got[0] == [0, 63, chunk * 20 - 1, 1400, 2000] and got[1] == [0, 0, 0, 1, 0]
    # the word of 128 cells and the empty word against a query of the full T = 25, in ranges that start and end inside chunks
    long_q = ["p" * 25] * B
    begin, count = [2450, 2500, 2499, 2400, 2000], [100, 1, 2, 200, 1]
    got = _search(abi_dev, long_q, pool, begin, count)
    assert got == _search_want(long_q, pool, begin, count) and (got[0][1], got[1][1]) == (2500, 103) and (got[0][4], got[1][4]) == (2000, 25)
    begin, count = [1, 1, 1, 1, 1], [W - 1] * B                          # shifted by one: the copies at 63 | 64 now share a chunk, 0 is outside
    got = _search(abi_dev, queries, pool, begin, count)
    assert got == _search_want(queries, pool, begin, count) and got[0][:2] == [W - 1, 63]


def test_lexicon_search_wrapper_rejects_ranges_outside_the_pool(abi_dev):
    pool = ["ab", "cd", "ef"]
    for begin, count in (([0, 2], [3, 2]), ([-1, 0], [1, 1]), ([0, 0], [1, -1]), ([0, 3], [1, 1])):
        with pytest.raises(ValueError, match="outside the pool"):
            _search(abi_dev, ["ab", "cd"], pool, begin, count)
    assert _search(abi_dev, ["ab", "cd"], pool, [0, 3], [3, 0]) == ([0, -1], [0, -1])


def test_lexicon_search_clamps_ranges_in_the_kernel(abi_dev):
    """Below the wrapper: a range that reaches outside [0, W) is clamped by the entry point itself, not followed."""
    from dig_amd import _lib as L
    pool = ["ab", "cd", "ef", "gh"]
    q, ql = _strings(["gh", "ab", "ef"], abi_dev, 25)
    w, wl = _strings(pool, abi_dev)
    rng = torch.tensor([[2, -5, 4], [1000, 2, 7]], dtype=torch.int32, device=abi_dev)           # [2, 4), [0, 2), nothing
    bi, bd = torch.empty(3, dtype=torch.int32, device=abi_dev), torch.empty(3, dtype=torch.int32, device=abi_dev)
    ws = torch.empty(3 * 16, dtype=torch.int64, device=abi_dev)
    L.call("dig_lexicon_search", L.ptr(q), L.ptr(ql), 25, 3, L.ptr(w), L.ptr(wl), 2, 4, L.ptr(rng[0]), L.ptr(rng[1]), 1000, L.ptr(bi), L.ptr(bd),
           L.ptr(ws), ws.numel() * 8, L.stream())
    assert bi.cpu().tolist() == [3, 0, -1] and bd.cpu().tolist() == [0, 0, -1]


# ---------------------------------------------------------------------------------------------- dig_seq_confidence
def test_seq_confidence(abi_dev):
    """exp(sum(log)) in double over min(T, text_len + 1) scores.  Double rounding over at most 129 terms stays below 1e-13 relative; a
    float32 sum or logarithm is off by about 6e-8: the bound 1e-9 separates the two."""
    from dig_amd import evaluation_metric as EM
    B, T = 5, 25
    rng = np.random.RandomState(6)
    score = rng.uniform(1e-3, 1.0, size=(B, T)).astype(np.float32)
    text_len = [0, 3, 24, 25, 30]
    got = EM.seq_confidence(torch.from_numpy(score).to(abi_dev), torch.tensor(text_len, dtype=torch.int32, device=abi_dev)).cpu().tolist()
    for b in range(B):
        want = math.exp(sum(map(math.log, score[b, :min(T, text_len[b] + 1)])))
        assert abs(got[b] - want) <= 1e-9 * want, (b, got[b], want)


# ---------------------------------------------------------------------------------------------- the reference's functions
def _normalize_text(text):
    return "".join(filter(lambda x: x in (string.digits + string.ascii_letters), text)).lower()


def _ref_lexicon_search(lexicon, word):                                  # metrics.py:67-73
    ds = np.asarray([wagner_fischer(_normalize_text(w), _normalize_text(word)) for w in lexicon], dtype=np.int64)
    return lexicon[np.argmin(ds)]


def _ref_with_lexicon(pred_list, targ_list, dataset, file_names, per_pair, fold):      # metrics.py:103-139 / :150-186
    out = [fold([per_pair(p, t) for p, t in zip(pred_list, targ_list)])]
    for lex in (dataset.lexicons50, dataset.lexicons1k, dataset.lexiconsfull):
        if len(file_names) == 0 or len(lex[file_names[0]]) == 0:
            out.append(0)
        else:
            refined = [_ref_lexicon_search(lex[f], p) for f, p in zip(file_names, pred_list)]
            out.append(fold([per_pair(p, t) for p, t in zip(refined, targ_list)]))
    return out


def _ref_rec_post_process(pred_list, score, T):                          # metrics.py:189-202
    return [math.exp(sum(map(math.log, score[i, :min(T, len(p) + 1)]))) for i, p in enumerate(pred_list)]


def _metric_case(dev):
    targets = ["Hello", "world", "street9", "cafe", "a-b"]
    preds = ["Hellp", "wor1d", "street9", "kafe!", "ab"]
    names = ["img0", "img1", "img2", "img3", "img4"]
    lex50 = {"img0": ["helm", "HELLO", "hello"],                        # the upper-case word is the first nearest: never counts as correct
             "img1": ["sword", "world", "wor-ld"], "img2": ["street", "street9"], "img3": ["cafe", "kale"], "img4": ["a-b", "ab"]}
    lex1k = {n: [] if n == "img0" else ["x"] for n in names}              # an empty first lexicon: the level reports 0
    full = ["hello", "world", "street9", "cafe", "ab", "Street9", "wor1d"]
    lexfull = {n: full for n in names}                                   # one shared list
    dataset = types.SimpleNamespace(idx_to_class={i: c for i, c in enumerate(VOC)}, lexicons50=lex50, lexicons1k=lex1k, lexiconsfull=lexfull)
    out = torch.tensor([_encode(p) for p in preds], dtype=torch.int64, device=dev)
    tgt = torch.tensor([_encode(t) for t in targets], dtype=torch.int64, device=dev)
    return dataset, out, tgt, names


def test_metric_functions_match_the_reference_restatement(abi_dev):
    from dig_amd import evaluation_metric as EM
    assert EM.names() == ["accuracy", "accuracy_with_lexicon", "editdistance", "editdistance_with_lexicon", "recognition_fmeasure"]
    f = EM.factory()
    dataset, out, tgt, names = _metric_case(abi_dev)
    pred_list, targ_list = D.str_list(out.cpu().numpy(), VOC), D.str_list(tgt.cpu().numpy(), VOC)
    assert pred_list == ["hellp", "wor1d", "street9", "kafe", "ab"] and targ_list == ["hello", "world", "street9", "cafe", "ab"]
    mean = lambda v: 1.0 * sum(v) / len(v)
    want_acc = _ref_with_lexicon(pred_list, targ_list, dataset, names, lambda p, t: p == t, mean)
    want_ed = _ref_with_lexicon(pred_list, targ_list, dataset, names, wagner_fischer, sum)
    assert want_acc == [0.4, 0.6, 0, 0.8] and want_ed == [3, 5 + 1, 0, 1]                # the quirks are in the case: HELLO and a-b are chosen
    got_acc, got_ed = f["accuracy_with_lexicon"](out, tgt, dataset, names), f["editdistance_with_lexicon"](out, tgt, dataset, names)
    assert got_acc == want_acc and got_ed == want_ed
    assert isinstance(got_acc[2], int) and all(isinstance(v, int) for v in got_ed)
    assert f["accuracy_with_lexicon"](out, tgt, dataset, []) == [want_acc[0], 0, 0, 0]
    assert f["editdistance_with_lexicon"](out, tgt, dataset, []) == [want_ed[0], 0, 0, 0]
    ed = f["editdistance"](out, tgt, dataset)
    assert isinstance(ed, int) and ed == want_ed[0] == 3
    assert abs(f["accuracy"](out, tgt, dataset) - want_acc[0]) < 1e-7 and isinstance(f["accuracy"](out, tgt, dataset), float)
    assert abs(f["recognition_fmeasure"](out, tgt, dataset) - D.recognition_f_measure(out.cpu().numpy(), tgt.cpu().numpy(), VOC)) < 1e-12
    # RecPostProcess
    score = torch.from_numpy(np.random.RandomState(8).uniform(1e-3, 1.0, size=(5, 25)).astype(np.float32))
    p, t, s = EM.RecPostProcess(out, tgt, score.to(abi_dev), dataset)
    assert p == pred_list and t == targ_list
    want_s = _ref_rec_post_process(pred_list, score.numpy(), 25)
    assert len(s) == 5 and all(abs(a - b) <= 1e-9 * b for a, b in zip(s, want_s))


def test_lexicon_class():
    from dig_amd import evaluation_metric as EM
    shared = ["Abc", "d-e", "x"]
    lex = EM.Lexicon({"a": shared, "b": ["q"], "c": list(shared), "d": []})
    assert lex.ranges["a"] == lex.ranges["c"] == (0, 3) and lex.ranges["b"] == (3, 1) and lex.ranges["d"][1] == 0 and lex.n_words == 4
    assert lex["a"] == shared and lex["d"] == []
    row = lambda pool, n, i: "".join(chr(c) for c in pool[i, :n[i]])
    assert [row(lex.raw, lex.raw_len, i) for i in range(4)] == ["Abc", "d-e", "x", "q"]
    assert [row(lex.norm, lex.norm_len, i) for i in range(4)] == ["abc", "de", "x", "q"]
    assert lex.device("cpu") is lex.device("cpu")                        # uploaded once per device
    EM.Lexicon({"a": ["w" * 128]})
    with pytest.raises(ValueError, match="w" * 129):
        EM.Lexicon({"a": ["ok", "w" * 129]})
    dataset = types.SimpleNamespace(lexicons50={"a": shared})
    assert EM._lexicon(dataset, "lexicons50") is EM._lexicon(dataset, "lexicons50")                   # a plain dict is wrapped once
    dataset.lexicons50 = lex
    assert EM._lexicon(dataset, "lexicons50") is lex


# ---------------------------------------------------------------------------------------------- evaluate()
class _StubModel:
    """Returns the probabilities whose arg-max are the given predictions (what evaluate() reads of a recognizer)."""
    beam_width = 0

    def __init__(self, preds):
        self.preds, self.i = preds, 0

    def eval(self):
        return self

    def __call__(self, x):
        ids = self.preds[self.i].to(x[0].device)
        self.i += 1
        probs = torch.full(ids.shape + (len(VOC),), 0.01 / (len(VOC) - 1), device=ids.device)
        probs.scatter_(2, ids[..., None], 0.99)
        return probs, None, None, None


def _eval_case():
    rng = np.random.RandomState(9)
    words = _random_words(rng, 11, lo=1, hi=10, alphabet="abcXYZ019-")
    preds = [w[:-1] + "q" if i % 3 == 0 else (w[1:] if i % 3 == 1 else w) for i, w in enumerate(words)]
    batches, pred_ids = [], []
    for lo, hi in ((0, 4), (4, 11)):
        tgt = torch.tensor([_encode(w) for w in words[lo:hi]], dtype=torch.int64)
        lens = torch.tensor([len(w) + 1 for w in words[lo:hi]], dtype=torch.int64)
        batches.append((torch.zeros(hi - lo, 3, 32, 128), tgt, lens))
        pred_ids.append(torch.tensor([_encode(p) for p in preds[lo:hi]], dtype=torch.int64))
    loader = type("Loader", (list,), {})(batches)
    loader.dataset = types.SimpleNamespace(idx_to_class={i: c for i, c in enumerate(VOC)})
    want = sum(wagner_fischer(_normalize_text(p), _normalize_text(w)) for p, w in zip(preds, words)) / len(words)
    return loader, pred_ids, want


def test_evaluate_edit_distance_meter(abi_dev, capsys):
    from dig_amd.engine_for_finetuning import evaluate
    loader, pred_ids, want = _eval_case()
    plain = evaluate(loader, _StubModel(pred_ids), abi_dev, types.SimpleNamespace(beam_width=0))
    line_plain = [l for l in capsys.readouterr().out.splitlines() if l.startswith("* ")][-1]
    assert sorted(plain) == ["acc", "loss", "recognition_fmeasure"]
    assert line_plain == "* 11 images, Acc {:.4f} loss {:.4f} Rec_fmeasure {:.4f}".format(plain["acc"], plain["loss"], plain["recognition_fmeasure"])
    off = evaluate(loader, _StubModel(pred_ids), abi_dev, types.SimpleNamespace(beam_width=0, eval_edit_distance=False))
    assert off == plain
    capsys.readouterr()
    on = evaluate(loader, _StubModel(pred_ids), abi_dev, types.SimpleNamespace(beam_width=0, eval_edit_distance=True))
    line_on = [l for l in capsys.readouterr().out.splitlines() if l.startswith("* ")][-1]
    assert sorted(on) == ["acc", "edit_distance", "loss", "recognition_fmeasure"]
    assert want > 0 and abs(on["edit_distance"] - want) < 1e-12
    assert {k: on[k] for k in plain} == plain
    assert line_on == line_plain + " Edit_distance {:.4f}".format(want)
