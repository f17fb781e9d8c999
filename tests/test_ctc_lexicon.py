"""Lexicon-constrained CTC decoding by likelihood (`--ctc_lexicon`, dig_ctc_lexicon_decode in csrc/ctc.hip and cpu_abi/dig_cpu_rec.cpp)
against its specification tests/ctc_lexicon_model.py (torch's ctc_loss on log_softmax at float64 / float32).  Operator tests run on both
builds (`abi_dev`); the wiring through `LabelLexicon`, `CTCRecModelTrain.decode`, `evaluate`, the two metric functions and the driver flag
follows.

Which samples assert the arg-max is decided by the specification alone, by the procedure of tests/test_ctc_beam.py: its fixed-seed frame
generator draws 2n candidates per case; per sample the lexicon is the frames' collapse, single substitutions / deletions / insertions of it
and random words, shuffled.  With e32 = the largest |s32 - s64| over the finite scores and G = 64 * max(e32, 2^-20 * max |s64|), a sample
is kept when its float64 gap between the best and the second word is at least G; the first n kept are asserted, fewer than n kept fails.
Every finite score and logp must satisfy |got - s64| <= 4 e32 + 2^-20 |s64| (the bound of test_ctc_beam.py: the specification's own fp32
error, not the kernel's), the -inf pattern must be exact, cells past lex_count must be -inf, and a second launch must give equal bits."""
import ctypes
import itertools
import math
import os
import random
import types

import numpy as np
import pytest
import torch

import ctc_lexicon_model as LM
import ctc_model as S
from test_ctc_beam import _draw, _symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")


def _chunk():
    from dig_amd import _lib as L
    return L.const("DIG_CTC_LEX_CHUNK")


def _collapse(frames, blank):
    return [c for j, c in enumerate(frames) if c != blank and not (j > 0 and frames[j - 1] == c)]


def _lexicon_for(frames, C, blank, n_words, rng, max_len):
    """n_words distinct words: the collapse of `frames`, single edits of it, random words; shuffled."""
    T = len(frames)
    classes = [c for c in range(C) if c != blank]
    base = _collapse(frames, blank)[:max_len]
    words, seen = [], set()

    def add(w):
        w = tuple(w[:max_len])
        if w not in seen and len(words) < n_words:
            seen.add(w)
            words.append(list(w))

    add(base)
    tries = 0
    while len(words) < max(1, n_words // 2) and tries < 20 * n_words:       # single edits
        tries += 1
        kind, w = rng.randrange(3), list(base)
        if kind == 0 and w:
            w[rng.randrange(len(w))] = rng.choice(classes)
        elif kind == 1 and w:
            del w[rng.randrange(len(w))]
        else:
            w.insert(rng.randrange(len(w) + 1), rng.choice(classes))
        add(w)
    while len(words) < n_words:                                              # random words (repeats allowed: some have no alignment)
        add([rng.choice(classes) for _ in range(rng.randrange(0, min(T, max_len) + 1))])
    rng.shuffle(words)
    return words


def _pool_tensors(pool, dev, ldw=None):
    ldw = max([len(w) for w in pool] + [1]) if ldw is None else ldw
    rows, lens = np.zeros((max(len(pool), 1), ldw), dtype=np.int32), np.zeros(max(len(pool), 1), dtype=np.int32)
    for i, w in enumerate(pool):
        rows[i, :len(w)] = w
        lens[i] = len(w)
    return torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)


def _spec(x, pool, begin, count, blank):
    """The specification's figures of one call: s64, e32, G, best, logp, gap."""
    s64 = LM.lexicon_scores(x, pool, begin, count, blank, torch.float64)
    s32 = LM.lexicon_scores(x, pool, begin, count, blank, torch.float32).double()
    fin = torch.isfinite(s64) & torch.isfinite(s32)
    assert bool((torch.isfinite(s64) == torch.isfinite(s32)).all())
    e32 = float((s32 - s64)[fin].abs().max()) if bool(fin.any()) else 0.0
    G = 64 * max(e32, 2.0 ** -20 * (float(s64[fin].abs().max()) if bool(fin.any()) else 0.0))
    best, logp, gap = LM.choose(s64, begin)
    return dict(s64=s64, e32=e32, G=G, best=best, logp=logp, gap=gap)


def _run(dev, x, C, pool, begin, count, sym=None, ldw=None):
    from dig_amd.ctc_recognizer import ctc_lexicon_decode
    blank, eos, pad = _symbols(C) if sym is None else sym
    out = ctc_lexicon_decode(x.to(dev), C, blank, eos, pad, _pool_tensors(pool, dev, ldw), begin, count, want_scores=True)
    return [t.cpu() for t in out]


def _check(dev, x, C, pool, begin, count, min_kept=0, sp=None, tag="", sym=None):
    """One call against the specification: every score, the -inf pattern, the rows; the arg-max on the samples the gap rule keeps (all of
    them must number at least min_kept).  Returns (outputs, specification)."""
    blank, eos, pad = _symbols(C) if sym is None else sym
    B, T = x.shape[0], x.shape[1]
    sp = _spec(x[:, :, :C], pool, begin, count, blank) if sp is None else sp
    best_index, logp, ids, score, n, scores = _run(dev, x, C, pool, begin, count, sym)
    mc = max([int(c) for c in count] + [0])
    assert best_index.dtype == torch.int32 and ids.dtype == torch.int64 and n.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(scores.shape) == (B, mc) and tuple(ids.shape) == (B, T + 1) and tuple(score.shape) == (B, T + 1) and tuple(logp.shape) == (B,)
    s64, e32 = sp["s64"], sp["e32"]
    fin = torch.isfinite(s64)
    assert torch.equal(scores == NINF, ~fin), "the -inf pattern"            # (cells past lex_count are -inf in the specification too)
    err = (scores.double() - s64)[fin].abs()
    bound = (4 * e32 + 2.0 ** -20 * s64.abs())[fin]
    keep = sp["gap"] >= sp["G"]
    print(f"{tag}: kept {int(keep.sum())} of {B}, e32 {e32:.3e}, G {sp['G']:.3e}, score err {float(err.max()) if err.numel() else 0.0:.3e}")
    assert bool((err <= bound).all()), (float(err.max()), e32)
    assert int(keep.sum()) >= min_kept
    # whatever was chosen: logp is the score of the chosen cell, and the row is that word
    for b in range(B):
        w = int(best_index[b])
        if w < 0:
            assert not bool(fin[b].any()) and float(logp[b]) == NINF and float(score[b, 0]) == 0.0 and int(n[b]) == 0
            word = []
        else:
            j = w - int(begin[b])
            assert 0 <= j < int(count[b]) and float(logp[b]) == float(scores[b, j]) == float(scores[b].max())
            assert j == int((scores[b] == scores[b].max()).nonzero()[0])      # the first of equal scores
            word = pool[w]
            want_s0 = math.exp(float(logp[b]))
            assert abs(float(score[b, 0]) - want_s0) <= 1e-6 * want_s0 + 2.0 ** -149       # (fp32: half an ulp, or one denormal step)
        assert int(n[b]) == len(word) and ids[b, :len(word)].tolist() == word
        assert int(ids[b, len(word)]) == eos and bool((ids[b, len(word) + 1:] == pad).all())
        assert bool((score[b, 1:] == 1.0).all())
    kb = keep.nonzero().reshape(-1)
    assert torch.equal(best_index.long()[kb], sp["best"][kb]), (best_index, sp["best"])
    kb = (keep & (sp["best"] >= 0)).nonzero().reshape(-1)                    # (no word: logp = -inf on both sides, checked above)
    lerr = (logp.double() - sp["logp"])[kb].abs()
    assert bool((lerr <= 4 * e32 + 2.0 ** -20 * sp["logp"][kb].abs()).all())
    return (best_index, logp, ids, score, n, scores), sp


# ---------------------------------------------------------------------------------------------- 1. the table of cases
# (T, C, words per sample, B, peak, bump).  Kept of drawn with these values (the generator above, seeds as below): T32_50 16 of 16,
# T32_1000 7 of 8, T64_65 8 of 8, C256_33 4 of 4, grid_edge 12 of 12, T5 4 of 4, flat 16 of 16; e32 from 2.3e-6 (T5) to 1.5e-4 (T64_65)
CASES = {
    "T32_50": (32, 98, 50, 8, 5.0, 4.0),                                      # the recipe shape
    "T32_1000": (32, 98, 1000, 4, 5.0, 4.0),
    "T64_65": (64, 98, 65, 4, 5.0, 4.0),
    "C256_33": (8, 256, 33, 2, 5.0, 4.0),
    "grid_edge": (12, 6, 129, 6, 2.5, 2.0),                                   # about a fifth of the words have no alignment
    "T5": (5, 4, 7, 2, 5.0, 4.0),
    "flat": (32, 98, 64, 8, 2.0, 2.0),                                        # flat frames
}
_REF = {}


def _reference(name):
    """Computed once per case and shared: the first B kept samples of 2 B drawn, their disjoint ranges and the specification's figures."""
    if name not in _REF:
        T, C, nw, B, peak, bump = CASES[name]
        blank, eos, pad = _symbols(C)
        x, frames = _draw(T, C, 2 * B, seed=77 * T + 10 * C + nw, peak=peak, bump=bump)
        rng = random.Random(1000 * T + C + nw)
        lex = [_lexicon_for(frames[b].tolist(), C, blank, nw, rng, 63) for b in range(2 * B)]
        pool = [w for l in lex for w in l]
        begin = [b * nw for b in range(2 * B)]
        sp = _spec(x[:, :, :C], pool, begin, [nw] * (2 * B), blank)
        keep = (sp["gap"] >= sp["G"]).nonzero().reshape(-1)
        infeasible = float((sp["s64"] == NINF).double().mean())
        print(f"{name}: kept {len(keep)} of {2 * B}, e32 {sp['e32']:.3e}, G {sp['G']:.3e}, words without a score {infeasible:.2f}")
        assert len(keep) >= B, (name, len(keep), 2 * B)
        keep = keep[:B]
        sub = dict(s64=sp["s64"][keep], e32=sp["e32"], G=sp["G"], best=sp["best"][keep], logp=sp["logp"][keep], gap=sp["gap"][keep])
        _REF[name] = dict(x=x[keep].contiguous(), frames=frames[keep], pool=pool, begin=[begin[int(k)] for k in keep], count=[nw] * B, sp=sub)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_ctc_lexicon_decode_equals_the_specification(abi_dev, name):
    T, C, nw, B, _, _ = CASES[name]
    r = _reference(name)
    assert r["x"].shape[0] == B and bool(torch.isnan(r["x"][:, :, C:]).all())
    out, _ = _check(abi_dev, r["x"], C, r["pool"], r["begin"], r["count"], min_kept=B, sp=r["sp"], tag=name)
    again = _run(abi_dev, r["x"], C, r["pool"], r["begin"], r["count"])       # a second launch: equal bits
    for a, b_ in zip(out, again):
        assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8))
    if name == "grid_edge":
        assert 0.05 < float((r["sp"]["s64"] == NINF).double().mean()) < 0.5


def test_ctc_lexicon_decode_at_the_limits(abi_dev):
    """T = 64, C = 256, ldw = 63: the sample's table fills 64 KB of LDS, more than a launch gets without asking.  Kept: 2 of 2."""
    T, C, B, nw = 64, 256, 2, 9
    blank = C - 1
    x, frames = _draw(T, C, B, seed=64256, peak=5.0, bump=4.0)
    rng = random.Random(256)
    pool = []
    for b in range(B):
        pool += _lexicon_for(frames[b].tolist(), C, blank, nw - 1, rng, 63) + [_word_of_length(63, frames[b].tolist(), C, blank, rng)]
    out, _ = _check(abi_dev, x, C, pool, [0, nw], [nw, nw], min_kept=B, tag="limits")
    assert tuple(_pool_tensors(pool, "cpu")[0].shape) == (2 * nw, 63) and bool(torch.isfinite(out[5][:, -1]).all())


# ---------------------------------------------------------------------------------------------- 2. exhaustive
def test_ctc_lexicon_decode_over_every_labeling(abi_dev):
    """T = 5, C = 4: the lexicon is all 364 labelings of length <= 5 over the 3 classes other than the blank (several chunks, one range
    shared by the samples).  Their probabilities partition the alignments: the exponentiated finite scores sum to 1, in double on the host,
    within 364 * 4 e32; the winner is the best labeling by brute force."""
    T, C, n_keep = 5, 4, 4
    blank = C - 1
    pool = [list(l) for k in range(T + 1) for l in itertools.product(range(3), repeat=k)]
    assert len(pool) == 364 and len(pool) > 2 * _chunk()
    x, _ = _draw(T, C, 2 * n_keep, seed=555, peak=5.0, bump=4.0)
    begin, count = [0] * (2 * n_keep), [364] * (2 * n_keep)
    sp = _spec(x[:, :, :C], pool, begin, count, blank)
    assert float((torch.exp(sp["s64"]).sum(1) - 1).abs().max()) <= 1e-12     # the specification, on the CPU first
    keep = (sp["gap"] >= sp["G"]).nonzero().reshape(-1)
    assert len(keep) >= n_keep, (len(keep), sp["e32"], sp["G"])
    keep = keep[:n_keep]
    sub = {k: (v[keep] if torch.is_tensor(v) else v) for k, v in sp.items()}
    (best_index, logp, ids, score, n, scores), _ = _check(abi_dev, x[keep].contiguous(), C, pool, [0] * n_keep, [364] * n_keep, min_kept=n_keep,
                                                        sp=sub, tag="exhaustive")
    total = torch.exp(scores.double()).sum(1)
    print(f"exhaustive: sum of probabilities - 1 = {float((total - 1).abs().max()):.3e} (bound {364 * 4 * sp['e32']:.3e})")
    assert bool(((total - 1).abs() <= 364 * 4 * sp["e32"]).all())
    assert torch.equal(best_index.long(), sub["s64"].argmax(1))


# ---------------------------------------------------------------------------------------------- 3. against the loss kernel
@pytest.mark.parametrize("name", ["T32_50", "T64_65"])
def test_ctc_lexicon_scores_are_the_loss_kernels_likelihoods(abi_dev, name):
    """scores[b][j] against -nll of dig_ctc_loss on the same sample and word.  The device kernels share ctc_alpha_step, the emission
    arithmetic, the re-centring and the double offset, so on the device the two are asserted equal bit for bit; the plain C++ build's loss
    runs in double, so there the bound of the specification holds: |score + nll| <= 4 e32 + 2^-20 |s64|."""
    from dig_amd.ctc_recognizer import ctc_loss
    T, C, nw, B, _, _ = CASES[name]
    blank = C - 1
    r = _reference(name)
    _, _, _, _, _, scores = _run(abi_dev, r["x"], C, r["pool"], r["begin"], r["count"])
    words = [r["pool"][r["begin"][b] + j] for b in range(B) for j in range(nw)]
    ldt = max(len(w) for w in words)
    target = torch.zeros((B * nw, ldt), dtype=torch.int64)
    for i, w in enumerate(words):
        target[i, :len(w)] = torch.tensor(w, dtype=torch.int64)
    lens = torch.tensor([len(w) for w in words])
    xr = r["x"].repeat_interleave(nw, 0).contiguous()
    nll, _ = ctc_loss(xr.to(abi_dev), C, target.to(abi_dev), lens.to(abi_dev), blank, len_offset=0)
    nll = nll.cpu().reshape(B, nw)
    fin = torch.isfinite(scores)
    assert bool((nll[~fin] == 0).all())                                       # (zero_infinity on the loss's side)
    diff = (scores.double() + nll.double())[fin].abs()
    print(f"{name}: largest |score + nll| {float(diff.max()):.3e} over {int(fin.sum())} pairs, bits differ in {int((scores != -nll)[fin].sum())}")
    if abi_dev.type == "cuda":
        assert torch.equal(scores[fin].view(torch.int32), (-nll)[fin].view(torch.int32))
    else:
        assert bool((diff <= (4 * r["sp"]["e32"] + 2.0 ** -20 * r["sp"]["s64"].abs())[fin]).all())


# ---------------------------------------------------------------------------------------------- 4. segment widths
def _word_of_length(k, frames, C, blank, rng):
    """k labels without adjacent repeats (feasible up to k = T), starting from the frames' collapse."""
    classes = [c for c in range(C) if c != blank]
    w = _collapse(frames, blank)[:k]
    while len(w) < k:
        c = rng.choice(classes)
        if not w or w[-1] != c:
            w.append(c)
    return w


_WIDTHS = {}


def _width_lexicons():
    """T = 64, C = 98, four ranges: longest word 15 / 31 / 63 labels (16, 32 and 64 lanes per word), each with the lengths 0, 1, 15, 16, 31,
    32, 63 that fit, and one range sorted by length whose three chunks take the three widths in turn."""
    if not _WIDTHS:
        T, C, B = 64, 98, 8
        blank = C - 1
        x, frames = _draw(T, C, B, seed=6464, peak=5.0, bump=4.0)
        rng = random.Random(64)
        f0 = frames[0].tolist()
        pool, begin, count = [], [], []
        for longest in (15, 31, 63):
            lens = [k for k in (0, 1, 15, 16, 31, 32, 63) if k <= longest] + [rng.randrange(0, longest + 1) for _ in range(6)]
            rng.shuffle(lens)
            begin.append(len(pool))
            count.append(len(lens))
            pool += [_word_of_length(k, frames[rng.randrange(B)].tolist(), C, blank, rng) for k in lens]
        ch = _chunk()
        lens = sorted([0, 1, 15] + [rng.randrange(0, 16) for _ in range(ch - 3)]) + sorted([16, 31] + [rng.randrange(16, 32) for _ in range(ch - 2)]) \
            + sorted([32, 63] + [rng.randrange(32, 64) for _ in range(9)])
        begin.append(len(pool))
        count.append(len(lens))
        pool += [_word_of_length(k, f0 if i % 3 else frames[rng.randrange(B)].tolist(), C, blank, rng) for i, k in enumerate(lens)]
        b8, c8 = [begin[i % 4] for i in range(B)], [count[i % 4] for i in range(B)]
        _WIDTHS.update(x=x, pool=pool, begin=b8, count=c8, sp=_spec(x[:, :, :C], pool, b8, c8, blank), C=C)
    return _WIDTHS


def test_ctc_lexicon_decode_segment_widths(abi_dev):
    """Kept by the gap rule with these values: 8 of 8."""
    w = _width_lexicons()
    assert max(len(v) for v in w["pool"]) == 63 and min(len(v) for v in w["pool"]) == 0
    _check(abi_dev, w["x"], w["C"], w["pool"], w["begin"], w["count"], min_kept=8, sp=w["sp"], tag="segment widths")


# ---------------------------------------------------------------------------------------------- 5. ranges and chunk edges
_EDGE = {}


def _edge_pool():
    if not _EDGE:
        T, C, B = 12, 6, 5
        blank = C - 1
        ch = _chunk()
        x, frames = _draw(T, C, B, seed=1212, peak=2.5, bump=2.0)
        rng = random.Random(12)
        pool = []
        for b in range(B):
            pool += _lexicon_for(frames[b].tolist(), C, blank, ch + 3, rng, T)
        pool += [[2] * T, [1, 1] * (T // 2), [0] * (T - 1) + [3], [3, 3, 3, 3, 3, 3, 3], [4] * 8]      # words without an alignment
        _EDGE.update(T=T, C=C, B=B, x=x, pool=pool, bad0=len(pool) - 5, ch=ch)
        assert len(pool) >= 5 * ch + 2                                          # (the disjoint layout's last range ends there)
    return _EDGE


@pytest.mark.parametrize("layout", ["shared", "counts", "disjoint", "overlapping", "empty_and_infeasible"])
def test_ctc_lexicon_decode_ranges_and_chunk_edges(abi_dev, layout):
    """T = 12, C = 6; counts 1, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 in ranges that coincide, follow one another or overlap; an empty
    range and a range of words without an alignment give (-1, -inf), the empty row and score[b][0] = 0."""
    e = _edge_pool()
    ch, B, W = e["ch"], e["B"], len(e["pool"])
    sizes = [1, ch - 1, ch, ch + 1, 2 * ch + 1]
    if layout == "shared":
        begin, count = [3] * B, [2 * ch + 1] * B
    elif layout == "counts":
        begin, count = [0] * B, sizes
    elif layout == "disjoint":
        begin, count = [0, 1, ch, 2 * ch, 3 * ch + 1], sizes
    elif layout == "overlapping":
        begin, count = [0, 10, 20, 30, 40], sizes[::-1]
    else:
        begin, count = [5, e["bad0"], W, 0, e["bad0"] - 2], [0, 5, 0, ch, 7]
    assert all(b + c <= W for b, c in zip(begin, count))
    out, sp = _check(abi_dev, e["x"], e["C"], e["pool"], begin, count, tag=layout)
    if layout == "empty_and_infeasible":
        assert out[0].tolist()[:3] == [-1, -1, -1] and out[0][3] >= 0 and out[0][4] >= 0
        assert bool((out[1][:3] == NINF).all()) and bool((out[3][:3, 0] == 0).all())
    else:
        assert int((sp["gap"] >= sp["G"]).sum()) >= 1


# ---------------------------------------------------------------------------------------------- 6. unusable words
def test_ctc_lexicon_decode_unusable_words(abi_dev):
    """Labels -1, C, 2^31 - 1 and the blank, and a word with n + repeats = T + 1, score -inf; n + repeats = T stays finite; the other words'
    scores have the bits they have without them."""
    T, C, B = 12, 6, 3
    blank = C - 1
    x, frames = _draw(T, C, B, seed=66, peak=2.5, bump=2.0)
    rng = random.Random(6)
    good = _lexicon_for(frames[0].tolist(), C, blank, 9, rng, T)
    at_T = [0, 0, 0, 1, 1, 1, 2, 3]                                            # 8 labels + 4 repeats = 12 = T: one alignment
    over_T = [0, 0, 0, 1, 1, 1, 2, 2]                                          # 8 + 5 = 13 = T + 1: none
    bad = [[1, -1, 2], [C, 0], [0, 2 ** 31 - 1], [blank], [0, blank, 1], over_T]
    pool = good[:3] + bad[:2] + good[3:6] + bad[2:] + good[6:] + [at_T]
    where_bad = [3, 4, 8, 9, 10, 11]
    assert [pool[i] for i in where_bad] == bad
    begin, count = [0] * B, [len(pool)] * B
    (_, _, _, _, _, scores), sp = _check(abi_dev, x, C, pool, begin, count, tag="unusable")
    assert bool((scores[:, where_bad] == NINF).all()) and bool(torch.isfinite(scores[:, -1]).all())
    rest = [i for i in range(len(pool)) if i not in where_bad]
    clean = _run(abi_dev, x, C, [pool[i] for i in rest], begin, [len(rest)] * B)[5]
    assert torch.equal(scores[:, rest].view(torch.int32), clean.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 7. ties
def test_ctc_lexicon_decode_takes_the_first_of_equal_words(abi_dev):
    """The same word twice in a range (in one chunk, and a chunk apart): the first occurrence is chosen."""
    T, C, B = 12, 6, 4
    blank = C - 1
    ch = _chunk()
    x, frames = _draw(T, C, B, seed=77, peak=5.0, bump=4.0)
    rng = random.Random(7)
    pool, begin, count, first = [], [], [], []
    for b in range(B):
        lex = _lexicon_for(frames[b].tolist(), C, blank, 2 * ch + 8, rng, T)
        j = int(LM.word_scores(x[b, :, :C], lex, blank).argmax())              # the specification's choice: it gets a twin
        gap = 1 if b % 2 == 0 else ch                                          # ... right behind it / a chunk away
        at = j + gap if j + gap <= len(lex) else j - gap + 1
        words = lex[:at] + [lex[j]] + lex[at:]
        begin.append(len(pool))
        count.append(len(words))
        first.append(len(pool) + min(j, at))
        pool += words
    sp = _spec(x[:, :, :C], pool, begin, count, blank)
    assert sp["best"].tolist() == first and bool((sp["gap"] == 0).all())       # the specification: the first of the two equal words
    best_index = _run(abi_dev, x, C, pool, begin, count)[0]
    assert best_index.tolist() == first
    _check(abi_dev, x, C, pool, begin, count, sp=sp, tag="ties")


# ---------------------------------------------------------------------------------------------- 8. peaked frames
def test_ctc_lexicon_decode_on_peaked_frames(abi_dev):
    """Peak 12: a lexicon that holds the greedy string returns it, with logp within the bound of the specification; a lexicon of strings the
    greedy decode would not give returns the specification's choice."""
    T, C, B, nw = 32, 98, 4, 40
    blank, eos, pad = _symbols(C)
    x, frames = _draw(T, C, B, seed=1232, peak=12.0, bump=4.0)
    greedy_ids, _, greedy_n = S.greedy_decode(x[:, :, :C], blank, -1, pad)      # (eos -1: the collapse with nothing removed)
    rng = random.Random(8)
    pool, begin, want = [], [], []
    for b in range(B):
        g = greedy_ids[b, :int(greedy_n[b])].tolist()
        assert g == _collapse(frames[b].tolist(), blank)
        lex = _lexicon_for(frames[b].tolist(), C, blank, nw, rng, 63)
        begin.append(len(pool))
        want.append(len(pool) + lex.index(g))
        pool += lex
    out, sp = _check(abi_dev, x, C, pool, begin, [nw] * B, min_kept=B, tag="peaked, with the greedy string")
    assert out[0].tolist() == want == sp["best"].tolist()
    assert torch.equal(out[2], torch.where(greedy_ids == -1, torch.full_like(greedy_ids, eos), greedy_ids))
    without = [w for i, w in enumerate(pool) if i not in want]
    begin2 = [b * (nw - 1) for b in range(B)]
    _check(abi_dev, x, C, without, begin2, [nw - 1] * B, min_kept=B, tag="peaked, without it")       # kept: 4 of 4


# ---------------------------------------------------------------------------------------------- 9. host-side validation (no GPU)
@pytest.mark.parametrize("build", ["hip", "cpu_abi"])
def test_ctc_lexicon_entry_point_validates_on_the_host(build):
    """Every error code of dig_ctc_lexicon_decode before any launch, on both builds; a refused call writes nothing; B == 0 and the
    workspace query."""
    from cpu_abi_util import build as build_cpu
    from dig_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH if build == "hip" else build_cpu())
    f, q = lib.dig_ctc_lexicon_decode, lib.dig_ctc_lexicon_workspace_bytes
    f.restype, f.argtypes = ctypes.c_int, L._prototypes()["dig_ctc_lexicon_decode"]
    q.restype, q.argtypes = ctypes.c_longlong, L._prototypes()["dig_ctc_lexicon_workspace_bytes"]
    ARG, UNS, OK = L.const("DIG_ERR_ARG"), L.const("DIG_ERR_UNSUPPORTED"), L.const("DIG_OK")
    ch = L.const("DIG_CTC_LEX_CHUNK")
    assert q(4, 32, 98, 50) == 4 * 1 * 8 + 4 * 32 * 98 * 4 and q(4, 32, 98, ch + 1) == 4 * 2 * 8 + 4 * 32 * 98 * 4
    assert q(4, 32, 98, 0) == 4 * 8 + 4 * 32 * 98 * 4 and q(0, 32, 98, 5) == 0 and q(4, 32, 98, -1) == 0
    assert q(65535, 64, 256, 90000) == 65535 * 1407 * 8 + 65535 * 64 * 256 * 4                  # (above 2^32: a long long)
    poison = 0x5A
    names = ("x", "words", "wl", "lb", "lc", "bi", "logp", "ids", "score", "n", "scores", "ws")
    bufs = {k: (ctypes.c_ubyte * 4096)(*([poison] * 4096)) for k in names}
    p = {k: ctypes.cast(v, ctypes.c_void_p) for k, v in bufs.items()}
    big = 1 << 40

    def dec(**kw):
        a = dict(x=p["x"], ld=128, B=4, T=32, C=98, blank=97, eos=94, pad=95, words=p["words"], wl=p["wl"], ldw=25, W=100, lb=p["lb"], lc=p["lc"],
                 mc=50, bi=p["bi"], logp=p["logp"], ids=p["ids"], score=p["score"], n=p["n"], scores=p["scores"], ws=p["ws"], wsb=big)
        a.update(kw)
        return f(a["x"], a["ld"], a["B"], a["T"], a["C"], a["blank"], a["eos"], a["pad"], a["words"], a["wl"], a["ldw"], a["W"], a["lb"], a["lc"],
                 a["mc"], a["bi"], a["logp"], a["ids"], a["score"], a["n"], a["scores"], a["ws"], a["wsb"], None)

    for k in names:
        if k != "scores":
            assert dec(**{k: None}) == ARG, k
    for kw in ({"B": -1}, {"T": 0}, {"T": -3}, {"C": 0}, {"C": -1}, {"ldw": 0}, {"ldw": -1}, {"ld": 97}, {"ld": 0}, {"blank": 98}, {"blank": -1},
               {"W": -1}, {"mc": -1}, {"wsb": q(4, 32, 98, 50) - 1}, {"wsb": 0}):
        assert dec(**kw) == ARG, kw
    for kw in ({"T": 65}, {"C": 257, "ld": 257}, {"C": 1, "blank": 0, "ld": 1}, {"ldw": 64}, {"B": 65536}):
        assert dec(**kw) == UNS, kw
    ALIGN = L.const("DIG_ERR_ALIGN")                                           # the workspace holds 64-bit keys: 8-byte aligned
    base = ctypes.addressof(bufs["ws"])
    odd = ctypes.c_void_p(base + (4 if base % 8 == 0 else 8 - base % 8 + 4))
    assert odd.value % 8 == 4 and dec(ws=odd) == ALIGN and dec(ws=ctypes.c_void_p(odd.value - 3)) == ALIGN
    assert dec(B=0) == OK and dec(B=0, scores=None, T=64, C=256, ld=256, blank=255, ldw=63, W=0, mc=0, wsb=0) == OK
    assert dec(B=0, eos=-1, pad=10 ** 6) == OK                                 # (eos and padding are any ints)
    assert all(all(v == poison for v in b) for b in bufs.values())


def test_ctc_lexicon_decode_with_nothing_to_score(abi_dev):
    """max_count == 0 (every range empty) and an empty pool are legal: every sample gets -1; the wrapper refuses a range outside the pool."""
    from dig_amd.ctc_recognizer import ctc_lexicon_decode
    T, C, B = 12, 6, 3
    blank, eos, pad = _symbols(C)
    x, _ = _draw(T, C, B, seed=90, peak=5.0, bump=4.0)
    for pool in ([[0, 1], [2]], []):
        best_index, logp, ids, score, n, scores = _run(abi_dev, x, C, pool, [0] * B, [0] * B)
        assert best_index.tolist() == [-1] * B and bool((logp == NINF).all()) and n.tolist() == [0] * B and tuple(scores.shape) == (B, 0)
        assert bool((ids[:, 0] == eos).all()) and bool((ids[:, 1:] == pad).all()) and bool((score[:, 0] == 0).all()) and bool((score[:, 1:] == 1).all())
    for begin, count in (([0, 0, 1], [2, 2, 2]), ([-1, 0, 0], [1, 1, 1]), ([0, 0, 0], [1, -1, 1])):
        with pytest.raises(ValueError, match="outside the pool"):
            ctc_lexicon_decode(x.to(abi_dev), C, blank, eos, pad, _pool_tensors([[0, 1], [2]], abi_dev), begin, count)
    with pytest.raises(ValueError, match="one entry per sample"):
        ctc_lexicon_decode(x.to(abi_dev), C, blank, eos, pad, _pool_tensors([[0, 1], [2]], abi_dev), [0], [1])


def test_ctc_lexicon_kernel_uses_no_scratch():
    from dig_amd import build
    build.build(verbose=False)
    rows = [r for r in build.kernel_resources() if r["name"].startswith("ctc_lex_score_kernel")]
    assert len(rows) == 1 and rows[0]["scratch"] == 0 and rows[0]["hot"], rows


# ---------------------------------------------------------------------------------------------- 10. wiring: LabelLexicon, decode, evaluate()
def test_label_lexicon_rows_order_and_casings():
    from dig_amd.ctc_recognizer import LabelLexicon
    from dig_amd.datasets import find_classes
    voc = find_classes("ALLCASES_SYMBOLS")
    enc = lambda w: [voc.index(c) if c in voc else voc.index("UNKNOWN") for c in w]
    lex = LabelLexicon({"a.png": ["Hello", "AB", "zebra", "ab"], "b.png": ["x"], "c.png": ["Hello", "AB", "zebra", "ab"], "d.png": []})
    assert lex.ranges["a.png"] == lex.ranges["c.png"] and lex.ranges["b.png"][1] == 2 and lex.ranges["d.png"][1] == 0     # x, X
    assert lex.words == ["Hello", "AB", "zebra", "ab", "x"] and lex["a.png"] == ["Hello", "AB", "zebra", "ab"] and len(lex) == 4
    b, c = lex.ranges["a.png"]
    got = [(lex.labels[r, :lex.label_len[r]].tolist(), lex.word_of(r)) for r in range(b, b + c)]
    # shortest first, then first listed (word by word; as written, lower, upper, capitalize, de-duplicated per word)
    want = [("AB", "AB"), ("ab", "AB"), ("Ab", "AB"), ("ab", "ab"), ("AB", "ab"), ("Ab", "ab"),
            ("Hello", "Hello"), ("hello", "Hello"), ("HELLO", "Hello"), ("zebra", "zebra"), ("ZEBRA", "zebra"), ("Zebra", "zebra")]
    assert got == [(enc(f), w) for f, w in want]
    assert lex.word_of(-1) is None and lex.n_rows == 14 and lex.labels.dtype == np.int32
    plain = LabelLexicon(["Hello", "AB"], casings=False)
    assert plain.n_rows == 2 and plain.ranges[None] == (0, 2) and [plain.word_of(r) for r in range(2)] == ["AB", "Hello"]
    low = LabelLexicon(["Hello", "AB", "aé~"], "LOWERCASE")                 # folds; no casings; the accent is no class
    lvoc = find_classes("LOWERCASE")
    rows = [low.labels[r, :low.label_len[r]].tolist() for r in range(low.n_rows)]
    assert rows == [[lvoc.index("a"), lvoc.index("b")], [lvoc.index("a"), lvoc.index("UNKNOWN"), lvoc.index("~")], [lvoc.index(c) for c in "hello"]]
    assert low.nb_classes == len(lvoc) == 71 and lex.nb_classes == 97
    assert LabelLexicon(["a" * 63]).n_rows == 3
    with pytest.raises(ValueError, match="longer than 63 labels.*" + "b" * 64):
        LabelLexicon({"long.png": ["ok", "b" * 64]})
    empty = LabelLexicon([])
    assert empty.n_rows == 0 and empty.ranges[None] == (0, 0) and empty.labels.shape[0] == 1


def _tiny_ctc_model(**kw):
    import dig_oracle as O
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    ecfg = O.DiGConfig(**O.TINY)
    return CTCRecModelTrain(embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads, nb_classes=97, max_len=25, **kw)


def test_ctc_model_takes_its_lexicon_from_the_arguments(tmp_path):
    from dig_amd.ctc_recognizer import CTCRecModelTrain, LabelLexicon
    assert _tiny_ctc_model().ctc_lexicon is None
    lex = LabelLexicon(["one", "two"])
    assert _tiny_ctc_model(ctc_lexicon=lex).ctc_lexicon is lex
    assert _tiny_ctc_model(ctc_lexicon=["one", "two"]).ctc_lexicon.words == ["one", "two"]
    f = tmp_path / "lex.txt"
    f.write_text("one\n\n  two \nthrée\n", encoding="utf-8")
    args = dict(model="simmim_vit_tiny_patch4_32x128", nb_classes=97, max_len=25, drop=0.0, attn_drop_rate=0.0, drop_path=0.0)
    m = CTCRecModelTrain(types.SimpleNamespace(ctc_lexicon=str(f), voc_type="ALLCASES_SYMBOLS", **args))
    assert m.ctc_lexicon.words == ["one", "two", "thrée"] and m.ctc_lexicon.voc_type == "ALLCASES_SYMBOLS"
    assert CTCRecModelTrain(types.SimpleNamespace(**args)).ctc_lexicon is None
    with pytest.raises(ValueError, match="ctc_beam_width"):
        _tiny_ctc_model(ctc_lexicon=lex, ctc_beam_width=4)
    with pytest.raises(ValueError, match="one flat list"):
        _tiny_ctc_model(ctc_lexicon=LabelLexicon({"a": ["x"]}))
    with pytest.raises(ValueError, match="71 classes"):
        _tiny_ctc_model(ctc_lexicon=LabelLexicon(["x"], "LOWERCASE"))


_WIRE = {}


def _wiring():
    """8 samples at the recipe shape, one flat lexicon of words over the ALLCASES_SYMBOLS vocabulary: every sample's collapse (without EOS /
    PADDING / UNKNOWN labels), edits of it and random words, as strings; the specification's choice per sample."""
    if not _WIRE:
        from dig_amd.ctc_recognizer import LabelLexicon
        from dig_amd.datasets import find_classes
        T, C, B = 32, 98, 8
        voc = find_classes("ALLCASES_SYMBOLS")
        blank, eos, pad = C - 1, voc.index("EOS"), voc.index("PADDING")
        x, frames = _draw(T, C, B, seed=3298, peak=5.0, bump=4.0)
        x = x[:, :, :C].contiguous()
        x[:, :, eos:blank] -= 30.0                                              # (words are made of characters)
        rng = random.Random(10)
        words = []
        for b in range(B):
            for w in _lexicon_for(x[b].argmax(-1).tolist(), eos, blank, 12, rng, 20):
                s = "".join(voc[c] for c in w if c < eos)
                if s and s not in words:
                    words.append(s)
        lex = LabelLexicon(words, casings=False)
        pool = [lex.labels[r, :lex.label_len[r]].tolist() for r in range(lex.n_rows)]
        sp = _spec(x, pool, [0] * B, [lex.n_rows] * B, blank)
        assert bool((sp["gap"] >= sp["G"]).all()), sp["gap"]
        ids, n = LM.rows(sp["best"], pool, T, eos, pad)
        _WIRE.update(T=T, C=C, B=B, voc=voc, x=x, lex=lex, pool=pool, sp=sp, ids=ids, n=n, sym=(blank, eos, pad))
    return _WIRE


def test_ctc_lexicon_reaches_decode_and_evaluate(abi_dev):
    from dig_amd import recognizer
    from dig_amd.ctc_recognizer import ctc_greedy_decode
    from dig_amd.engine_for_finetuning import evaluate
    w = _wiring()
    T, C, B, voc, x, lex = w["T"], w["C"], w["B"], w["voc"], w["x"], w["lex"]
    blank, eos, pad = w["sym"]
    xd = x.to(abi_dev)
    # ---- the model's decode: the lexicon in eval mode, greedy while training and when a width is named
    m = _tiny_ctc_model(ctc_lexicon=lex)
    assert (m.blank, m.eos, m.padding) == (blank, eos, pad) and m.training
    want_greedy = ctc_greedy_decode(xd, C, blank, eos, pad)
    for got in (m.decode(xd), m.decode(xd, beam_width=0), m.eval().decode(xd, beam_width=0)):
        assert len(got) == 3 and all(torch.equal(a.cpu().view(torch.uint8), b_.cpu().view(torch.uint8)) for a, b_ in zip(got, want_greedy))
    ids, score, n = m.eval().decode(xd)
    assert torch.equal(ids.cpu(), w["ids"]) and torch.equal(n.cpu().long(), w["n"]) and bool((score[:, 1:] == 1.0).all())
    assert bool(((score[:, 0].cpu().double() - torch.exp(w["sp"]["logp"])).abs() <= 1e-3 * torch.exp(w["sp"]["logp"]) + 2.0 ** -149).all())
    assert not torch.equal(ids.cpu(), want_greedy[0].cpu())                    # (the lexicon corrects something)
    # ---- evaluate(): targets = the specification's rows for the even samples, a neighbour's for the odd ones
    target, lens = w["ids"].clone(), w["n"] + 1
    target[1::2], lens[1::2] = w["ids"][0::2], (w["n"] + 1)[0::2]
    split = ((0, 3), (3, B))
    batches = [(torch.zeros(hi - lo, 3, 32, 128), target[lo:hi], lens[lo:hi]) for lo, hi in split]
    loader = type("Loader", (list,), {})(batches)
    loader.dataset = types.SimpleNamespace(idx_to_class={i: c for i, c in enumerate(voc)})

    class Stub:
        """What evaluate() reads of a CTC model, with fixed logits per batch and `decode` the real method."""
        is_ctc, beam_width, ctc_beam_width = True, 0, 0

        def __init__(self, lexicon):
            from dig_amd.ctc_recognizer import CTCRecModelTrain
            self.i, self.blank, self.eos, self.padding, self.ctc_lexicon, self.training = 0, blank, eos, pad, lexicon, True
            self.decode = types.MethodType(CTCRecModelTrain.decode, self)

        def eval(self):
            self.training = False
            return self

        def __call__(self, batch):
            lo, hi = split[self.i]
            self.i += 1
            return x[lo:hi].to(batch[0].device), None, None, None

    args = types.SimpleNamespace(beam_width=0, ctc_lexicon="lexicon.txt")
    with_lex = evaluate(loader, Stub(lex), abi_dev, args)
    greedy = evaluate(loader, Stub(None), abi_dev, args)
    want = sum(float(recognizer.accuracy(w["ids"][lo:hi].to(abi_dev), target[lo:hi].to(abi_dev), voc)) * (hi - lo) for lo, hi in split) / B
    assert 0.0 < want < 1.0 and with_lex["acc"] == want and greedy["acc"] != want
    assert sorted(with_lex) == sorted(greedy) == ["acc", "loss", "recognition_fmeasure"]
    assert with_lex["loss"] == greedy["loss"] and math.isfinite(with_lex["loss"])


# ---------------------------------------------------------------------------------------------- 11. the two metric functions
def test_ctc_metrics_with_lexicon(abi_dev):
    """6 samples, per-image lexicons of 3 to 70 words (one of them upper case), against a host model: the specification's choice per image,
    its raw word normalised, python's edit distance to the normalised target."""
    from dig_amd import evaluation_metric as EM
    from dig_amd.ctc_recognizer import LabelLexicon
    w = _wiring()
    T, C, voc, lexall = w["T"], w["C"], w["voc"], w["lex"]
    blank, eos, pad = w["sym"]
    B = 6
    x = w["x"][:B]
    names = [f"img{b}.png" for b in range(B)]
    chosen = [lexall.word_of(int(r)) for r in w["sp"]["best"][:B]]
    others = [s for s in lexall.words if s not in chosen]
    sizes = [3, 70, 10, 5, 33, 64]
    rng = random.Random(11)
    by_name = {}
    for b in range(B):
        lst = rng.sample(others, min(sizes[b] - 1, len(others)))
        lst.insert(rng.randrange(len(lst) + 1), chosen[b])
        by_name[names[b]] = lst
    by_name[names[2]] = [s.upper() for s in by_name[names[2]]]                # an upper-case benchmark lexicon
    small = {k: v[:3] if chosen[i] in v[:3] or i == 2 else [chosen[i]] + v[:2] for i, (k, v) in enumerate(by_name.items())}
    target, lens = w["ids"][:B].clone(), (w["n"][:B] + 1)
    target[5], lens[5] = w["ids"][6], w["n"][6] + 1                            # one target that the lexicon of its image does not hold
    ds = types.SimpleNamespace(idx_to_class={i: c for i, c in enumerate(voc)}, lexicons50=small, lexicons1k=by_name,
                               lexiconsfull={k: [] for k in names})           # the third level: an empty first lexicon reports 0

    def lev(a, b_):
        d = list(range(len(b_) + 1))
        for i, ca in enumerate(a, 1):
            p, d[0] = d[0], i
            for j, cb in enumerate(b_, 1):
                p, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, p + (ca != cb))
        return d[-1]

    norm = EM._normalize_text
    tstr = ["".join(voc[c] for c in target[b, :int(lens[b]) - 1].tolist()) for b in range(B)]
    greedy_ids, _, greedy_n = S.greedy_decode(x, blank, eos, pad)
    gstr = ["".join(voc[c] for c in greedy_ids[b, :int(greedy_n[b])].tolist() if voc[c] != "UNKNOWN") for b in range(B)]
    want = {"none": [lev(norm(g), norm(t)) for g, t in zip(gstr, tstr)]}
    for level, d in (("lexicons50", small), ("lexicons1k", by_name)):
        host = LabelLexicon(d)
        dist = []
        for b in range(B):
            beg, cnt = host.ranges[names[b]]
            pool = [host.labels[r, :host.label_len[r]].tolist() for r in range(beg, beg + cnt)]
            s64 = LM.word_scores(x[b], pool, blank)
            top = s64.sort(descending=True).values
            assert float(top[0] - top[1]) >= w["sp"]["G"]                      # (the gap rule on this lexicon)
            dist.append(lev(norm(host.word_of(beg + int(s64.argmax()))), norm(tstr[b])))
        want[level] = dist
    xd, td = x.to(abi_dev), target.to(abi_dev)
    acc = EM.CTCAccuracy_with_lexicon(xd, td, ds, names)
    ed = EM.CTCEditDistance_with_lexicon(xd, td, ds, names)
    assert acc == [sum(v == 0 for v in want[k]) / B for k in ("none", "lexicons50", "lexicons1k")] + [0]
    assert ed == [sum(want[k]) for k in ("none", "lexicons50", "lexicons1k")] + [0]
    assert want["lexicons1k"][2] == 0 and acc[2] >= 5 / 6 > acc[0]            # the upper-case lexicon word counts; the lexicon corrects
    assert EM.CTCAccuracy_with_lexicon(xd, td, ds, []) == [acc[0], 0, 0, 0]    # no file names: the levels report 0
    ds.lexiconsfull = dict(by_name, **{names[3]: []})                          # an empty lexicon further down raises
    with pytest.raises(ValueError, match="empty sequence.*lexiconsfull.*img3"):
        EM.CTCEditDistance_with_lexicon(xd, td, ds, names)
    assert "ctc_accuracy_with_lexicon" not in EM.factory() and len(EM.factory()) == 5


# ---------------------------------------------------------------------------------------------- 12. the driver
from test_finetune_driver import COMMON, _driver  # noqa: E402

CTC = COMMON + " --decoder_type ctc"


def test_driver_ctc_lexicon_flag(tmp_path):
    drv = _driver()
    f, empty = tmp_path / "words.txt", tmp_path / "empty.txt"
    f.write_text("hello\n\nworld\n", encoding="utf-8")
    empty.write_text("\n \n", encoding="utf-8")
    assert drv.get_args(CTC.split()).ctc_lexicon is None and drv.get_args(COMMON.split()).ctc_lexicon is None
    args = drv.get_args((CTC + f" --ctc_lexicon {f}").split())
    assert args.ctc_lexicon == str(f) and args.ctc_beam_width == 0 and args.decoder_type == "ctc"
    for other in (COMMON, COMMON + " --decoder_type attention"):
        with pytest.raises(SystemExit, match="--ctc_lexicon with --decoder_type.*--decoder_type ctc"):
            drv.get_args((other + f" --ctc_lexicon {f}").split())
    with pytest.raises(SystemExit, match="--ctc_lexicon with --ctc_beam_width"):
        drv.get_args((CTC + f" --ctc_lexicon {f} --ctc_beam_width 4").split())
    with pytest.raises(SystemExit, match="no such file"):
        drv.get_args((CTC + f" --ctc_lexicon {tmp_path / 'missing.txt'}").split())
    with pytest.raises(SystemExit, match="holds no word"):
        drv.get_args((CTC + f" --ctc_lexicon {empty}").split())
    assert "--ctc_lexicon" in drv.__doc__
