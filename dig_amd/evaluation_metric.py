"""The reference's `evaluation_metric` package on the device: same keys, signatures and return types, quirks included.

    from dig_amd import evaluation_metric
    evaluation_metric.factory()["editdistance_with_lexicon"](output, target, dataset, file_names)

`output` / `target` are [B, T] tensors of class ids on the device the library runs on; `dataset` gives the vocabulary the way
`engine_for_finetuning._vocabulary` reads it (`idx_to_class` or `voc`) and, for the lexicon metrics, `lexicons50`, `lexicons1k` and
`lexiconsfull`: `Lexicon` objects, or plain {file name: [words]} dicts that are wrapped (and cached on the dataset) on first use.

What runs where: the strings never leave the device.  `dig_tokens_to_text` normalises both label tensors (get_str_list, metrics.py:19-64),
`dig_lexicon_search` finds each prediction's nearest lexicon word (one launch for the batch, whatever the lexicon size), `dig_edit_distance`
compares pairs, `dig_seq_confidence` gives RecPostProcess's score; every function reads its results back in one copy.

Mirrored literally from metrics.py:103-186: the search compares NORMALISED lexicon words with the normalised prediction but returns the RAW
word; accuracy then tests raw word == normalised target (a lexicon word with an upper-case letter or punctuation never counts as correct) and
the edit distance is taken between the raw word and the normalised target; a lexicon level reports 0 when `file_names` is empty or the
lexicon of `file_names[0]` is empty -- only the first file name is looked at, and an empty lexicon further down raises as np.argmin does.

`ctc_get_str_list` and `CTCAccuracy` (metrics.py:205-251) are module functions with the reference's signatures: `output` is the per-frame
arg-max [B, T] of the CTC head (dig_amd/ctc_recognizer.py), collapsed by the device rule of `dig_ctc_greedy_decode` into decoder-shaped rows,
which `dig_string_match` / `dig_tokens_to_text` then read like any other prediction; a target narrower than T + 1 is padded with PADDING.

`CTCAccuracy_with_lexicon` and `CTCEditDistance_with_lexicon` are this project's own (no `factory()` keys: the reference has no such metric):
they take the CTC head's logits and decode each image to the lexicon word of highest likelihood (`dig_ctc_lexicon_decode`, one launch per
lexicon level) where the mirrored lexicon metrics snap a decoded string to the nearest word; they compare normalised with normalised.
`CTCAlignment` is own as well: it turns the forced alignment of the CTC head (`dig_ctc_align`) into one record per image, the character
boxes in crop columns with a log-probability per character.

Two keys of the reference's factory are left out of `factory()`: `ctc_accuracy` (the function is here, as `CTCAccuracy`; the five keys are what
the reference's fine-tune path can reach) and `multi_label_fmeasure` (no model emits multi-label outputs; not built)."""
import string

import numpy as np
import torch

from . import _lib as L
from . import recognizer

MAX_WORD_LEN = L.const("DIG_LEV_MAX_LEN")
CHUNK = L.const("DIG_LEXICON_CHUNK")    # words per workgroup of the search
_KEEP = string.digits + string.ascii_letters


def _normalize_text(text):
    """metrics.py:14-16."""
    return "".join(c for c in text if c in _KEEP).lower()


# ---------------------------------------------------------------------------------------------- device operators
def tokens_to_text(tokens, voc):
    """Normalised strings of [B, T] class ids: (text int32 [B, T] code points, length int32 [B])."""
    B, T = tokens.shape
    dev = tokens.device
    tok, canon = tokens.long().contiguous(), recognizer.class_canon(voc).to(dev)
    text = torch.empty((B, T), device=dev, dtype=torch.int32)
    length = torch.empty(B, device=dev, dtype=torch.int32)
    L.call("dig_tokens_to_text", L.ptr(tok), L.ptr(canon), len(voc), voc.index("EOS"), B, T, L.ptr(text), L.ptr(length), L.stream())
    return text, length


def edit_distance(a, a_len, b, b_len, a_index=None):
    """Levenshtein distance of n pairs of device strings (int32 rows + int32 lengths): dist int32 [n] = d(a[a_index[i]] or a[i], b[i])."""
    n = b.shape[0]
    dist = torch.empty(n, device=b.device, dtype=torch.int32)
    L.call("dig_edit_distance", L.ptr(a), L.ptr(a_len), a.shape[1], a.shape[0], L.ptr(a_index), L.ptr(b), L.ptr(b_len), b.shape[1], n,
           L.ptr(dist), L.stream())
    return dist


def lexicon_search_workspace_bytes(B, max_count):
    return L.query("dig_lexicon_search_workspace_bytes", B, max_count)


def lexicon_search(query, query_len, words, word_len, lex_begin, lex_count):
    """For each query row the first nearest word of pool rows [lex_begin[b], lex_begin[b] + lex_count[b]): (best_index, best_dist), int32 [B],
    both -1 for an empty range.  lex_begin / lex_count are host sequences; a range outside the pool is refused here, before upload."""
    B, W = query.shape[0], words.shape[0]
    begin, count = np.asarray(lex_begin, dtype=np.int64).reshape(-1), np.asarray(lex_count, dtype=np.int64).reshape(-1)
    if begin.shape != (B,) or count.shape != (B,):
        raise ValueError(f"lex_begin / lex_count need one entry per query ({B})")
    bad = np.nonzero((begin < 0) | (count < 0) | (begin + count > W))[0]
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"lexicon range of query {b} ([{int(begin[b])}, {int(begin[b] + count[b])})) is outside the pool of {W} words")
    dev = query.device
    max_count = int(count.max())
    ranges = torch.from_numpy(np.stack([begin, count]).astype(np.int32)).to(dev)
    ws_bytes = lexicon_search_workspace_bytes(B, max_count)
    ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.int64)
    best_index = torch.empty(B, device=dev, dtype=torch.int32)
    best_dist = torch.empty(B, device=dev, dtype=torch.int32)
    L.call("dig_lexicon_search", L.ptr(query), L.ptr(query_len), query.shape[1], B, L.ptr(words), L.ptr(word_len), words.shape[1], W,
           L.ptr(ranges[0]), L.ptr(ranges[1]), max_count, L.ptr(best_index), L.ptr(best_dist), L.ptr(ws), ws_bytes, L.stream())
    return best_index, best_dist


def seq_confidence(score, text_len):
    """RecPostProcess's score per row (metrics.py:195-200): float64 [B] from score [B, T] fp32 and the normalised lengths."""
    B, T = score.shape
    sc, tl = score.float().contiguous(), text_len.to(torch.int32).contiguous()
    conf = torch.empty(B, device=score.device, dtype=torch.float64)
    L.call("dig_seq_confidence", L.ptr(sc), L.ptr(tl), B, T, L.ptr(conf), L.stream())
    return conf


def edit_distances(pred_tokens, target_tokens, voc):
    """Per-sample edit distance of the normalised strings of two [B, T] label tensors: int32 [B] on the device (no host read)."""
    p, pl = tokens_to_text(pred_tokens, voc)
    t, tl = tokens_to_text(target_tokens.to(pred_tokens.device), voc)
    return edit_distance(p, pl, t, tl)


# ---------------------------------------------------------------------------------------------- lexicons
def _pool(words):
    n, ld = max(len(words), 1), max([len(w) for w in words] + [1])
    rows, lens = np.zeros((n, ld), dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i, w in enumerate(words):
        rows[i, :len(w)] = [ord(c) for c in w]
        lens[i] = len(w)
    return rows, lens


class Lexicon:
    """Host preparation of a lexicon set {name: [words]}, done once: the RAW words and their `_normalize_text` as code-point rows with
    lengths, in two pools indexed alike, and per name a range (begin, count) into them.  Identical lists are stored once and share their
    range.  `device(dev)` uploads once per device.  `lex[name]` is the list of raw words, as in the reference's dicts."""

    def __init__(self, words_by_name):
        self.ranges, self._lists = {}, {}
        raw, seen = [], {}
        for name, words in words_by_name.items():
            key = tuple(words)
            r = seen.get(key)
            if r is None:
                for w in key:
                    if len(w) > MAX_WORD_LEN:
                        raise ValueError(f"lexicon word longer than {MAX_WORD_LEN} code points ({len(w)}) in {name!r}: {w!r}")
                r = seen[key] = (len(raw), len(key), list(key))
                raw.extend(key)
            self.ranges[name] = r[:2]
            self._lists[name] = r[2]
        self.words = raw
        self.n_words = len(raw)
        self.raw, self.raw_len = _pool(raw)
        self.norm, self.norm_len = _pool([_normalize_text(w) for w in raw])
        self._dev = {}

    def __getitem__(self, name):
        return self._lists[name]

    def __contains__(self, name):
        return name in self._lists

    def __len__(self):
        return len(self._lists)

    def keys(self):
        return self._lists.keys()

    def device(self, dev):
        """(raw, raw_len, norm, norm_len) on `dev`."""
        dev = torch.device(dev)
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = tuple(torch.from_numpy(a).to(dev) for a in (self.raw, self.raw_len, self.norm, self.norm_len))
        return t


def _lexicon(dataset, attr):
    lex = getattr(dataset, attr)
    if isinstance(lex, Lexicon):
        return lex
    cache = getattr(dataset, "_dig_lexicons", None)
    if cache is None:
        cache = {}
        setattr(dataset, "_dig_lexicons", cache)
    ent = cache.get(attr)
    if ent is None or ent[0] is not lex:
        ent = cache[attr] = (lex, Lexicon(lex))
    return ent[1]


def _voc(dataset):
    from .engine_for_finetuning import _vocabulary
    return _vocabulary(dataset)


_LEVELS = ("lexicons50", "lexicons1k", "lexiconsfull")


def _with_lexicon(output, target, dataset, file_names):
    """Per level None (the reference reports 0) or the int32 [n] distances between the chosen RAW word and the normalised target, then
    the no-lexicon distances [B]; all read back in one copy.  n = min(len(file_names), B), as the reference's zip() cuts."""
    voc = _voc(dataset)
    pred, pred_len = tokens_to_text(output, voc)
    targ, targ_len = tokens_to_text(target.to(output.device), voc)
    parts = [edit_distance(pred, pred_len, targ, targ_len)]
    n = min(len(file_names), pred.shape[0])
    used = []
    for attr in _LEVELS:
        if len(file_names) == 0:
            continue
        lex = _lexicon(dataset, attr)
        if len(lex[file_names[0]]) == 0:
            continue
        rng = [lex.ranges[f] for f in file_names[:n]]
        empty = [f for f, r in zip(file_names[:n], rng) if r[1] == 0]
        if empty:
            raise ValueError(f"attempt to get argmin of an empty sequence: the {attr} lexicon of {empty[0]!r} is empty")
        raw, raw_len, norm, norm_len = lex.device(pred.device)
        best, _ = lexicon_search(pred[:n], pred_len[:n], norm, norm_len, [r[0] for r in rng], [r[1] for r in rng])
        parts.append(edit_distance(raw, raw_len, targ[:n], targ_len[:n], a_index=best))
        used.append(attr)
    vals = torch.cat(parts).tolist()
    B = pred.shape[0]
    out = {"none": vals[:B]}
    for i, attr in enumerate(used):
        out[attr] = vals[B + i * n:B + (i + 1) * n]
    return out


# ---------------------------------------------------------------------------------------------- the reference's functions
def Accuracy(output, target, dataset=None):
    return float(recognizer.accuracy(output, target, _voc(dataset)).double().item())


def recognition_f_measure(output, target, dataset=None):
    return float(recognizer.recognition_f_measure(output, target, _voc(dataset)).item())


def EditDistance(output, target, dataset=None):
    return int(edit_distances(output, target, _voc(dataset)).sum().item())


def Accuracy_with_lexicon(output, target, dataset=None, file_names=None):
    d = _with_lexicon(output, target, dataset, file_names)
    return [1.0 * sum(v == 0 for v in d[k]) / len(d[k]) if k in d else 0 for k in ("none",) + _LEVELS]


def EditDistance_with_lexicon(output, target, dataset=None, file_names=None):
    d = _with_lexicon(output, target, dataset, file_names)
    return [sum(d[k]) if k in d else 0 for k in ("none",) + _LEVELS]


def RecPostProcess(output, target, score, dataset=None):
    voc = _voc(dataset)
    pred, pred_len = tokens_to_text(output, voc)
    targ, targ_len = tokens_to_text(target.to(output.device), voc)
    conf = seq_confidence(score.to(output.device), pred_len)
    B, T = pred.shape
    host = torch.cat([pred.reshape(-1).double(), pred_len.double(), targ.reshape(-1).double(), targ_len.double(), conf]).tolist()
    p, pl, t, tl, c = host[:B * T], host[B * T:B * T + B], host[B * T + B:2 * B * T + B], host[2 * B * T + B:2 * B * T + 2 * B], host[2 * B * T + 2 * B:]
    strs = lambda cells, lens: ["".join(chr(int(v)) for v in cells[b * T:b * T + int(lens[b])]) for b in range(B)]
    return strs(p, pl), strs(t, tl), c


def _ctc_rows(output, target, dataset):
    """The per-frame arg-max [B, T] of a CTC head as decoder-shaped rows: the device rule of dig_ctc_greedy_decode (csrc/ctc.hip) on
    one-hot logits over len(voc) + 1 classes (blank = len(voc), metrics.py:211), and the targets at the same width (padded with PADDING on
    the host side).  Returns (ids, targets, voc)."""
    from .ctc_recognizer import ctc_greedy_decode, match_widths
    assert output.dim() == 2 and target.dim() == 2 and output.shape[0] == target.shape[0]
    voc = _voc(dataset)
    C = len(voc) + 1
    frames = output.long()
    if bool(((frames < 0) | (frames >= C)).any()):
        raise ValueError(f"frame classes outside [0, {C}): the blank is class {C - 1}")
    onehot = torch.zeros(frames.shape + (C,), device=frames.device, dtype=torch.float32)
    onehot.scatter_(2, frames.unsqueeze(-1), 1.0)
    ids, _, _ = ctc_greedy_decode(onehot, C, C - 1, voc.index("EOS"), voc.index("PADDING"))
    ids, targ = match_widths(ids, target, voc.index("PADDING"))
    return ids, targ, voc


def ctc_get_str_list(output, target, dataset=None):
    """metrics.py:205-244: (pred_list, targ_list) of normalised strings; `output` = the per-frame arg-max [B, T] of a CTC head."""
    ids, targ, voc = _ctc_rows(output, target, dataset)
    pred, pred_len = tokens_to_text(ids, voc)
    t, t_len = tokens_to_text(targ, voc)
    B, T = pred.shape
    host = torch.cat([pred.reshape(-1), pred_len, t.reshape(-1), t_len]).tolist()                      # the one host read
    p, pl, tt, tl = host[:B * T], host[B * T:B * T + B], host[B * T + B:2 * B * T + B], host[2 * B * T + B:]
    strs = lambda cells, lens: ["".join(chr(int(v)) for v in cells[b * T:b * T + int(lens[b])]) for b in range(B)]
    return strs(p, pl), strs(tt, tl)


def CTCAccuracy(output, target, dataset=None):
    """metrics.py:246-251."""
    ids, targ, voc = _ctc_rows(output, target, dataset)
    B, T = ids.shape
    canon = recognizer.class_canon(voc).to(ids.device)
    match = torch.empty(B, device=ids.device, dtype=torch.uint8)
    ids, targ = ids.contiguous(), targ.contiguous()
    L.call("dig_string_match", L.ptr(ids), L.ptr(targ), L.ptr(canon), len(voc), voc.index("EOS"), B, T, L.ptr(match), L.stream())
    return 1.0 * int(match.sum().item()) / B                                   # (the count divided on the host, in double as the reference does)


def _label_lexicon(dataset, attr, voc):
    """The `LabelLexicon` of a lexicon level of `dataset` (built and cached on first use, like `_lexicon`) with, beside it, the normalised
    raw words as a code-point pool."""
    from .ctc_recognizer import LabelLexicon, _VOC_BY_CLASSES
    lex = getattr(dataset, attr)
    if not isinstance(lex, LabelLexicon):
        cache = getattr(dataset, "_dig_label_lexicons", None)
        if cache is None:
            cache = {}
            setattr(dataset, "_dig_label_lexicons", cache)
        ent = cache.get(attr)
        if ent is None or ent[0] is not lex:
            voc_type = getattr(dataset, "voc_type", None) or _VOC_BY_CLASSES.get(len(voc))
            if voc_type is None:
                raise ValueError(f"no vocabulary type has {len(voc)} classes: give the dataset a `voc_type` or `LabelLexicon` levels")
            ent = cache[attr] = (lex, LabelLexicon(lex, voc_type))
        lex = ent[1]
    return lex


def _ctc_with_lexicon(logits, target, dataset, file_names):
    """`_with_lexicon` for a CTC head's logits [B, T, len(voc) + 1]: per level None or the int32 [n] distances between the NORMALISED
    chosen raw word and the normalised target, then the greedy collapse's distances [B]; all read back in one copy."""
    from .ctc_recognizer import ctc_greedy_decode, ctc_lexicon_decode
    voc = _voc(dataset)
    C = len(voc) + 1
    assert logits.dim() == 3 and logits.shape[2] == C, f"logits [B, T, {C}] (the blank is class {C - 1})"
    x = logits.detach().float().contiguous()
    dev = x.device
    blank, eos, padding = C - 1, voc.index("EOS"), voc.index("PADDING")
    pred, pred_len = tokens_to_text(ctc_greedy_decode(x, C, blank, eos, padding)[0], voc)
    targ, targ_len = tokens_to_text(target.to(dev), voc)
    B = x.shape[0]
    parts = [edit_distance(pred, pred_len, targ, targ_len)]
    n = min(len(file_names), B)
    used = []
    for attr in _LEVELS:
        if len(file_names) == 0:
            continue
        lex = _label_lexicon(dataset, attr, voc)
        if len(lex[file_names[0]]) == 0:
            continue
        rng = [lex.ranges[f] for f in file_names[:n]]
        empty = [f for f, r in zip(file_names[:n], rng) if r[1] == 0]
        if empty:
            raise ValueError(f"attempt to get argmax of an empty sequence: the {attr} lexicon of {empty[0]!r} is empty")
        best = ctc_lexicon_decode(x[:n], C, blank, eos, padding, lex, [r[0] for r in rng], [r[1] for r in rng])[0]
        norm, norm_len, row_word = lex.normalized_words(dev)
        word = torch.where(best >= 0, row_word[best.clamp(min=0).long()], torch.full_like(best, -1))     # (-1, no word: the empty string)
        parts.append(edit_distance(norm, norm_len, targ[:n].contiguous(), targ_len[:n].contiguous(), a_index=word.contiguous()))
        used.append(attr)
    vals = torch.cat(parts).tolist()                                                                       # the one host read
    out = {"none": vals[:B]}
    for i, attr in enumerate(used):
        out[attr] = vals[B + i * n:B + (i + 1) * n]
    return out


def CTCAccuracy_with_lexicon(logits, target, dataset=None, file_names=None):
    """[none, lexicons50, lexicons1k, lexiconsfull] accuracies of a CTC head's `logits` [B, T, len(voc) + 1]: `none` is the greedy
    collapse; a level decodes image i to the most probable word of the lexicon of file_names[i] (one dig_ctc_lexicon_decode launch per
    level, casings as `LabelLexicon` adds them).  The reference has no such metric, and the comparison is this project's own: the
    NORMALISED chosen raw word against the normalised target (the reference's lexicon functions, mirrored in `Accuracy_with_lexicon`,
    compare the raw word, so an upper-case lexicon word is never correct there).  Its conventions are kept: a level reports 0 when
    `file_names` is empty or the lexicon of file_names[0] is empty; an empty lexicon further down raises."""
    d = _ctc_with_lexicon(logits, target, dataset, file_names if file_names is not None else [])
    return [1.0 * sum(v == 0 for v in d[k]) / len(d[k]) if k in d else 0 for k in ("none",) + _LEVELS]


def CTCEditDistance_with_lexicon(logits, target, dataset=None, file_names=None):
    """The summed edit distances of the same decodes (see `CTCAccuracy_with_lexicon`): [none, lexicons50, lexicons1k, lexiconsfull]."""
    d = _ctc_with_lexicon(logits, target, dataset, file_names if file_names is not None else [])
    return [sum(d[k]) if k in d else 0 for k in ("none",) + _LEVELS]


class CTCAlignment:
    """Records of the CTC head's forced alignment (`dig_ctc_align`; `CTCRecModelTrain.align`), this project's own (no `factory()` key):
    `CTCAlignment(dataset)(rows, n, start, end, char_logp, path_logp)` -> one dict per image,
        {"text": str, "path_logp": float, "chars": [[char, x0, x1, logp], ...]}
    from the label rows [B, >= ldt] that were aligned, their label counts n [B] (without EOS) and the four outputs of the alignment.
    Character k covers the crop columns [x0, x1) = [start * frame_columns, end * frame_columns) and has the log-probability logp on them;
    `text` is the concatenation of the characters.  A class id is turned into its character by the dataset's vocabulary, the rule
    `dig_tokens_to_text` / `RecPostProcess` start from, but nothing is normalised away, since every label has a box: punctuation and case
    stay, and a class that is no character (UNKNOWN; EOS or PADDING inside a row) reads U+FFFD.  An image without an alignment
    (path_logp -inf) has `path_logp` None and no `chars`; its `text` is still the row's.  One host read per call."""
    NO_CHAR = "\ufffd"

    def __init__(self, dataset, frame_columns=4):
        self.voc = [c if len(c) == 1 else self.NO_CHAR for c in _voc(dataset)]
        self.frame_columns = int(frame_columns)

    def strings(self, rows, n):
        """The rows' first n[b] labels as strings by the same rule (the ground-truth word of a record).  One host read."""
        host = torch.cat([rows, n.to(rows.device).reshape(-1, 1).to(rows.dtype)], dim=1).tolist()
        voc = self.voc
        return ["".join(voc[c] if 0 <= c < len(voc) else self.NO_CHAR for c in r[:max(0, min(r[-1], len(r) - 1))]) for r in host]

    def __call__(self, rows, n, start, end, char_logp, path_logp):
        B, ldt = start.shape
        dev = start.device
        parts = [rows.to(dev)[:, :ldt], n.to(dev).reshape(B, 1), start, end, char_logp, path_logp.reshape(B, 1)]
        host = torch.cat([p.double() for p in parts], dim=1).tolist()
        voc, fc, out = self.voc, self.frame_columns, []
        for r in host:
            k = max(0, min(int(r[ldt]), ldt))
            ids, st, en, lp, path = r[:k], r[ldt + 1:], r[2 * ldt + 1:], r[3 * ldt + 1:], r[4 * ldt + 1]
            chars = [voc[int(c)] if 0 <= int(c) < len(voc) else self.NO_CHAR for c in ids]
            if path == float("-inf"):
                out.append({"text": "".join(chars), "path_logp": None, "chars": []})
            else:
                out.append({"text": "".join(chars), "path_logp": path,
                            "chars": [[chars[i], int(st[i]) * fc, int(en[i]) * fc, lp[i]] for i in range(k)]})
        return out


__factory = {
    'accuracy': Accuracy,
    'editdistance': EditDistance,
    'accuracy_with_lexicon': Accuracy_with_lexicon,
    'editdistance_with_lexicon': EditDistance_with_lexicon,
    'recognition_fmeasure': recognition_f_measure,
}


def names():
    return sorted(__factory.keys())


def factory():
    return __factory
