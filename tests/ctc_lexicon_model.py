"""The specification of the CTC lexicon decode (dig_ctc_lexicon_decode, include/dig_hip.h) in plain torch: test infrastructure, like
tests/ctc_model.py and tests/ctc_beam_model.py.

  s(b, w) = log p(labels_w | frames of b) = -F.ctc_loss(log_softmax(x_b), labels_w, reduction="none", zero_infinity=False), taken at
  float64 or float32; -inf for a word that holds a label outside [0, C) or equal to the blank (no index is formed from it), for a word
  without an alignment (torch reports inf) and for a probability that is no number.  The chosen word is the first largest s of the
  sample's range; a range that is empty or all -inf chooses -1."""
import torch
import torch.nn.functional as TF


def word_scores(x, words, blank, dtype=torch.float64):
    """x [T, C] logits of one sample, words: a list of label lists.  Returns s [len(words)] in `dtype`."""
    T, C = x.shape
    n = len(words)
    out = torch.full((n,), float("-inf"), dtype=dtype)
    usable = [i for i, w in enumerate(words) if all(0 <= l < C and l != blank for l in w)]
    if not usable:
        return out
    ld = max([len(words[i]) for i in usable] + [1])
    tgt = torch.full((len(usable), ld), (blank + 1) % C, dtype=torch.int64)
    lens = torch.zeros(len(usable), dtype=torch.int64)
    for j, i in enumerate(usable):
        tgt[j, :len(words[i])] = torch.tensor(words[i], dtype=torch.int64)
        lens[j] = len(words[i])
    lp = TF.log_softmax(x.to(dtype), -1).unsqueeze(1).expand(T, len(usable), C)
    nll = TF.ctc_loss(lp, tgt, torch.full((len(usable),), T, dtype=torch.int64), lens, blank=blank, reduction="none", zero_infinity=False)
    s = -nll
    s = torch.where(torch.isfinite(s), s, torch.full_like(s, float("-inf")))
    out[torch.tensor(usable)] = s
    return out


def lexicon_scores(x, pool, begin, count, blank, dtype=torch.float64):
    """x [B, T, C]; pool: a list of label lists; sample b is scored against pool[begin[b] : begin[b] + count[b]].
    Returns scores [B, max(count)] (-inf past a range) in `dtype`."""
    B = x.shape[0]
    mc = max([int(c) for c in count] + [0])
    out = torch.full((B, mc), float("-inf"), dtype=dtype)
    for b in range(B):
        k = (int(begin[b]), int(count[b]))
        if k[1]:
            out[b, :k[1]] = word_scores(x[b], pool[k[0]:k[0] + k[1]], blank, dtype)
    return out


def choose(scores, begin):
    """(best_index [B] pool indices or -1, logp [B], gap [B] = best minus second best, inf when there is no second) of scores [B, mc]."""
    B, mc = scores.shape
    best = torch.full((B,), -1, dtype=torch.int64)
    logp = torch.full((B,), float("-inf"), dtype=scores.dtype)
    gap = torch.full((B,), float("inf"), dtype=scores.dtype)
    for b in range(B):
        if mc == 0:
            continue
        v, j = scores[b].max(0)                                             # (the first maximum)
        if v > float("-inf"):
            best[b], logp[b] = int(begin[b]) + int(j), v
            rest = torch.cat([scores[b, :j], scores[b, j + 1:]])
            if rest.numel() and rest.max() > float("-inf"):
                gap[b] = v - rest.max()
    return best, logp, gap


def rows(best, pool, T, eos, padding):
    """(ids int64 [B, T + 1], n int64 [B]) of the chosen words: labels, EOS, PADDING; the empty row for -1."""
    B = best.shape[0]
    ids = torch.full((B, T + 1), padding, dtype=torch.int64)
    n = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        w = pool[int(best[b])] if int(best[b]) >= 0 else []
        ids[b, :len(w)] = torch.tensor(w, dtype=torch.int64)
        ids[b, len(w)] = eos
        n[b] = len(w)
    return ids, n
