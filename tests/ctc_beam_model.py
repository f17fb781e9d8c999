"""The project's own specification of the CTC prefix beam search (`--ctc_beam_width`, dig_ctc_beam_decode; test infrastructure, like
tests/ctc_model.py): the rule as a plain loop over a dict keyed by the prefix, in float64 or float32.  The reference has no CTC beam
search, so this file is the definition that csrc/ctc.hip and cpu_abi/dig_cpu_rec.cpp are tested against.

  * lp[t] = log_softmax of frame t over the C classes, taken in the working dtype;
  * a hypothesis is (prefix, lb, ln): the log-probability of the alignments of frames 0..t that collapse to the prefix and end in blank / in
    the prefix's last class; tot = logaddexp(lb, ln); start: ((), 0, -inf);
  * frame t visits the hypotheses best first; each adds (logaddexp) tot + lp[blank] to its own lb, ln + lp[last] to its own ln when it is not
    empty, and for every class c != blank in ascending order (lb if c repeats the last symbol else tot) + lp[c] to the ln of prefix + (c,),
    which may be a live prefix itself; `eos` is an ordinary class;
  * the W candidates of largest tot (all when fewer) survive, ties broken by the order in which the prefixes were first touched (a dict
    keeps it; the sort is stable);
  * the result is the best hypothesis after the last frame: logp = its tot, the row = its prefix without the symbols equal to `eos`.

Every arithmetic step goes through the working dtype (a Python float holds a float32 value exactly; sums and logaddexp are numpy's of that
dtype)."""
import numpy as np
import torch

NEG = float("-inf")


def beam_search_one(x, blank, W, dtype=np.float64):
    """x [T, C] logits of one sample -> (prefix tuple, logp float, kept = per frame the list of surviving prefixes, gap = the smallest tot
    difference between the last kept and the first dropped candidate of any frame or between the final two best; inf when there is none)."""
    dt = np.dtype(dtype).type
    tdt = torch.float64 if dt is np.float64 else torch.float32
    lp = torch.log_softmax(torch.as_tensor(x).to(tdt), -1).numpy()
    T, C = lp.shape

    def lae(a, b):
        return float(np.logaddexp(dt(a), dt(b)))

    def add(a, b):
        return float(dt(a) + dt(b))

    beam = [((), 0.0, NEG)]                                                # (prefix, lb, ln), best first
    kept, gap = [], float("inf")
    for t in range(T):
        row = lp[t]
        cand = {}                                                          # prefix -> [lb, ln], in creation order
        for p, lb, ln in beam:
            tot = lae(lb, ln)
            cell = cand.setdefault(p, [NEG, NEG])
            cell[0] = lae(cell[0], add(tot, row[blank]))
            if p:
                cell[1] = lae(cell[1], add(ln, row[p[-1]]))
            ext_tot = (dt(tot) + row).tolist()                             # tot + lp[c] for every c at once (the same dtype sums)
            for c in range(C):
                if c == blank:
                    continue
                v = add(lb, row[c]) if (p and c == p[-1]) else ext_tot[c]
                q = p + (c,)
                cell = cand.get(q)
                if cell is None:
                    cand[q] = [NEG, v]
                else:
                    cell[1] = lae(cell[1], v)
        scored = [(p, lb, ln, lae(lb, ln)) for p, (lb, ln) in cand.items()]
        scored.sort(key=lambda h: -h[3])                                   # stable: ties keep the creation order
        if len(scored) > W:
            gap = min(gap, scored[W - 1][3] - scored[W][3])
        beam = [(p, lb, ln) for p, lb, ln, _ in scored[:W]]
        kept.append([p for p, _, _ in beam])
        final = scored[:2]
    if len(final) > 1:
        gap = min(gap, final[0][3] - final[1][3])
    return beam[0][0], final[0][3], kept, gap


def beam_decode(x, blank, eos, padding, W, dtype=np.float64):
    """x [B, T, C] -> (ids int64 [B, T + 1] = prefix without EOS, EOS, PADDING; logp float64 [B]; n int64 [B]; kept: per sample, per frame the
    surviving prefixes; gap float64 [B])."""
    B, T, _ = x.shape
    ids = torch.full((B, T + 1), padding, dtype=torch.int64)
    logp, gap = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    n = torch.zeros(B, dtype=torch.int64)
    kept = []
    for b in range(B):
        p, lpb, k, g = beam_search_one(x[b], blank, W, dtype)
        row = [c for c in p if c != eos]
        ids[b, :len(row)] = torch.tensor(row, dtype=torch.int64)
        ids[b, len(row)] = eos
        n[b], logp[b], gap[b] = len(row), lpb, g
        kept.append(k)
    return ids, logp, n, kept, gap
