"""The specification of the CTC forced alignment (dig_ctc_align, the rule in include/dig_hip.h) in numpy: test infrastructure, like
tests/ctc_beam_model.py.  `lp` is always a [T, C] table of frame log-probabilities -- `torch.log_softmax` of the logits in float64 or in
float32 -- and every function works in lp's precision, so the same code gives the float64 figures and their float32 twin.

States of n labels are s = 0..2n: an even state is the blank, state 2k + 1 is label k.  v[0][0] = lp[0][blank], v[0][1] = lp[0][l_0];
v[t][s] = lp[t][cls(s)] + max over stay (s), step (s - 1), skip (s - 2: odd s >= 3 with l_k != l_{k-1}) in that order, a later one
taken only when strictly larger; the path ends in state 2n unless v[T-1][2n-1] is strictly larger, and is read off the recorded choices."""
import numpy as np


def extended(labels, blank):
    """The class of every state: blank, l_0, blank, l_1, ..., blank."""
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(labels, dtype=np.int64)
    return ext


def feasible(labels, blank, T, C):
    labels = list(labels)
    if any(l < 0 or l >= C or l == blank for l in labels):
        return False
    return len(labels) + sum(labels[i] == labels[i - 1] for i in range(1, len(labels))) <= T


def _run(lp, labels, blank, forbidden):
    """K Viterbi runs at once, run k with the cell forbidden[k] = (t, s) struck out ((-1, 0): none): (score [K], states [K, T])."""
    lp = np.asarray(lp)
    T = lp.shape[0]
    ext = extended(labels, blank)
    S, n, K = len(ext), len(labels), len(forbidden)
    em = lp[:, ext]                                                         # [T, S]
    ninf = np.array(-np.inf, dtype=lp.dtype)
    skip_ok = np.zeros(S, dtype=bool)
    skip_ok[3::2] = ext[3::2] != ext[1:-2:2]
    ft, fs = np.array([f[0] for f in forbidden]), np.array([f[1] for f in forbidden])
    rows = np.arange(K)
    v = np.full((K, S), ninf, dtype=lp.dtype)
    v[:, 0] = em[0, 0]
    if n:
        v[:, 1] = em[0, 1]
    v[rows[ft == 0], fs[ft == 0]] = ninf
    choice = np.zeros((T, K, S), dtype=np.int8)
    for t in range(1, T):
        step = np.concatenate([np.full((K, 1), ninf), v[:, :-1]], axis=1)
        skip = np.concatenate([np.full((K, min(2, S)), ninf), v[:, :-2]], axis=1)[:, :S]
        skip = np.where(skip_ok[None, :], skip, ninf)
        m, c = v, np.zeros((K, S), dtype=np.int8)
        take = step > m
        m, c = np.where(take, step, m), np.where(take, 1, c)
        take = skip > m
        m, c = np.where(take, skip, m), np.where(take, 2, c)
        v = (m + em[t][None, :]).astype(lp.dtype)
        v[rows[ft == t], fs[ft == t]] = ninf
        choice[t] = c
    s = np.full(K, S - 1)
    if n:
        s = np.where(v[:, S - 2] > v[:, S - 1], S - 2, S - 1)
    score = v[rows, s]
    states = np.zeros((K, T), dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[:, t] = s
        if t:
            s = s - choice[t, rows, s]
    return score, states


def viterbi(lp, labels, blank):
    """(score, states [T]) of the best path; score -inf (states meaningless) when the labels have no path."""
    score, states = _run(lp, labels, blank, [(-1, 0)])
    return score[0], states[0]


def path_score(lp, labels, blank, states):
    """The sum of lp along a path, frame by frame in lp's precision."""
    lp = np.asarray(lp)
    ext = extended(labels, blank)
    total = lp.dtype.type(0)
    for t, s in enumerate(states):
        total = lp.dtype.type(total + lp[t, ext[int(s)]])
    return total


def validity(states, labels):
    """A path of the labels: starts in state 0 or 1, ends in 2n or 2n - 1, never moves down, moves up by at most one state, or by two
    from a label to the next label when the two differ."""
    n = len(labels)
    states = [int(s) for s in states]
    if not states or states[0] not in (0, 1) or states[-1] not in (2 * n, 2 * n - 1) or min(states) < 0:
        return False
    for a, b in zip(states, states[1:]):
        d = b - a
        if d < 0 or d > 2:
            return False
        if d == 2 and not (b & 1 and b >= 3 and labels[b >> 1] != labels[(b >> 1) - 1]):
            return False
    return True


def spans(lp, labels, blank, states):
    """(start [n], end [n], char_logp [n]) of a valid path: label k on the frames [start, end), the sum of its lp over them."""
    lp = np.asarray(lp)
    n = len(labels)
    start, end, logp = [-1] * n, [-1] * n, [lp.dtype.type(0)] * n
    for t, s in enumerate(states):
        s = int(s)
        if s & 1:
            k = s >> 1
            if start[k] < 0:
                start[k] = t
            end[k] = t + 1
            logp[k] = lp.dtype.type(logp[k] + lp[t, labels[k]])
    return start, end, logp


def states_of_frame_labels(frame_label):
    """The states of a frame_label row (k on a frame of label k, -1 on a blank frame): a blank frame sits behind the last label seen."""
    out, last = [], -1
    for k in frame_label:
        k = int(k)
        if k >= 0:
            last = k
            out.append(2 * k + 1)
        else:
            out.append(2 * (last + 1))
    return out


def second_best_gap(lp, labels, blank):
    """The best score minus the best score of any OTHER path: another path avoids at least one cell (t, s*_t) of the best path, so the
    largest score of the T runs with one of those cells struck out is the second-best score, exactly.  inf when there is one path only."""
    best, states = viterbi(lp, labels, blank)
    if not np.isfinite(best):
        return float("nan")
    other, _ = _run(lp, labels, blank, [(t, int(s)) for t, s in enumerate(states)])
    return float(best - other.max())
