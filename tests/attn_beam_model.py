"""Specification (test infrastructure only) of the beam search of the GRU attention head: `AttentionRecognitionHead.beam_search`
(models/attn_decoder.py:84-200) restated statement by statement on `attn_decoder_oracle.decoder_step`, in float64 unless the caller asks
otherwise.  Its only departure from the reference: `predecessors` is an integer division (:127 divides to a float, which no current torch
accepts as an index).  The reference never reaches the method (`AttnRecModel.forward` calls `sample`), so there is no fixture written from
it; what pins this restatement is tests/test_attn_beam.py: width 1 against the greedy `head_sample` of the fixture model, and the final
back-tracking (:140-200, restated here in torch) against `dig_amd.recognizer.beam_backtrack` on decisions whose hypotheses end at different
steps.

`beam_search` keeps what a comparison needs from every step: the scores of all K*C candidates of a sample, the chosen candidates, and the
three stored lists of the reference (scores before the EOS mask, predecessors, emitted symbols).  It can follow given decisions
(`force_decisions`, candidate indices k*C + c in place of the top-K) and rank given classifier outputs (`force_logits`)."""
import types

import torch
import torch.nn.functional as F

import attn_decoder_oracle as AD

NEG_INF = float("-inf")


def cast_state(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def backtrack(stored_scores, stored_preds, stored_syms, B, K, eos):
    """attn_decoder.py:140-200 on the stored lists ([T] of [B*K] tensors): ids [B, T] of the best hypothesis per sample, and the lengths."""
    T = len(stored_syms)
    pos = (torch.arange(B) * K).view(-1, 1)
    lens = [[T] * K for _ in range(B)]
    sorted_score, sorted_idx = stored_scores[-1].view(B, K).topk(K)        # the last step's beams are not sorted
    s = sorted_score.clone()
    found = [0] * B                                                          # EOS found per sample in the backward walk
    t_pred = (sorted_idx + pos).view(B * K)
    steps = []
    for t in range(T - 1, -1, -1):
        cur = stored_syms[t].index_select(0, t_pred)
        t_pred = stored_preds[t].index_select(0, t_pred)
        ended = stored_syms[t].eq(eos).nonzero()
        for i in range(ended.size(0) - 1, -1, -1):
            idx = int(ended[i, 0])
            b = idx // K
            k = K - (found[b] % K) - 1                                       # an ended hypothesis replaces the worst slot first
            found[b] += 1
            r = b * K + k
            t_pred[r] = stored_preds[t][idx]
            cur[r] = stored_syms[t][idx]
            s[b, k] = stored_scores[t][idx]
            lens[b][k] = t + 1
        steps.append(cur)
    s, order = s.topk(K)
    lens = [[lens[b][int(k)] for k in order[b]] for b in range(B)]
    order = (order + pos).view(B * K)
    seqs = torch.cat([st.index_select(0, order).view(B, K, 1) for st in reversed(steps)], -1)
    return seqs[:, 0, :], [l[0] for l in lens]


def beam_search(P, c, x, beam_width, eos, force_logits=None, force_decisions=None, dtype=torch.float64):
    """x: encoder tokens [B, N, in_planes].  force_logits [T, B*K, C]; force_decisions [T, B, K] int64.  Returns a namespace:
    cand_scores [T, B, K*C] (running score + log-probability of every candidate), candidates [T, B, K], scores / preds / syms [T, B*K]
    (the stored lists), logits [T, B*K, C] (the decoder's own outputs), masked (slots set to -inf, [T, B*K] bool), ids [B, T], lens [B]."""
    P = cast_state(P, dtype)
    K, C, T = int(beam_width), c.num_classes, c.max_len
    B, N, D = x.shape
    xin = x.to(dtype).unsqueeze(1).repeat(1, K, 1, 1).view(B * K, N, D)      # sample b -> rows b*K .. b*K + K - 1
    xproj = xin @ P[AD.PRE + "attention_unit.xEmbed.weight"].t() + P[AD.PRE + "attention_unit.xEmbed.bias"]
    state = torch.zeros(B * K, c.sDim, dtype=dtype)
    pos = (torch.arange(B) * K).view(-1, 1)
    seq = torch.full((B * K, 1), NEG_INF, dtype=torch.float64)
    seq[::K] = 0.0
    y_prev = torch.full((B * K,), C, dtype=torch.long)
    st_scores, st_preds, st_syms, all_cand, all_choice, all_logits, all_masked = [], [], [], [], [], [], []
    for i in range(T):
        out, state, _ = AD.decoder_step(P, c, xin, xproj, state, y_prev)
        all_logits.append(out.detach().double())
        if force_logits is not None:
            out = force_logits[i].to(out.dtype)
        logp = F.log_softmax(out.double(), dim=1)
        cand_scores = (seq.repeat(1, C) + logp).view(B, K * C)
        if force_decisions is None:
            scores, cands = cand_scores.topk(K, dim=1)
        else:
            cands = force_decisions[i].long().view(B, K)
            scores = cand_scores.gather(1, cands)
        y_prev = (cands % C).view(B * K)
        seq = scores.reshape(B * K, 1)
        preds = (cands // C + pos).view(B * K)                               # (the one departure: an integer division)
        state = state.index_select(0, preds)
        st_scores.append(seq.view(-1).clone())
        ended = y_prev.view(-1, 1).eq(eos)
        seq = seq.masked_fill(ended, NEG_INF)
        st_preds.append(preds)
        st_syms.append(y_prev)
        all_cand.append(cand_scores); all_choice.append(cands); all_masked.append(ended.view(-1))
    ids, lens = backtrack(st_scores, st_preds, st_syms, B, K, eos)
    return types.SimpleNamespace(cand_scores=torch.stack(all_cand), candidates=torch.stack(all_choice), scores=torch.stack(st_scores),
                                 preds=torch.stack(st_preds), syms=torch.stack(st_syms), logits=torch.stack(all_logits),
                                 masked=torch.stack(all_masked), ids=ids, lens=lens)
