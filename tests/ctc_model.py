"""The project's own specification of the CTC recognition head in plain torch (fp32 / fp64; test infrastructure, like
tests/textcond_model.py): what dig_amd/ctc_recognizer.py and csrc/ctc.hip are tested against, itself asserted equal to the reference's
`CTCRecModel` and `ctc_get_str_list` through tests/golden/ctc_tiny.npz (tools/gen_ctc_golden.py) on the CPU.

  * the head (models/model_builder.py:30-38) on oracle/finetune_oracle._encoder_train: column means of the token grid, Linear, LayerNorm(eps
    1e-6), GELU, Linear;
  * the criterion: `F.ctc_loss(..., reduction='none', zero_infinity=True)` per sample, summed and divided by B; the labels of a row are
    its first length - len_offset cells; a row holding a label outside [0, C) or equal to the blank counts as 0, like a row without an
    alignment;
  * the decode rule as a loop: per frame the first arg-max; a frame emits when it is not the blank, differs from the previous frame's
    arg-max and is not EOS; rows = emitted classes, EOS, PADDING; scores = the emitting frames' softmax probabilities, then 1."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as TF

import decode_oracle as D
import dig_oracle as O
import finetune_oracle as F

D_EMBEDDING = 512
PRE = "ctc_classifier."


def head_shapes(enc_dim, nb_classes):
    return OrderedDict([(PRE + "0.weight", (D_EMBEDDING, enc_dim)), (PRE + "0.bias", (D_EMBEDDING,)), (PRE + "1.weight", (D_EMBEDDING,)),
                        (PRE + "1.bias", (D_EMBEDDING,)), (PRE + "3.weight", (nb_classes + 1, D_EMBEDDING)), (PRE + "3.bias", (nb_classes + 1,))])


def det_head_state(enc_dim, nb_classes, seed):
    """Deterministic head values of the fixture (the scheme of decode_oracle.det_encoder_state)."""
    P = OrderedDict()
    for n, s in head_shapes(enc_dim, nb_classes).items():
        if n == PRE + "1.weight":
            P[n] = O.det_tensor(n, s, seed, 0.1, 1.0)
        elif n.endswith("bias"):
            P[n] = O.det_tensor(n, s, seed, 0.05)
        else:
            P[n] = O.det_tensor(n, s, seed, 1.0 / np.sqrt(float(s[1])))
    return P


def state(ecfg, nb_classes, seed_enc, seed_head):
    return OrderedDict(list(D.det_encoder_state(ecfg, seed_enc).items()) + list(det_head_state(ecfg.embed_dim, nb_classes, seed_head).items()))


def logits(P, ecfg, images, drop=None):
    """CTCRecModel.forward: [B, 32, nb_classes + 1]."""
    drop = F.DropOracle(0, 0, depth=ecfg.depth) if drop is None else drop
    cols = D.columns_1d(F._encoder_train(P, ecfg, images, drop), ecfg)
    h = TF.linear(cols, P[PRE + "0.weight"], P[PRE + "0.bias"])
    h = TF.gelu(TF.layer_norm(h, (D_EMBEDDING,), P[PRE + "1.weight"], P[PRE + "1.bias"], 1e-6))
    return TF.linear(h, P[PRE + "3.weight"], P[PRE + "3.bias"])


def ctc_nll(x, target, n, blank):
    """Per-sample -log p(labels | x): x [B, T, C], target [B, ldt], n [B] label counts.  Differentiable in x."""
    B, T, C = x.shape
    n = n.clamp(0, target.shape[1])
    live = torch.arange(target.shape[1])[None, :] < n[:, None]
    bad = (((target < 0) | (target >= C) | (target == blank)) & live).any(1)
    safe = torch.where(live & ~bad[:, None], target, torch.full_like(target, (blank + 1) % C))
    nll = TF.ctc_loss(TF.log_softmax(x.float() if x.dtype == torch.bfloat16 else x, -1).transpose(0, 1), safe, torch.full((B,), T, dtype=torch.int64),
                      torch.where(bad, torch.zeros_like(n), n), blank=blank, reduction="none", zero_infinity=True)
    return torch.where(bad, torch.zeros_like(nll), nll)


def ctc_nll_and_grad(x, target, n, blank):
    """(nll [B], d nll_b / d x [B, T, C]) in x's precision, as float64 / float32 tensors."""
    x = x.detach().clone().requires_grad_(True)
    nll = ctc_nll(x, target, n, blank)
    nll.sum().backward()
    return nll.detach(), x.grad.detach()


def loss(lg, target, length, blank, len_offset=1):
    """SeqCTCLoss: sum_b nll_b / B."""
    return ctc_nll(lg, target, length - len_offset, blank).sum() / lg.shape[0]


def loss_and_grads(P, ecfg, images, targets, lens, blank):
    Q = OrderedDict((k, v.detach().clone().requires_grad_(k != "encoder.mask_token")) for k, v in P.items())
    lg = logits(Q, ecfg, images)
    l = loss(lg, targets, lens, blank)
    l.backward()
    grads = OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v))) for k, v in Q.items())
    return l.item(), grads, lg.detach()


def greedy_decode(x, blank, eos, padding):
    """(ids int64 [B, T + 1], score fp32 [B, T + 1], n int64 [B]) of logits x [B, T, C]."""
    B, T, C = x.shape
    probs = torch.softmax(x.float(), -1)
    ids = torch.full((B, T + 1), padding, dtype=torch.int64)
    score = torch.ones((B, T + 1), dtype=torch.float32)
    n = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        prev, k = -1, 0
        for t in range(T):
            c = int(torch.argmax(x[b, t]))                                   # (the first maximum)
            if c != blank and not (t > 0 and c == prev) and c != eos:
                ids[b, k], score[b, k] = c, probs[b, t, c]
                k += 1
            prev = c
        ids[b, k] = eos
        n[b] = k
    return ids, score, n


def frames_to_strings(frames, voc, blank):
    """ctc_get_str_list's predictions (metrics.py:220-227,241) from per-frame classes [B, T]."""
    import string
    keep = string.digits + string.ascii_letters
    out = []
    for row in frames.tolist():
        chars = [voc[c] for j, c in enumerate(row) if c != blank and not (j > 0 and row[j - 1] == c) and voc[c] not in ("EOS", "UNKNOWN")]
        out.append("".join(ch for ch in chars if ch in keep).lower())
    return out
