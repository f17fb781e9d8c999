"""Test-only fp32 torch specification of the text-conditional decoder cross-attention (`--text_cond_vis`), written from its formulas:

    (gamma | beta)[t] = gamma_decode(q_in[t])                      q_in = the decoder layer's norm2 output
    vk[k]             = LN_vis(vis_proj(mem[k]))
    cond[t, k]        = mem[k] + LN_cond(tanh(gamma[t]) * vk[k] + tanh(beta[t]))
    literal : K = linear_k(cond), V = linear_v(cond)  ([B, Lq, Lk, d] through both projections), softmax over k of scale * q_h[t] . K_h[t, k]
    folded  : u[t, h] = scale * Wk_h^T q_h[t],  logit[t, h, k] = u[t, h] . cond[t, k],  c[t, h] = sum_k w[t, h, k] cond[t, k],  out_h[t] = Wv_h c[t, h]
    maps    = the head mean of the weights BEFORE dropout; dropout acts on the normalised weights; then fc and proj_drop as in the plain layer.

`core` is the part the device runs in one launch (dig_tcv_attn_fwd; autograd supplies what dig_tcv_attn_bwd returns); the decoder layer, the
teacher-forced step and greedy / beam decoding are the plain oracle's (oracle/decode_oracle.py, oracle/finetune_oracle.py) with this cross-attention
in place of MultiHeadAttention.  `rnd` rounds at the tensor boundaries of the device path (film, vk, u, c and every GEMM output): with
`bf16_round` the same functions are the bf16 yardstick.  tests/golden/text_cond_tiny.npz (tools/gen_text_cond_golden.py) pins all of it against the
unmodified reference modules."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as TF

import decode_oracle as D
import dig_oracle as O
import finetune_oracle as FO

NEW_TENSORS = ("gamma_decode.weight", "gamma_decode.bias", "vis_proj.weight", "vis_proj.bias", "vis_norm.weight", "vis_norm.bias",
               "vis_cond_norm.weight", "vis_cond_norm.bias")


def ident(x):
    return x


class _Bf16Round(torch.autograd.Function):
    """Value and gradient both rounded to bf16: what a bf16 tensor boundary does to the forward and to the backward."""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


def bf16_round(x):
    return _Bf16Round.apply(x)


def text_cond_shapes(c):
    """The eight tensors a decoder layer gains, in the reference's registration order (behind enc_attn.fc.weight)."""
    hk = c.n_head * c.d_k
    o = OrderedDict()
    for i in range(c.n_layers):
        p = f"decoder.layer_stack.{i}.enc_attn."
        o[p + "gamma_decode.weight"] = (2 * hk, hk); o[p + "gamma_decode.bias"] = (2 * hk,)
        o[p + "vis_proj.weight"] = (hk, hk); o[p + "vis_proj.bias"] = (hk,)
        o[p + "vis_norm.weight"] = (hk,); o[p + "vis_norm.bias"] = (hk,)
        o[p + "vis_cond_norm.weight"] = (hk,); o[p + "vis_cond_norm.bias"] = (hk,)
    return o


def param_shapes(c):
    """decode_oracle.decoder_param_shapes with the new tensors behind each layer's enc_attn.fc.weight."""
    new, o = text_cond_shapes(c), OrderedDict()
    for k, s in D.decoder_param_shapes(c).items():
        o[k] = s
        if k.endswith("enc_attn.fc.weight"):
            for n in NEW_TENSORS:
                o[k[:-len("fc.weight")] + n] = new[k[:-len("fc.weight")] + n]
    return o


def det_text_cond_state(c, seed):
    """Deterministic values of the new tensors (norm weights near 1, biases small, matrices at 1 / sqrt(fan_in))."""
    P = OrderedDict()
    for n, s in text_cond_shapes(c).items():
        if n.endswith("norm.weight"):
            P[n] = O.det_tensor(n, s, seed, 0.1, 1.0)
        elif n.endswith(".bias"):
            P[n] = O.det_tensor(n, s, seed, 0.05)
        else:
            P[n] = O.det_tensor(n, s, seed, 1.0 / np.sqrt(s[-1]))
    return P


def keep_factor(k0, k1, thr, scale, S, H, Lq, N):
    """The weights' dropout factor [S, H, Lq, N] under a site key: keep rule of dig_seq_attn_fwd_dropout."""
    a = (np.arange(Lq, dtype=np.uint32)[:, None] << np.uint32(16)) | np.arange(N, dtype=np.uint32)[None, :]
    b = np.arange(S * H, dtype=np.uint32)[:, None, None]
    keep = FO.keep_mask(k0, k1, a[None], b, thr)
    return torch.from_numpy(keep).view(S, H, Lq, N).float() * scale


def cond_rows(film, vk, mem, lnc_g, lnc_b, eps=1e-5, spm=1):
    """film [S, Lq, 2d], vk / mem [M, N, d] -> cond [S, Lq, N, d] (sequence s reads memory s // spm)."""
    d = vk.shape[-1]
    g, b = torch.tanh(film[..., :d]), torch.tanh(film[..., d:])
    if spm > 1:
        vk, mem = vk.repeat_interleave(spm, 0), mem.repeat_interleave(spm, 0)
    z = g[:, :, None, :] * vk[:, None] + b[:, :, None, :]
    return mem[:, None] + TF.layer_norm(z, (d,), lnc_g, lnc_b, eps)


def core(film, u, vk, mem, lnc_g, lnc_b, eps=1e-5, spm=1, keep=None):
    """The folded attention between the two fold GEMMs.  u [S, Lq, H, d] (scale included); keep [S, H, Lq, N] or None.
    Returns c [S, Lq, H, d], lse [S, Lq, H], wmean [S, Lq, N]."""
    cond = cond_rows(film, vk, mem, lnc_g, lnc_b, eps, spm)
    logits = torch.einsum("sthd,stkd->sthk", u, cond)
    w = logits.softmax(-1)
    wd = w if keep is None else w * keep.permute(0, 2, 1, 3).to(w.dtype)
    return torch.einsum("sthk,stkd->sthd", wd, cond), torch.logsumexp(logits, -1), w.mean(2)


def attn_literal(P, pre, c, q_in, mem, keep=None):
    """The module as the reference states it: every query's memory goes through linear_k and linear_v.  Returns (fc output, maps)."""
    B, Lq, _ = q_in.shape
    N, hk = mem.shape[1], c.n_head * c.d_k
    film = q_in @ P[pre + "gamma_decode.weight"].t() + P[pre + "gamma_decode.bias"]
    vk = TF.layer_norm(mem @ P[pre + "vis_proj.weight"].t() + P[pre + "vis_proj.bias"], (hk,), P[pre + "vis_norm.weight"], P[pre + "vis_norm.bias"], 1e-5)
    cond = cond_rows(film, vk, mem, P[pre + "vis_cond_norm.weight"], P[pre + "vis_cond_norm.bias"])
    q = (q_in @ P[pre + "linear_q.weight"].t()).view(B, Lq, c.n_head, c.d_k)
    k = (cond @ P[pre + "linear_k.weight"].t()).view(B, Lq, N, c.n_head, c.d_k)
    v = (cond @ P[pre + "linear_v.weight"].t()).view(B, Lq, N, c.n_head, c.d_k)
    w = (torch.einsum("bthe,btkhe->bhtk", q, k) * c.d_k ** -0.5).softmax(-1)
    wd = w if keep is None else w * keep.to(w.dtype)
    out = torch.einsum("bhtk,btkhe->bthe", wd, v).reshape(B, Lq, hk)
    return out @ P[pre + "fc.weight"].t(), w.mean(1)


def attn_folded(P, pre, c, q_in, mem, keep=None, rnd=ident, vk=None, spm=1):
    """The same module folded, in the device path's steps; rnd rounds where that path stores a tensor.  vk: a cached LN_vis(vis_proj(mem))."""
    B, Lq, _ = q_in.shape
    H, dk, hk = c.n_head, c.d_k, c.n_head * c.d_k
    film = rnd(q_in @ P[pre + "gamma_decode.weight"].t() + P[pre + "gamma_decode.bias"])
    if vk is None:
        vk = fold_vk(P, pre, c, mem, rnd)
    q = rnd((q_in @ P[pre + "linear_q.weight"].t()) * dk ** -0.5).view(B, Lq, H, dk)
    u = rnd(torch.einsum("bthe,hed->bthd", q, P[pre + "linear_k.weight"].view(H, dk, hk)))
    cc, _, maps = core(film, u, vk, mem, P[pre + "vis_cond_norm.weight"], P[pre + "vis_cond_norm.bias"], 1e-5, spm, keep)
    a = rnd(torch.einsum("bthd,hed->bthe", rnd(cc), P[pre + "linear_v.weight"].view(H, dk, hk))).reshape(B, Lq, hk)
    return a @ P[pre + "fc.weight"].t(), maps


def fold_vk(P, pre, c, mem, rnd=ident):
    hk = c.n_head * c.d_k
    return rnd(TF.layer_norm(rnd(mem @ P[pre + "vis_proj.weight"].t() + P[pre + "vis_proj.bias"]), (hk,), P[pre + "vis_norm.weight"],
                             P[pre + "vis_norm.bias"], 1e-5))


# ---------------------------------------------------------------------------------------------- decoder
def decoder_attention(P, c, trg_seq, tgt_lens, memory, dr=None, attn=attn_folded):
    """TFDecoder._attention with the text-conditional cross-attention (train mode under the masks of `dr`, a finetune_oracle.DropOracle, or
    eval mode with dr = None); returns (output [B, L, d], the last layer's maps)."""
    B, L = trg_seq.shape
    pd = dr.decoder_dropout if dr is not None else 0.0
    elem = (lambda site, x: dr.elem(site, x, pd)) if dr is not None else (lambda site, x: x)
    x = elem(FO.DEC_TGT, P["decoder.trg_word_emb.weight"][trg_seq] + D.position_table(c.n_position, c.d_model)[None, :L])
    pad = torch.arange(L)[None, :] < tgt_lens[:, None]
    sub = (1 - torch.triu(torch.ones(L, L), diagonal=1)).bool()
    mask = pad.unsqueeze(-2) & sub.unsqueeze(0)
    maps = None
    for i in range(c.n_layers):
        p = f"decoder.layer_stack.{i}."
        h = TF.layer_norm(x, (c.d_model,), P[p + "norm1.weight"], P[p + "norm1.bias"], 1e-5)
        if dr is not None:
            x = x + FO._mha_train(P, p + "self_attn.", c, h, h, mask, dr, FO.dec_site(i, 0), FO.dec_site(i, 1))
        else:
            x = x + D._mha(P, p + "self_attn.", c, h, h, mask)[0]
        h = TF.layer_norm(x, (c.d_model,), P[p + "norm2.weight"], P[p + "norm2.bias"], 1e-5)
        keep = None
        if dr is not None and pd:
            k0, k1 = dr.key(FO.dec_site(i, 2))
            keep = keep_factor(k0, k1, dr.thr(pd), 1.0 / (1.0 - pd), B, c.n_head, L, memory.shape[1])
        a, maps = attn(P, p + "enc_attn.", c, h, memory, keep)
        x = x + elem(FO.dec_site(i, 3), a)
        h = TF.layer_norm(x, (c.d_model,), P[p + "norm3.weight"], P[p + "norm3.bias"], 1e-5)
        u = elem(FO.dec_site(i, 4), TF.gelu(h @ P[p + "mlp.w_1.weight"].t() + P[p + "mlp.w_1.bias"]))
        x = x + elem(FO.dec_site(i, 5), u @ P[p + "mlp.w_2.weight"].t() + P[p + "mlp.w_2.bias"])
    return TF.layer_norm(x, (c.d_model,), P["decoder.layer_norm.weight"], P["decoder.layer_norm.bias"], 1e-6), maps


def memory_of(P, ecfg, c, images, dr=None, use_1d_attdec=False):
    enc = D.encoder_features(P, ecfg, images) if dr is None else FO._encoder_train(P, ecfg, images, dr)
    if use_1d_attdec:
        enc = D.columns_1d(enc, ecfg)
    return TF.layer_norm(enc @ P["linear_norm.0.weight"].t() + P["linear_norm.0.bias"], (c.d_model,), P["linear_norm.1.weight"],
                         P["linear_norm.1.bias"], 1e-5)


def forward_train(P, ecfg, c, images, targets, lens, dr=None, use_1d_attdec=False, attn=attn_folded):
    """RecModel.forward in train mode with text_cond_vis: teacher-forced logits [B, T, C]."""
    mem = memory_of(P, ecfg, c, images, dr, use_1d_attdec)
    bos = torch.full((images.shape[0], 1), c.start_idx, dtype=targets.dtype)
    query = torch.cat([bos, targets], dim=-1)[:, :-1]
    out = decoder_attention(P, c, query, lens, mem, dr, attn)[0]
    return out @ P["decoder.classifier.weight"].t() + P["decoder.classifier.bias"]


def loss_and_grads(P, ecfg, c, images, targets, lens, dr=None, use_1d_attdec=False, attn=attn_folded):
    Q = OrderedDict((k, v.detach().clone().requires_grad_(k != "encoder.mask_token")) for k, v in P.items())
    logits = forward_train(Q, ecfg, c, images, targets, lens, dr, use_1d_attdec, attn)
    loss = D.seq_cross_entropy(logits, targets, lens)
    loss.backward()
    grads = OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v))) for k, v in Q.items())
    return loss.item(), grads, logits.detach()


def step_logits(P, c, seq, step, memory, attn=attn_folded):
    """Classifier logits of position `step` given the (BOS-prefixed) sequence so far: one step of forward_test / beam_search."""
    o, m = decoder_attention(P, c, seq, torch.full((seq.shape[0],), step + 1, dtype=torch.long), memory, None, attn)
    return o[:, step] @ P["decoder.classifier.weight"].t() + P["decoder.classifier.bias"], m[:, step]


def greedy_decode(P, c, memory, force_tokens=None, attn=attn_folded):
    """TFDecoder.forward_test: (probabilities [B, T, C], maps [B, T, N], tokens [B, T]); force_tokens feeds the given tokens instead of the arg-max."""
    B = memory.shape[0]
    seq = torch.zeros((B, c.max_seq_len + 1), dtype=torch.long)
    seq[:, 0] = c.start_idx
    outs, maps, toks = [], [], []
    for step in range(c.max_seq_len):
        lg, m = step_logits(P, c, seq, step, memory, attn)
        prob = lg.softmax(-1)
        outs.append(prob); maps.append(m); toks.append(prob.argmax(-1))
        seq[:, step + 1] = toks[-1] if force_tokens is None else force_tokens[:, step]
    return torch.stack(outs, 1), torch.stack(maps, 1), torch.stack(toks, 1)


def beam_search(P, c, memory, beam_width, eos=94, force_logits=None, force_syms=None, attn=attn_folded):
    """TFDecoder.beam_search (decode_oracle.beam_search's bookkeeping) on this decoder.  force_logits [T, B*bw, C]: rank these instead of the
    decoder's; force_syms [T, B*bw]: feed these symbols back whatever was ranked.  Returns (ids [B, T], step logits [T, B*bw, C], symbols [T, B*bw])."""
    B, N, C = memory.shape
    bw, T, nc = beam_width, c.max_seq_len, c.num_classes
    mem = memory.unsqueeze(1).repeat(1, bw, 1, 1).reshape(-1, N, C)
    seq = torch.zeros((B * bw, T + 1), dtype=torch.long)
    seq[:, 0] = c.start_idx
    pos_index = (torch.arange(B) * bw).view(-1, 1)
    seq_scores = torch.full((B * bw, 1), -float("inf"))
    seq_scores[torch.arange(B) * bw] = 0.0
    s_scores, s_pred, s_sym, kept = [], [], [], []
    for step in range(T):
        lg = step_logits(P, c, seq, step, mem, attn)[0]
        kept.append(lg)
        logp = TF.log_softmax(lg if force_logits is None else force_logits[step], dim=-1)
        scores, cand = (seq_scores.repeat(1, nc) + logp).view(B, -1).topk(bw, dim=1)
        sym = (cand % nc).view(B * bw)
        seq_scores = scores.view(B * bw, 1)
        s_scores.append(seq_scores.clone())
        seq_scores = seq_scores.masked_fill(sym.view(-1, 1).eq(eos), -float("inf"))
        s_pred.append((cand // nc + pos_index.expand_as(cand)).view(B * bw, 1))
        s_sym.append(sym)
        seq[:, step + 1] = sym if force_syms is None else force_syms[step]
    ids = D.backtrack(torch.stack(s_scores).squeeze(-1), torch.stack(s_pred).squeeze(-1), torch.stack(s_sym), B, bw, eos)
    return ids, torch.stack(kept), torch.stack(s_sym)
