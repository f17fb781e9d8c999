"""The cross-attention forms of the recognition decoder (`enc_attn` of a TransformerDecoderLayer, models/transformer_layer.py): which one a
model runs is decided once, by `choose`, from three shape facts; everything else the package knows about a form is on its class --

  * `extra_shapes` / `views`: the parameters it adds behind `enc_attn.fc.weight` and its entries of the layer's view dict (RecModel);
  * training (`finetune._DecoderStep`, passed in as `step`): `prepare`, the work that depends on the encoder memory alone -- the step issues it
    for all layers on the second stream before the layer loop, one event per layer, and `step.prepared(p)` waits for layer p's; `forward`
    (norm2's output, the layer's dropout spec) -> (attention output, saved state); `backward` (the gradient behind enc_attn.fc's proj_drop,
    that state) -> the gradient w.r.t. norm2's output, weight gradients through `step.side`, the memory gradient through `step.add_dmem`;
  * evaluation (`RecModel._decode_state / _decode_step`): `decode_state`, `decode_step` (writes st.a) and `attn_map`, the last layer's
    head-mean attention weights.

A form object holds shapes only -- no weights, no step -- so one is built per model and shared by its copies (ModelEma).  `p` is a layer's
name prefix ("decoder.layer_stack.3."), `pv` its view dict (`RecModel._w[p]`)."""
import ctypes

import torch

from . import _lib as L
from . import encoder_blocks as EB
from . import ops

BF16, F32 = torch.bfloat16, torch.float32
cf = ctypes.c_float


def choose(text_cond_vis, n_mem, d_model, n_head, d_k):
    form = TextConditional if text_cond_vis else MfmaFewQuery if n_mem == 256 and d_k == 64 else SequenceKernel
    return form(d_model, n_head, d_k, n_mem)


class _Form:
    prepares_memory = True

    def __init__(self, d_model, n_head, d_k, n_mem):
        self.d, self.nh, self.dk, self.hk, self.n_mem, self.scale = d_model, n_head, d_k, n_head * d_k, n_mem, d_k ** -0.5

    def extra_shapes(self, a):
        """((name, shape), ...) behind `a`fc.weight (a: "decoder.layer_stack.i.enc_attn.")."""
        return ()

    def views(self, a, p, s):
        """The form's own entries of the layer's view dict (p / s: name -> view of the fp32 arena / of the bf16 shadow)."""
        return {}


class _ProjectedKV(_Form):
    """linear_k | linear_v of the memory as ONE GEMM (the two weights are adjacent in the arena: pv["kv2"]), then dot-product attention of the
    T queries over it.  The two forms differ in their attention launches (`attend` / `attend_backward`) and in where the K|V GEMM runs."""

    def forward(self, step, p, h2, drop):
        q2 = ops.linear_fwd(h2, step.m._w[p]["q2"])
        a2, kv, kept = self.attend(step, p, q2, drop)
        return a2, (h2, q2, kv, kept, drop)

    def backward(self, step, p, dz, saved):
        h2, q2, kv, kept, drop = saved
        pv, side, mem, hk, rows = step.m._w[p], step.side, step.mem, self.hk, step.B * self.n_mem
        da2 = ops.linear_dgrad(dz, pv["fc2"])
        dq2, dkv = self.attend_backward(step, q2, kv, kept, da2, drop)
        side(lambda: ops.linear_wgrad(dq2, h2, step.g(p + "enc_attn.linear_q.weight")), dq2, h2)
        dh2 = ops.linear_dgrad(dq2, pv["q2"])
        side(lambda: ops.wgrad(dkv, mem, step.g_of(pv["kv2"]), 2 * hk, hk, rows), dkv, mem)
        # the gradient w.r.t. the encoder memory is needed only after the decoder loop: its GEMM runs on the second stream too
        side(lambda: step.add_dmem(ops.gemm(dkv, pv["kv2"], rows, hk, 2 * hk, tb=True)), dkv)
        return dh2

    def decode_state(self, st, mem, layers):
        st.kv_mem = [ops.linear_fwd(mem, pv["kv2"]) for pv in layers]                                   # [B*n_mem, 2hk]
        st.wts = torch.empty((st.S, self.nh, st.n_mem), device=mem.device, dtype=F32)

    def decode_step(self, st, i, pv, h, last):
        q2 = ops.linear_fwd(h, pv["q2"])
        L.call("dig_decode_cross_attn", L.ptr(q2), L.ptr(st.kv_mem[i]), L.ptr(st.a), L.ptr(st.wts) if last else None, st.S, st.n_mem, self.nh,
               self.dk, cf(self.scale), st.spm, L.stream())

    def attn_map(self, st):
        return st.wts.mean(1)


class MfmaFewQuery(_ProjectedKV):
    """256 keys, head dim 64: the MFMA attention kernel of the encoder.  The T queries of a sample sit in rows [0, T) of a fused q|k|v buffer
    of 256 rows per sample, and the kernels are told to compute the first ceil(T / 32) query blocks only (rows T..31 are zero queries with a
    zero output gradient: no contribution).  The K|V GEMM into that buffer depends on no decoder state: `prepare`, overlapping the (small,
    latency-bound) self-attention kernels of the decoder chain."""

    def prepare(self, mem, pv):
        fused = torch.empty((mem.shape[0], 3 * self.hk), device=mem.device, dtype=BF16)
        ops.gemm(mem, pv["kv2"], mem.shape[0], 2 * self.hk, self.d, out=fused[:, self.hk:], ldc=3 * self.hk)
        return (fused,)

    def attend(self, step, p, q2, drop):
        fused, = step.prepared(p)
        a2, ctx2, lse2 = EB.cross_attn_fwd(fused, q2, step.B, step.m.max_len, self.nh, self.hk, self.scale, drop=drop)
        return a2, fused, (ctx2, lse2)

    def attend_backward(self, step, q2, fused, kept, da2, drop):
        ctx2, lse2 = kept
        return EB.cross_attn_bwd(fused, ctx2, lse2, da2, step.B, step.m.max_len, self.nh, self.hk, self.scale, drop=drop)


class SequenceKernel(_ProjectedKV):
    """Head dim 24 / 48 (the `corres_*` decoders), --use_1d_attdec (32 keys): the sequence kernels over all keys.  Nothing is prepared: the K|V
    GEMM stays inside the layer loop on the main stream."""
    prepares_memory = False

    def attend(self, step, p, q2, drop):
        kv = ops.linear_fwd(step.mem, step.m._w[p]["kv2"])
        a2, lse2 = ops.seq_attn_fwd(q2, kv, kv[:, self.hk:], step.B, self.nh, step.m.max_len, self.n_mem, self.dk, self.scale, drop=drop)
        return a2, kv, lse2

    def attend_backward(self, step, q2, kv, lse2, da2, drop):
        dq2, dkv = torch.empty_like(q2), torch.empty_like(kv)
        ops.seq_attn_bwd(q2, kv, kv[:, self.hk:], da2, lse2, dq2, dkv, dkv[:, self.hk:], step.B, self.nh, step.m.max_len, self.n_mem, self.dk, self.scale,
                         drop=drop)
        return dq2, dkv


class TextConditional(_Form):
    """--text_cond_vis (TextConditionalMultiHeadAttention, models/transformer_layer.py:284-383), folded (csrc/text_cond_attn.hip): every query
    modulates the memory before linear_k / linear_v; neither has a bias, so both fold across the attention -- film = gamma_decode(h2); the
    scaled queries through Wk head by head (u); the attention over cond, which only exists row by row inside the kernel; its result through Wv
    head by head.  What depends on the memory alone is vk = LN_vis(vis_proj(memory)): `prepare`."""

    def __init__(self, d_model, n_head, d_k, n_mem):
        if d_k != 64 or n_head * d_k != d_model or d_model not in (128, 384, 512):
            raise NotImplementedError(f"text-conditional attention is built for d_model = 64 * n_head in {{128, 384, 512}} (the fold kernels are 64-wide "
                                      f"per head), not for head dimension {d_k} with d_model {d_model}")
        super().__init__(d_model, n_head, d_k, n_mem)

    def extra_shapes(self, a):                  # TextConditionalMultiHeadAttention.__init__ (transformer_layer.py:320-323), in its order
        hk = self.hk
        return ((a + "gamma_decode.weight", (2 * hk, hk)), (a + "gamma_decode.bias", (2 * hk,)), (a + "vis_proj.weight", (hk, hk)),
                (a + "vis_proj.bias", (hk,)), (a + "vis_norm.weight", (hk,)), (a + "vis_norm.bias", (hk,)),
                (a + "vis_cond_norm.weight", (hk,)), (a + "vis_cond_norm.bias", (hk,)))

    def views(self, a, p, s):
        return dict(k2=s(a + "linear_k.weight"), v2=s(a + "linear_v.weight"), gd=s(a + "gamma_decode.weight"), gdb=p(a + "gamma_decode.bias"),
                    vp=s(a + "vis_proj.weight"), vpb=p(a + "vis_proj.bias"), vnw=p(a + "vis_norm.weight"), vnb=p(a + "vis_norm.bias"),
                    cnw=p(a + "vis_cond_norm.weight"), cnb=p(a + "vis_cond_norm.bias"))

    def prepare(self, mem, pv):
        """(vk = LN_vis(vis_proj(mem)), then what the backward reads: the Linear's output, mean, rstd)."""
        h = ops.linear_fwd(mem, pv["vp"], bias=pv["vpb"])
        vk, mu, rs = ops.layernorm_fwd(h, pv["vnw"], pv["vnb"], 1e-5)
        return vk, h, mu, rs

    def fold_queries(self, q2s, wk):
        """u[r, h, :] = Wk_h^T q2s[r, h] per head ([rows, 64] x [64, d] on strided views; q2s carries the scale): bf16 [rows, heads * d].
        (The backward sends the attention output's gradient through Wv the same way.)"""
        rows, d, dk = q2s.shape[0], self.d, self.dk
        u = torch.empty((rows, self.nh * d), device=q2s.device, dtype=BF16)
        for h in range(self.nh):
            ops.gemm(q2s[:, h * dk:(h + 1) * dk], wk[h * dk:(h + 1) * dk], rows, d, dk, tb=True, out=u[:, h * d:(h + 1) * d])
        return u

    def fold_values(self, c, wv, out=None, **scale):
        """a[r, h] = Wv_h c[r, h] per head ([rows, d] x [64, d]^T): bf16 [rows, heads * 64].  (The backward sends du through Wk the same way,
        with the GEMM's alpha / alpha_cols as **scale.)"""
        rows, d, dk = c.shape[0], self.d, self.dk
        a = torch.empty((rows, self.nh * dk), device=c.device, dtype=BF16) if out is None else out
        for h in range(self.nh):
            ops.gemm(c[:, h * d:(h + 1) * d], wv[h * dk:(h + 1) * dk], rows, dk, d, out=a[:, h * dk:(h + 1) * dk], **scale)
        return a

    def forward(self, step, p, h2, drop):
        pv = step.m._w[p]
        film = ops.linear_fwd(h2, pv["gd"], bias=pv["gdb"])
        q2 = step.padded_rows(h2.shape[0], self.hk, h2.device)                  # (a weight-gradient operand read in 128-column tiles)
        ops.linear_fwd(h2, pv["q2"], alpha=self.scale, alpha_cols=self.hk, out=q2)
        u2 = self.fold_queries(q2, pv["k2"])
        vk, *vsaved = step.prepared(p)
        c2, lse2 = ops.tcv_attn_fwd(film, u2, vk, step.mem, pv["cnw"], pv["cnb"], step.B, step.m.max_len, self.n_mem, self.nh, 1, drop)
        return self.fold_values(c2, pv["v2"]), (h2, q2, film, u2, vk, vsaved, c2, lse2, drop)

    def backward(self, step, p, dz, saved):
        """The Wv fold gives dc and linear_v's gradient, dig_tcv_attn_bwd gives du / dfilm / dvk / the residual term of dmem and vis_cond_norm's
        gradients, the Wk fold gives the query gradient and linear_k's; gamma_decode, vis_proj and vis_norm are a Linear and a LayerNorm."""
        h2, q2, film, u2, vk, (hv, vmu, vrs), c2, lse2, drop = saved
        side, g, mem = step.side, step.g, step.mem
        d, nh, dk, hk, rows = self.d, self.nh, self.dk, self.hk, dz.shape[0]
        pv, a = step.m._w[p], p + "enc_attn."
        head = lambda t_, h, w_: t_[:, h * w_:(h + 1) * w_]
        da2 = step.padded_rows(rows, hk, dz.device)
        ops.linear_dgrad(dz, pv["fc2"], out=da2)
        dc = self.fold_queries(da2, pv["v2"])
        gv, gk = g(a + "linear_v.weight"), g(a + "linear_k.weight")
        side(lambda: [ops.wgrad(head(da2, h, dk), head(c2, h, d), gv[h * dk:(h + 1) * dk], dk, d, rows) for h in range(nh)], da2, c2)
        du, dfilm, dvk, dmem = ops.tcv_attn_bwd(film, u2, vk, mem, pv["cnw"], pv["cnb"], c2, lse2, dc, g(a + "vis_cond_norm.weight"),
                                                g(a + "vis_cond_norm.bias"), step.B, step.m.max_len, self.n_mem, nh, drop)
        dq2 = self.fold_values(du, pv["k2"], alpha=self.scale, alpha_cols=dk)         # q2 carries the scale: so does its gradient
        side(lambda: [ops.wgrad(head(q2, h, dk), head(du, h, d), gk[h * dk:(h + 1) * dk], dk, d, rows) for h in range(nh)], q2, du)
        side(lambda: ops.linear_wgrad(dq2, h2, g(a + "linear_q.weight")), dq2, h2)
        side(lambda: ops.linear_wgrad(dfilm, h2, g(a + "gamma_decode.weight")), dfilm, h2)
        side(lambda: ops.colsum(dfilm, g(a + "gamma_decode.bias")), dfilm)
        dh2 = ops.linear_dgrad(dq2, pv["q2"])
        dh2b = ops.linear_dgrad(dfilm, pv["gd"])
        ops.add_bf16(dh2, dh2b, dh2)

        def vis_path():
            dhv = ops.layernorm_bwd(dvk, hv, pv["vnw"], pv["vnb"], vmu, vrs, None, g(a + "vis_norm.weight"), g(a + "vis_norm.bias"))
            ops.linear_wgrad(dhv, mem, g(a + "vis_proj.weight"))
            ops.colsum(dhv, g(a + "vis_proj.bias"))
            dm = ops.linear_dgrad(dhv, pv["vp"])
            ops.add_bf16(dm, dmem, dm)
            step.add_dmem(dm)
        side(vis_path, dvk, dmem, hv, vmu, vrs, mem)
        return dh2

    def decode_state(self, st, mem, layers):
        st.mem = mem
        st.vk = [self.prepare(mem, pv)[0] for pv in layers]                                             # [B*n_mem, d]
        st.maps = torch.empty((st.S, st.n_mem), device=mem.device, dtype=F32)

    def decode_step(self, st, i, pv, h, last):
        film = ops.linear_fwd(h, pv["gd"], bias=pv["gdb"])
        u2 = self.fold_queries(ops.linear_fwd(h, pv["q2"], alpha=self.scale, alpha_cols=self.hk), pv["k2"])
        c2, _ = ops.tcv_attn_fwd(film, u2, st.vk[i], st.mem, pv["cnw"], pv["cnb"], st.S, 1, st.n_mem, self.nh, st.spm, None, st.maps if last else None)
        self.fold_values(c2, pv["v2"], out=st.a)

    def attn_map(self, st):
        return st.maps
