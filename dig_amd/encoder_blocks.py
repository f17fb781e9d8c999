"""The per-entry-point walk over the ViT encoder blocks -- norm1 -> qkv -> attention -> proj -> norm2 -> fc1 / GELU / fc2 and its explicit
reverse -- for every caller: the pre-training step (engine_core._Step), the fine-tune step (finetune._EncoderStep) and the recognition forward
(recognizer.RecModel).  One launch sequence, written once; what differs between the callers comes in as arguments:

  blocks   one dict per block under _EncWeights' key names ("norm1.weight", ..., "attn.qkv.weight", ..., "qkv_bias"; "g": the same names in the
           gradient arena), built once per arena binding by the caller
  plan     a Plan: which fused launches and which backward schedule, resolved by the caller once per call from its own switches
  drops    per block (attention, proj-branch, MLP-branch) dropout.DropSpec, any of them None; None = no block drops anything
  on_side / block_done / grad_ready / mark   the caller's second-stream hand-over, keep-list release, bucket callback and phase marks

The block-call path (one FFI crossing per block, the pre-training step's default) is block_calls.forward / backward; its saved activations
are read here as tensors.  The two helpers at the end run a few-query cross-attention on the encoder's MFMA attention kernels (PatchNet,
the recognition decoder)."""
from typing import NamedTuple

import torch

from . import ops

BF16 = torch.bfloat16
_NO_DROP = (None, None, None)


class Plan(NamedTuple):
    """The decisions of one walk.  Everything defaults to the plain form (the recognition forward runs Plan())."""
    # forward
    chain: bool = False             # fc1 -> GELU -> fc2 + residual in one launch (blocks whose MLP branch is not dropped)
    chain_ln: bool = False          # ... with norm2 in front and the LayerNorm behind the block in the same launch
    attn_block: bool = False        # qkv -> attention -> proj + residual in one launch (blocks without attention / proj dropout)
    # backward
    chain_bwd: bool = False         # both data gradients of the MLP in one launch, in the blocks (chain_every, chain_phase) select
    chain_every: int = 1
    chain_phase: int = 0
    chain_lnb: bool = False         # norm2's backward inside that launch
    chain_proj: bool = False        # ... and the projection's data gradient behind it
    attn_proj: bool = False         # the projection's data gradient inside the attention backward launch
    direct: bool = False            # data gradients as direct-form GEMMs on the transposed weight copies (wT[i][1:4]) where that form exists
    fused_qv: bool = False          # q / v bias gradients from the attention backward's per-image partial sums
    grouping: str = "off"           # the block's weight gradients on the grouped kernel: "block" (one launch), "pair" (MLP | attention), "off"
    inline: bool = False            # the grouped launch in the data-gradient chain (else on the second stream)
    side_each: bool = False         # every reduction handed to the second stream as it becomes ready (else: one hand-over per block)
    batch_reduce: bool = False      # a block's reductions as two launches (ops.GradReduceBatch)
    red_defer: bool = False         # grouped only: all blocks' bias / LayerNorm column sums in one launch behind the walk


def _tensors(s):
    """A block's saved activations: the tuple forward() made, or the views of a block-call forward's buffers (block_calls._BlockSaved)."""
    return s if isinstance(s, tuple) else s.tensors()


def _no_mark(name, dev):
    pass


def forward(plan, blocks, x, n_img, heads, eps, save, drops=None, tail=(None, None), frozen=0):
    """x: bf16 [n_img * 256, D] rows behind the patch embedding.  Returns (x behind the last block, saved, nxt).
    saved: [] unless `save`; then per block (x, ln1, mu1, rs1, qkv, ctx, lse, x_mid, ln2, mu2, rs2, pre, act) -- what backward() reads -- or
    None for the blocks below `frozen` (no gradient flows into them: nothing is kept, and no LayerNorm rides behind them).
    tail: (weight, bias) of the LayerNorm behind the last block; nxt = its (rows, mean, rstd) where the last chain launch made it, else None."""
    R, D = x.shape
    scale = (D // heads) ** -0.5
    saved, nxt, last = [], None, len(blocks) - 1
    for i, blk in enumerate(blocks):
        keep = save and i >= frozen
        ln1, mu1, rs1 = nxt if nxt is not None else ops.layernorm_fwd(x, blk["norm1.weight"], blk["norm1.bias"], eps)
        nxt = None
        # x + drop_path(dropout(branch)): per-sample keep / scale in the producing epilogue
        da, dp, dm = (drops[i] or _NO_DROP) if drops is not None else _NO_DROP
        if plan.attn_block and da is None and dp is None:
            # qkv Linear -> attention -> proj Linear + residual in one launch (csrc/attn_block.hip); qkv / lse exist only where kept
            x_mid, ctx, qkv, lse = ops.attn_block_fwd(ln1, x, blk["attn.qkv.weight"], blk["qkv_bias"], blk["attn.proj.weight"],
                                                      blk["attn.proj.bias"], n_img, heads, D, scale, save=keep)
        else:
            qkv = ops.linear_fwd(ln1, blk["attn.qkv.weight"], bias=blk["qkv_bias"], alpha=scale, alpha_cols=D)
            ctx, lse = ops.attn_fwd(qkv, n_img, heads, D, drop=da)
            x_mid = ops.linear_fwd(ctx, blk["attn.proj.weight"], bias=blk["attn.proj.bias"], resid=x, drop=dp)
        if plan.chain_ln:
            # norm2 -> fc1 -> GELU -> fc2 (+ residual) -> the LayerNorm behind the block (the next block's norm1, or `tail`) in one launch:
            # between two blocks the residual stream is written once and no LayerNorm launch remains; norm2 is taken on the way in
            ng, nb = (blocks[i + 1]["norm1.weight"], blocks[i + 1]["norm1.bias"]) if i < last else tail
            if i < frozen:
                ng = nb = None
            r = ops.mlp_chain_fwd_ln(x_mid, blk["norm2.weight"], blk["norm2.bias"], eps, blk["mlp.fc1.weight"], blk["mlp.fc1.bias"],
                                     blk["mlp.fc2.weight"], blk["mlp.fc2.bias"], ng, nb, save=keep, drop=dm)
            x_out, ln2, mu2, rs2, pre, act = r["out"], r["ln"], r["ln_mean"], r["ln_rstd"], r["pre"], r["act"]
            if ng is not None:
                nxt = (r["nln"], r["nln_mean"], r["nln_rstd"])
        else:
            ln2, mu2, rs2 = ops.layernorm_fwd(x_mid, blk["norm2.weight"], blk["norm2.bias"], eps)
            if plan.chain and dm is None:
                # fc1 -> GELU -> fc2 (+ residual) in one launch: the [R, F] hidden tensor is never a GEMM operand in HBM; a kept block
                # still writes the pre-activation and the GELU output (the backward's inputs)
                r = ops.mlp_chain_fwd(ln2, blk["mlp.fc1.weight"], blk["mlp.fc1.bias"], blk["mlp.fc2.weight"], blk["mlp.fc2.bias"], x_mid, save=keep)
                x_out, pre, act = r if keep else (r, None, None)
            else:
                pre = torch.empty((R, blk["mlp.fc1.weight"].shape[0]), device=x.device, dtype=BF16) if keep else None
                act = ops.linear_fwd(ln2, blk["mlp.fc1.weight"], bias=blk["mlp.fc1.bias"], act=1, pre=pre)
                x_out = ops.linear_fwd(act, blk["mlp.fc2.weight"], bias=blk["mlp.fc2.bias"], resid=x_mid, drop=dm)
        if save:
            saved.append((x, ln1, mu1, rs1, qkv, ctx, lse, x_mid, ln2, mu2, rs2, pre, act) if keep else None)
        x = x_out
    return x, saved, nxt


def backward(plan, blocks, saved, dx, wT, n_img, heads, on_side, first=0, drops=None, rows=None, block_done=None, grad_ready=None,
             mark=_no_mark):
    """The reverse of forward() over blocks [first, len(blocks)), last block first.  dx: bf16 gradient w.r.t. the last block's output rows
    (consumed); returns the gradient w.r.t. block `first`'s input rows.  Parameter gradients are accumulated into blk["g"].
    The data-gradient chain (dgrad GEMMs, attention backward, LayerNorm backward) runs on the caller's stream; what only consumes (dy, saved
    activation) pairs -- weight-gradient GEMMs, bias column sums -- goes through on_side(fn, *tensors the second stream will read).
    wT: per block (fc2.weight^T, fc1.weight^T[, proj.weight^T, qkv.weight^T]) where the plan reads them, or None.
    rows: only the first `rows` saved rows (the first n_img images) carry a gradient.
    block_done(): behind every block.  grad_ready(key): bucket "encoder.blocks.<i>" is final once both streams pass this point."""
    D = dx.shape[1]
    scale = (D // heads) ** -0.5
    dev = dx.device
    # The weight gradients of a block as ONE grouped launch (csrc/wgrad.hip), issued as soon as the block's last operand (dqkv) exists; its
    # slabs are folded into the gradient arena by the next block's launch (or the flush behind the walk), so block i's bucket is final one
    # launch later
    grp = ops.WgradGroup(dev) if plan.grouping != "off" else None
    # With the grouped launch, everything a block hands to the second stream -- the bias / LayerNorm-parameter column sums: five small launches
    # that only consume what the chain has produced -- goes over in ONE hand-over at the end of the block (one wait + one stream switch on the
    # host instead of five; the kernels are off the critical path either way), unless the plan asks for each on its own
    batch_side = grp is not None and not plan.side_each
    vred = ops.GradReduceBatch() if (plan.red_defer and grp) else None
    prev_block = None

    def launch_group(*tensors):
        if plan.inline:
            grp.launch()                                                 # in the data-gradient chain itself
        else:
            on_side(grp.launch, *tensors)

    for i in reversed(range(first, len(blocks))):
        blk, g = blocks[i], blocks[i]["g"]
        x, ln1, mu1, rs1, qkv, ctx, lse, x_mid, ln2, mu2, rs2, pre, act = _tensors(saved[i])
        saved[i] = None
        chain = plan.chain_bwd and (i % plan.chain_every == plan.chain_phase % plan.chain_every)
        if rows is not None:
            x, ln1, mu1, rs1, qkv, ctx, x_mid, ln2, mu2, rs2, pre, act = (t[:rows] for t in (x, ln1, mu1, rs1, qkv, ctx, x_mid, ln2, mu2, rs2, pre, act))
            lse = lse[:n_img * heads]
        # x_out = x_mid + fc2(gelu(fc1(ln2)))
        # batch_reduce: the reductions this block leaves behind (four split-R slab sums, five bias / LayerNorm-parameter column sums) are
        # collected in `red` and issued as two launches after the block's last weight-gradient GEMM
        red = ops.GradReduceBatch() if plan.batch_reduce else None
        wg = red.wgrad if red else ops.linear_wgrad
        csum = red.colsum_partials if red else ops.colsum_partials
        held = []                                                        # operands of the grouped launch (alive until the streams join)
        late, late_t = [], []

        def side_later(fn, *tensors):
            if batch_side:
                late.append(fn)
                late_t.extend(tensors)
            else:
                on_side(fn, *tensors)
        if grp:
            def wg(dy_, x_, dw_):
                if not grp.add(dy_, x_, dw_):                        # (never inside an assert: python -O would drop the weight gradient)
                    raise RuntimeError("grouped weight gradient: a problem of this block does not fit the group's plan")
                held.extend((dy_, x_))
        # a dropped branch (dropout and / or drop-path) back-propagates the residual gradient under the same mask; its bias gradient is the
        # column sum of the MASKED gradient, so the LayerNorm kernel's fused residual column sum is switched off for it
        da, dp, dm = (drops[i] or _NO_DROP) if drops is not None else _NO_DROP
        dz = ops.dropout_apply(dx, dm)
        if dm is not None:
            on_side(lambda dz=dz: ops.colsum(dz, g["mlp.fc2.bias"]), dz)
        if grp:
            wg(dz, act, g["mlp.fc2.weight"])
        else:
            on_side(lambda dz=dz: wg(dz, act, g["mlp.fc2.weight"]), dz, act)
        dctx = lnp = None
        if chain:
            # data gradient through fc2, GELU' and fc1 in one launch (d(pre-activation) leaves it as a side output for the fc1 weight
            # gradient, with its column sums = the fc1 bias gradient)
            w2t, w1t = wT[i][0], wT[i][1]
            if dm is not None or red is not None or not plan.chain_lnb:
                dln2, dact, bparts = ops.mlp_chain_bwd(dz, w2t, pre, w1t)
            elif plan.chain_proj:
                dx_mid, dact, bparts, lnp, dctx = ops.mlp_chain_bwd_ln(dx, w2t, pre, w1t, x_mid, blk["norm2.weight"], mu2, rs2, projt=wT[i][2])
                dln2 = dx_mid
            else:
                # ... with norm2's backward in the same launch: dx_mid = dx + LN2'(d ln2) leaves it, the three parameter-gradient sums
                # of norm2 / fc2's bias as partial rows
                dx_mid, dact, bparts, lnp = ops.mlp_chain_bwd_ln(dx, w2t, pre, w1t, x_mid, blk["norm2.weight"], mu2, rs2)
                dln2 = dx_mid
            mark("blk: fused MLP backward", dev)
        else:
            dact, bparts = ops.linear_dgrad(dz, blk["mlp.fc2.weight"], gelu_pre=pre, colsum=True)    # d(pre-activation): GELU' and
            dln2 = None                                                                               # the fc1 bias sums fused
        if grp:
            wg(dact, ln2, g["mlp.fc1.weight"])
            if vred:
                vred.colsum_partials(bparts, g["mlp.fc1.bias"])
            else:
                side_later(lambda: csum(bparts, g["mlp.fc1.bias"]), bparts)
            if plan.grouping == "pair":
                launch_group(*held)
        elif plan.side_each:
            on_side(lambda: csum(bparts, g["mlp.fc1.bias"]), bparts)
            on_side(lambda: wg(dact, ln2, g["mlp.fc1.weight"]), dact, ln2)
        else:
            on_side(lambda: (wg(dact, ln2, g["mlp.fc1.weight"]), csum(bparts, g["mlp.fc1.bias"])), dact, ln2, bparts)   # (0.3 ms/step vs a 201 MB pass)
        if dln2 is None:
            dln2 = ops.dgrad_direct(dact, wT[i][1]) if plan.direct else None
            if dln2 is None:
                dln2 = ops.linear_dgrad(dact, blk["mlp.fc1.weight"])
        if lnp is not None and vred:
            vred.layernorm_finalize_parts(lnp, g["norm2.weight"], g["norm2.bias"], g["mlp.fc2.bias"])
        elif lnp is not None:
            side_later(lambda lnp=lnp, g=g: ops.layernorm_finalize_parts(lnp, g["norm2.weight"], g["norm2.bias"], g["mlp.fc2.bias"]), lnp)
        else:
            fc2_b = g["mlp.fc2.bias"] if dm is None else None
            dx_mid, fin2, ws2 = ops.layernorm_bwd(dln2, x_mid, blk["norm2.weight"], blk["norm2.bias"], mu2, rs2, dx, g["norm2.weight"],
                                                  g["norm2.bias"], out=dln2, dres_colsum=fc2_b, defer=True)
            if red or vred:                                              # norm2 grads + colsum(dx) = fc2 bias grad: off the chain
                (red or vred).layernorm_finalize(ws2, x_mid.shape[0], D, g["norm2.weight"], g["norm2.bias"], fc2_b)
            else:
                side_later(fin2, ws2)
        # x_mid = x + proj(attn(ln1))
        dzp = ops.dropout_apply(dx_mid, dp)
        if dp is not None:
            on_side(lambda dzp=dzp: ops.colsum(dzp, g["attn.proj.bias"]), dzp)
        if grp:
            wg(dzp, ctx, g["attn.proj.weight"])
        else:
            on_side(lambda dzp=dzp: wg(dzp, ctx, g["attn.proj.weight"]), dzp, ctx)
        mark("blk: LayerNorm backward (norm2)", dev)
        # (the projection's data gradient inside the attention backward launch where that form exists: no GEMM, no d(ctx) rows)
        proj_attn = dctx is None and plan.attn_proj and plan.fused_qv and dp is None and da is None
        if dctx is None and not proj_attn:
            # (direct form on proj.weight^T where it pays: both operands K-contiguous, bit-identical to the transpose-read form)
            dctx = ops.dgrad_direct(dzp, wT[i][2]) if plan.direct else None
            if dctx is None:
                dctx = ops.linear_dgrad(dzp, blk["attn.proj.weight"])
        mark("blk: proj data gradient", dev)
        gb = g["qkv_bias"]
        if plan.fused_qv:
            # q_bias / v_bias gradients: per-image column sums of dQ (already carrying the q scale) and dV leave the attention kernel as
            # [n_img, D] fp32 partials (DPP row reductions of the accumulators, no extra pass over the 150 MB dqkv); K has no bias
            if proj_attn:
                dqkv, qs, vs = ops.attn_bwd_proj(qkv, ctx, dzp, wT[i][2], lse, n_img, heads, D, scale, bias_sums=True)
                dctx = None                                              # (no d(ctx) rows: the qkv data gradient below gets a buffer of its own)
            else:
                dqkv, qs, vs = ops.attn_bwd(qkv, ctx, dctx, lse, n_img, heads, D, scale, bias_sums=True, drop=da)
            mark("blk: attention backward", dev)
            if grp:
                wg(dqkv, ln1, g["attn.qkv.weight"])
                launch_group(*held)
                mark("blk: grouped weight gradients", dev)
                if vred:
                    vred.colsum_partials(qs, gb[:D]); vred.colsum_partials(vs, gb[2 * D:])
                else:
                    side_later(lambda: (csum(qs, gb[:D]), csum(vs, gb[2 * D:])), qs, vs)
            else:
                on_side(lambda: (wg(dqkv, ln1, g["attn.qkv.weight"]), csum(qs, gb[:D]), csum(vs, gb[2 * D:])), dqkv, ln1, qs, vs)
        else:
            dqkv = ops.attn_bwd(qkv, ctx, dctx, lse, n_img, heads, D, scale, drop=da)
            if grp:
                wg(dqkv, ln1, g["attn.qkv.weight"])
                launch_group(*held)
                side_later(lambda: (ops.colsum(dqkv, gb[:D], cols=D), ops.colsum(dqkv[:, 2 * D:], gb[2 * D:], cols=D)), dqkv)
            else:
                on_side(lambda: (wg(dqkv, ln1, g["attn.qkv.weight"]),
                                 ops.colsum(dqkv, gb[:D], cols=D), ops.colsum(dqkv[:, 2 * D:], gb[2 * D:], cols=D)), dqkv, ln1)
        dln1 = ops.dgrad_direct(dqkv, wT[i][3], out=dctx) if plan.direct else None
        if dln1 is None:
            dln1 = ops.linear_dgrad(dqkv, blk["attn.qkv.weight"], out=dctx)
        mark("blk: qkv data gradient", dev)
        proj_b = g["attn.proj.bias"] if dp is None else None
        dx, fin1, ws1 = ops.layernorm_bwd(dln1, x, blk["norm1.weight"], blk["norm1.bias"], mu1, rs1, dx_mid, g["norm1.weight"],
                                          g["norm1.bias"], out=dln1, dres_colsum=proj_b, defer=True)
        mark("blk: LayerNorm backward (norm1)", dev)
        if vred:
            vred.layernorm_finalize(ws1, x.shape[0], D, g["norm1.weight"], g["norm1.bias"], proj_b)
        elif red:                                                        # norm1 grads + colsum(dx_mid) = proj bias grad
            red.layernorm_finalize(ws1, x.shape[0], D, g["norm1.weight"], g["norm1.bias"], proj_b)
            side_later(red.flush, *red.tensors())
        else:
            side_later(fin1, ws1)
        if late:
            on_side(lambda: [f() for f in late], *late_t)
        del dact, pre, act, dln2, dqkv, dctx, held, late, late_t, dz, dzp
        if block_done is not None:
            block_done()
        # this block's gradients are final once BOTH streams pass this point.  (Grouped weight gradients: block i's slabs are folded by the
        # NEXT launch, so the bucket that is final here is block i + 1's.)
        done = i
        if grp:
            done, prev_block = prev_block, i
        if grad_ready is not None and done is not None:
            grad_ready(f"encoder.blocks.{done}")
    if vred:
        vred.flush()                                                     # (vectors only: one launch per 112 segments, on this stream)
    if grp:
        if plan.inline:
            grp.flush()
        else:
            on_side(grp.flush)
        if grad_ready is not None and prev_block is not None:
            grad_ready(f"encoder.blocks.{prev_block}")
    return dx


# ---- a few queries per image against its 256 keys on the encoder's MFMA attention kernels (head dim 64): the n queries of an image sit in rows
# [0, n) of a fused q | k | v buffer of 256 rows per image whose k | v columns [D, 3 D) the caller's projection GEMM has written; rows n .. (the
# end of the last 32-query block) are zero queries with a zero output gradient: no contribution

def cross_attn_fwd(fused, q, n_img, n, heads, D, scale, drop=None):
    """q: bf16 [n_img * n, D] unscaled queries (scale = 2^-3: exact in bf16).  Returns (attention output [n_img * n, D], ctx, lse): ctx / lse
    are the kernel's full-size outputs, which cross_attn_bwd reads."""
    fq = fused.view(n_img, 256, 3 * D)[:, :, :D]
    fq[:, n:(n + 31) // 32 * 32].zero_()
    fq[:, :n] = (q * scale).view(n_img, n, D)
    ctx, lse = ops.attn_fwd(fused, n_img, heads, D, drop=drop, q_rows=n)      # query blocks past n are not computed
    return ctx.view(n_img, 256, D)[:, :n].reshape(n_img * n, D), ctx, lse


def cross_attn_bwd(fused, ctx, lse, da, n_img, n, heads, D, scale, drop=None):
    """da: bf16 [n_img * n, D] gradient w.r.t. cross_attn_fwd's output.  Returns (dq [n_img * n, D], dkv: the [n_img * 256, 2 D] k | v columns
    of the fused gradient, row stride 3 D).  (Padded rows: finite outputs, zero dO -> delta = 0.)"""
    dctx = torch.empty((n_img * 256, D), device=da.device, dtype=BF16)
    dv = dctx.view(n_img, 256, D)
    dv[:, n:(n + 31) // 32 * 32].zero_()
    dv[:, :n] = da.view(n_img, n, D)
    dfused = ops.attn_bwd(fused, ctx, dctx, lse, n_img, heads, D, scale, drop=drop, q_rows=n)
    return dfused.view(n_img, 256, 3 * D)[:, :n, :D].reshape(n_img * n, D), dfused[:, D:]
