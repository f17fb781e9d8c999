"""The block-call path over the ViT encoder blocks: ONE FFI crossing per block (dig_encoder_block_fwd / dig_encoder_block_bwd,
include/dig_block_types.h) and two allocations per block (a bf16 buffer, an fp32 one) instead of a crossing per kernel and an allocation per
tensor.  Same kernels, same arguments, same order as encoder_blocks.forward / backward: bit-identical to the per-entry-point walk.
What differs between calls comes in as arguments, as in encoder_blocks: `blocks` (one dict per block under _EncWeights' key names; the call
structs are cached on them), the decisions the caller resolved from its own switches (forward: `fuse_attn`; backward: a Plan), the second
stream's handle and the caller's keep-list / bucket callbacks."""
import ctypes
import math
from typing import NamedTuple

import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32
_F32_PIECES = ("lse", "mu2", "rs2", "nmu", "nrs")


class Plan(NamedTuple):
    """The decisions of one block-call backward."""
    defer: bool                     # the grouped weight-gradient launches behind the LAST data gradient (else inside each block's call)
    red_defer: bool                 # deferred only: all blocks' bias / LayerNorm column sums in one launch behind the last data gradient
    tile_direct: int                # tile code of the direct-form data gradients on the transposed weight copies (0: the transpose-read form)
    attn_proj: bool                 # the projection's data gradient inside the attention backward launch
    fuse_ln2: bool                  # norm2's backward inside the fused MLP backward launch
    chain_proj: bool                # ... and the projection's data gradient behind it


class _BlockSaved:
    """What dig_encoder_block_fwd(save = 1) left for the backward of one block: two buffers (bf16 tensors, fp32 statistics) and the block's
    input rows x / ln1 / mean / rstd, which live in the PREVIOUS block's buffers (or, for block 0, in tensors of their own).  The block-call
    backward reads addresses (`ptr`); the per-entry-point backward asks for tensors()."""
    __slots__ = ("b16", "b32", "off", "rows", "D", "F", "n_img", "heads", "inp", "inp_ptr")

    def __init__(self, b16, b32, off, rows, D, F, n_img, heads, inp, inp_ptr):
        self.b16, self.b32, self.off, self.rows, self.D, self.F, self.n_img, self.heads = b16, b32, off, rows, D, F, n_img, heads
        self.inp = inp                   # keeps x, ln1, mu1, rs1 alive: 4 tensors (block 0) or the previous block's (b16, b32)
        self.inp_ptr = inp_ptr           # their addresses: (x, ln1, mu1, rs1)

    def ptr(self, name):
        return (self.b32 if name in _F32_PIECES else self.b16).data_ptr() + self.off[name]

    def view(self, name):
        R, D, F = self.rows, self.D, self.F
        if name == "lse":
            a = self.off["lse"] // 4
            return self.b32[a:a + self.n_img * self.heads * 256].view(self.n_img * self.heads, 256)
        if name in _F32_PIECES:
            a = self.off[name] // 4
            return self.b32[a:a + R]
        cols = {"qkv": 3 * D, "pre": F, "act": F}.get(name, D)
        a = self.off[name] // 2
        return self.b16[a:a + R * cols].view(R, cols)

    def tensors(self):
        """(x, ln1, mu1, rs1, qkv, ctx, lse, x_mid, ln2, mu2, rs2, pre, act) as tensors (views)."""
        if len(self.inp) == 4:
            x, ln1, mu1, rs1 = self.inp
        else:
            p = self.inp[2]
            x, ln1, mu1, rs1 = p.view("out"), p.view("nln"), p.view("nmu"), p.view("nrs")
        return (x, ln1, mu1, rs1) + tuple(self.view(k) for k in ("qkv", "ctx", "lse", "x_mid", "ln2", "mu2", "rs2", "pre", "act"))


def forward(blocks, x, n_img, heads, Fh, eps, save, fuse_attn):
    """x: bf16 [n_img * 256, D] rows behind the patch embedding.  Each call runs qkv GEMM -> attention -> proj GEMM + residual -> norm2 + MLP +
    residual + the next block's norm1.  Returns (x behind the last block, [a _BlockSaved per block] if `save` else [])."""
    R, D = x.shape
    dev = x.device
    off, n16, n32 = ops.block_fwd_layout(R, D, Fh, n_img, heads, save)
    ln1, mu1, rs1 = ops.layernorm_fwd(x, blocks[0]["norm1.weight"], blocks[0]["norm1.bias"], eps)
    inp, inp_ptr = (x, ln1, mu1, rs1), (x.data_ptr(), ln1.data_ptr(), mu1.data_ptr(), rs1.data_ptr())
    stream, key, fuse_attn = ops.L.stream(), ("fwd_call", bool(save), R, n_img), int(fuse_attn)
    saved, prev = [], None
    for i, blk in enumerate(blocks):
        st = blk.get(key)
        if st is None:
            nb = blocks[i + 1] if i + 1 < len(blocks) else None
            st = blk[key] = ops.BlockFwd(
                n_img=n_img, heads=heads, D=D, F=Fh, rows=R, save=int(bool(save)),
                tile_qkv=ops.fwd_tile_code(R, 3 * D, D) or ops.GEMM_BK_FWD, tile_proj=ops.fwd_tile_code(R, D, D, has_resid=True) or ops.GEMM_BK_FWD,
                fuse_attn=fuse_attn, eps=eps, scale=(D // heads) ** -0.5,
                qkv_w=blk["attn.qkv.weight"].data_ptr(), qkv_b=blk["qkv_bias"].data_ptr(), proj_w=blk["attn.proj.weight"].data_ptr(),
                proj_b=blk["attn.proj.bias"].data_ptr(), n2_g=blk["norm2.weight"].data_ptr(), n2_b=blk["norm2.bias"].data_ptr(),
                fc1_w=blk["mlp.fc1.weight"].data_ptr(), fc1_b=blk["mlp.fc1.bias"].data_ptr(), fc2_w=blk["mlp.fc2.weight"].data_ptr(),
                fc2_b=blk["mlp.fc2.bias"].data_ptr(), next_n1_g=nb["norm1.weight"].data_ptr() if nb else None,
                next_n1_b=nb["norm1.bias"].data_ptr() if nb else None)
        b16 = torch.empty(n16 // 2, device=dev, dtype=BF16)
        b32 = torch.empty(n32 // 4, device=dev, dtype=F32)
        p16, p32 = b16.data_ptr(), b32.data_ptr()
        st.fuse_attn = fuse_attn                                      # (a switch, like fuse_ln2 / wg_defer of the backward: set on every call)
        st.x, st.ln1 = inp_ptr[0], inp_ptr[1]
        for k in off:
            setattr(st, k, (p32 if k in _F32_PIECES else p16) + off[k])
        ops.L.call("dig_encoder_block_fwd", ctypes.byref(st), stream)
        cur = _BlockSaved(b16, b32, off, R, D, Fh, n_img, heads, inp, inp_ptr)
        if save:
            saved.append(cur)
            inp, inp_ptr = (b16, b32, cur), (p16 + off["out"], p16 + off["nln"], p32 + off["nmu"], p32 + off["nrs"])
        else:
            inp, inp_ptr = (b16, b32), (p16 + off["out"], p16 + off["nln"], 0, 0)     # (no chain of blocks: the previous buffers go back to the pool)
        prev = cur
    return prev.view("out"), saved


def _bwd_struct(blk, wplan, n_img, heads, D, Fh, R):
    """The fields of a block's dig_encoder_block_bwd call that hold from step to step: shapes, tile codes, weight and gradient addresses."""
    g, gb = blk["g"], blk["g"]["qkv_bias"]
    assert all(g[k].is_contiguous() for k in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"))
    return ops.BlockBwd(
        n_img=n_img, heads=heads, D=D, F=Fh, rows=R, tile_dgrad=ops.dgrad_tile_code(R, D) or ops.GEMM_BK_BWD, scale=(D // heads) ** -0.5,
        qkv_w=blk["attn.qkv.weight"].data_ptr(), proj_w=blk["attn.proj.weight"].data_ptr(),
        n1_g=blk["norm1.weight"].data_ptr(), n1_b=blk["norm1.bias"].data_ptr(), n2_g=blk["norm2.weight"].data_ptr(),
        n2_b=blk["norm2.bias"].data_ptr(),
        g_n1_g=g["norm1.weight"].data_ptr(), g_n1_b=g["norm1.bias"].data_ptr(), g_qkv_w=g["attn.qkv.weight"].data_ptr(),
        g_q_b=gb.data_ptr(), g_v_b=gb[2 * D:].data_ptr(), g_proj_w=g["attn.proj.weight"].data_ptr(),
        g_proj_b=g["attn.proj.bias"].data_ptr(), g_n2_g=g["norm2.weight"].data_ptr(), g_n2_b=g["norm2.bias"].data_ptr(),
        g_fc1_w=g["mlp.fc1.weight"].data_ptr(), g_fc1_b=g["mlp.fc1.bias"].data_ptr(), g_fc2_w=g["mlp.fc2.weight"].data_ptr(),
        g_fc2_b=g["mlp.fc2.bias"].data_ptr(),
        wg_fn=wplan.fn, wg_wa=wplan.wa, wg_splits=wplan.splits, wg_n_wg=wplan.n_wg, wg_fold_splits=wplan.splits,
        wg_trans=(ctypes.c_int * 4)(*wplan.trans))


def _hold_back(red, g, t32, off, R, n_img, D, Fh, n_b, n_l2):
    """What dig_encoder_block_bwd(defer_red = 1) did not launch on the second stream (csrc/encoder_block.inc), as nine segments of red's one
    launch: the fp32 partial rows in the block's buffer t32 -> the block's bias / LayerNorm gradients."""
    def piece(name, *shape):
        a = off[name] // 4
        return t32[a:a + math.prod(shape)].view(shape)
    gb = g["qkv_bias"]
    red.colsum_partials(piece("bparts", n_b, Fh), g["mlp.fc1.bias"])
    red.layernorm_finalize_parts(piece("ws2", n_l2, 3, D), g["norm2.weight"], g["norm2.bias"], g["mlp.fc2.bias"])
    red.colsum_partials(piece("qs", n_img, D), gb[:D])
    red.colsum_partials(piece("vs", n_img, D), gb[2 * D:])
    red.layernorm_finalize(t32[off["ws1"] // 4:], R, D, g["norm1.weight"], g["norm1.bias"], g["attn.proj.bias"])


def backward(plan, blocks, saved, dx, wT, wplan, n_img, heads, Fh, side, keep, block_done, grad_ready):
    """The reverse of forward(), last block first.  dx: contiguous bf16 gradient w.r.t. the last block's output rows; returns the gradient
    w.r.t. the patch embedding's output rows.  Each call runs the block's data-gradient chain on the caller's stream and, unless the plan holds
    them back, the grouped weight gradients inside it and the five parameter-gradient reductions on the stream `side` behind one event.
    wT: per block (fc2.weight^T, fc1.weight^T, proj.weight^T, qkv.weight^T); wplan: ops.wgrad_block_plan of these shapes.
    keep(t): the second stream reads t (None: it is the caller's stream).  block_done(): behind every call.  grad_ready(key): bucket
    "encoder.blocks.<i>" is final once both streams pass this point (a block's slabs are folded by the NEXT launch)."""
    R, D = dx.shape
    dev = dx.device
    off, n16, n32 = ops.block_bwd_layout(R, D, Fh, n_img)
    grp = wplan.group
    stream, key = ops.L.stream(), ("bwd_call", R, n_img)
    n_b, n_l2 = ops.L.query("dig_mlp_chain_colsum_rows", R), ops.L.query("dig_mlp_chain_ln_parts", R)
    red = ops.GradReduceBatch() if plan.red_defer else None

    def block(i, dy_ptr, probs, fold=None):
        """Block i's call on the incoming gradient at dy_ptr.  probs: the table its four weight-gradient problems go to; fold: (table, slabs)
        of the launch this call folds.  Returns (the block's bf16 buffer -- d(input rows) at off["dctx"] --, its fp32 buffer, the slab set
        its launch fills)."""
        blk, sv = blocks[i], saved[i]
        saved[i] = None
        st = blk.get(key)
        if st is None:
            st = blk[key] = _bwd_struct(blk, wplan, n_img, heads, D, Fh, R)
        # the switches, set on every call
        w2t, w1t, projt, qkvt = wT[i]
        st.w2t, st.w1t = w2t.data_ptr(), w1t.data_ptr()
        st.projt = projt.data_ptr() if plan.chain_proj else None
        st.tile_direct, st.attn_proj = plan.tile_direct, int(plan.attn_proj)
        st.proj_wt = projt.data_ptr() if (plan.tile_direct or plan.attn_proj) else None
        st.qkv_wt = qkvt.data_ptr() if plan.tile_direct else None
        st.wg_defer, st.fuse_ln2, st.defer_red = int(plan.defer), int(plan.fuse_ln2), int(plan.red_defer)
        # this call's addresses
        st.x, st.ln1, st.mu1, st.rs1 = sv.inp_ptr
        for k in ("qkv", "ctx", "lse", "x_mid", "ln2", "mu2", "rs2", "pre", "act"):
            setattr(st, k, sv.ptr(k))
        t16 = torch.empty(n16 // 2, device=dev, dtype=BF16)
        t32 = torch.empty(n32 // 4, device=dev, dtype=F32)
        p16, p32 = t16.data_ptr(), t32.data_ptr()
        st.dy = dy_ptr
        for k in off:
            setattr(st, k, (p16 if k in ("dln2", "dpre", "dctx", "dqkv") else p32) + off[k])
        slabs = grp.next_slabs(wplan.slab_bytes)
        st.wg_map, st.wg_slabs, st.wg_probs = wplan.wmap.data_ptr(), slabs.data_ptr(), ctypes.addressof(probs)
        st.wg_fold_n, st.wg_fold_probs, st.wg_fold_slabs = (4, ctypes.addressof(fold[0]), fold[1].data_ptr()) if fold else (0, None, None)
        st.side = side
        if red:
            _hold_back(red, blk["g"], t32, off, R, n_img, D, Fh, n_b, n_l2)
        ops.L.call("dig_encoder_block_bwd", ctypes.byref(st), stream)
        if keep is not None and not red:
            keep(t32)                                                    # the second stream's reductions read it
        block_done()
        return t16, t32, slabs

    def ready(i):
        if i is not None:
            grad_ready(f"encoder.blocks.{i}")

    def inline():
        """The grouped launch inside each block's call, folding its predecessor's slabs: two tables in turn, buckets one block behind."""
        tables = ((ops._WgProb * 4)(), (ops._WgProb * 4)())
        t16, t32, last, dy_ptr = dx, None, None, dx.data_ptr()
        for n, i in enumerate(reversed(range(len(blocks)))):
            t16, t32, slabs = block(i, dy_ptr, tables[n & 1], last and (last[1], last[2]))
            dy_ptr = t16.data_ptr() + off["dctx"]                        # the next block's incoming gradient lives in this block's buffer
            ready(last and last[0])
            last = (i, tables[n & 1], slabs)
        return t16, last

    def deferred():
        """Every block's call first -- one table each, operands kept alive --, the held-back reductions in one launch behind them (nothing runs
        beside it), then the grouped launches in block order, each folding its predecessor's slabs, every bucket behind its fold."""
        t16, t32, held, dy_ptr = dx, None, [], dx.data_ptr()
        for i in reversed(range(len(blocks))):
            own, sv = (ops._WgProb * 4)(), saved[i]
            t16, t32, _ = block(i, dy_ptr, own)
            held.append((i, own, t16, sv))
            dy_ptr = t16.data_ptr() + off["dctx"]
        if red:
            red.flush()
        last = None
        for i, own, _, _ in held:
            slabs = grp.next_slabs(wplan.slab_bytes)
            grp.call(ctypes.addressof(own), 4, ctypes.addressof(last[1]) if last else None, 4 if last else 0, wplan.splits, wplan.wmap, wplan.n_wg,
                     slabs, last and last[2], wplan.splits)
            ready(last and last[0])
            last = (i, own, slabs)
        return t16, last

    t16, (i, table, slabs) = (deferred if plan.defer else inline)()
    grp.fold(ctypes.addressof(table), 4, slabs, wplan.splits)            # the last launch's slabs, then the last bucket
    ready(i)
    a = off["dctx"] // 2
    return t16[a:a + R * D].view(R, D)


def defer_fits(cache, dev, extra_bytes):
    """The deferred weight-gradient plan keeps `extra_bytes` of gradient temporaries (and every block's saved activations) alive until
    the end of the backward: taken only while that leaves three quarters of what the device (and torch's pool) has free.  The answer
    is cached per size (`cache`: the model's dict): one hipMemGetInfo per new shape, not per step."""
    key = (dev.index, extra_bytes)
    if key not in cache:
        free, _ = torch.cuda.mem_get_info(dev)
        pooled = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        cache[key] = extra_bytes <= (free + pooled) // 4
    return cache[key]
