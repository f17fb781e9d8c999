"""Forward and hand-written backward of MoCo_ViT as a sequence of HIP kernel launches.

The math follows the reference step by step (citations: modeling_pretrain_moco_mim_ori.py:488-577 MoCo_ViT.forward,
modeling_pretrain_vit.py:89-106 encoder, modeling_finetune.py:87-158 attention/block/MLP, :444-461 InfoNCE); what is
new is the execution model: no autograd graph over ops, one custom autograd node for the whole model whose
backward is the explicit reverse sequence below, activations in bf16, gradients accumulated straight into the flat
fp32 gradient arena, per-stage callbacks so the data-parallel wrapper can start the RCCL all-reduce of a finished
parameter range while earlier layers are still in backward.
"""
import ctypes
import functools
import itertools
import os
import weakref
from typing import Optional, Tuple

import torch

from . import block_calls as BC
from . import encoder_blocks as EB
from . import ops
from .arena import enc_block_views
from .parallel import LOCAL, LocalComm, bn_backward, bn_forward  # noqa: F401  (LocalComm: part of this module's interface)

BF16, F32 = torch.bfloat16, torch.float32
FWD_MODE = os.environ.get("DIG_FWD_MODE", "flip")                   # two-stream plan of the forward (single process): "flip" (default) or "side"
CHAIN_BWD_EVERY = max(1, int(os.environ.get("DIG_CHAIN_BWD_EVERY", "1")))   # with DIG_MLP_CHAIN_MASK bit 2: the fused MLP backward in every k-th block only
CHAIN_BWD_PHASE = int(os.environ.get("DIG_CHAIN_BWD_PHASE", "0"))
BATCH_REDUCE = os.environ.get("DIG_BATCH_REDUCE", "0") == "1"       # an encoder block's eleven reduction launches as two: fewer launches,
#                                                                     0.1-0.15 ms SLOWER per step -> opt-in
FUSED_QV_BIAS_SUMS = os.environ.get("DIG_FUSED_QV_BIAS", "1") != "0"
# weight gradients of an encoder block on the grouped kernel (csrc/wgrad.hip): "block" = one launch per block (default: the block's
# accumulators are dumped once), "pair" = MLP pair | attention pair, "off" = the tiled split-R launches + their slab sums
WGRAD_GROUPING = os.environ.get("DIG_WGRAD_GROUPING", "block")
# The grouped weight-gradient launch owns the chip (one 8-wave workgroup per CU with every register and 140 KiB of LDS), and so do the fused
# MLP backward and the 256-row data-gradient tiles: beside it on a second stream the chain's next kernel only waits for CUs (its in-step
# duration grows by the launch's length, the step does not get shorter).  "1": the launch sits IN the data-gradient chain, on the caller's
# stream, between attention backward and the qkv data gradient -- back-to-back kernel boundaries instead of cross-stream events; the small
# reductions (bias / LayerNorm-parameter column sums) stay on the second stream.
WGRAD_INLINE = os.environ.get("DIG_WGRAD_INLINE", "1") == "1"
# Block-call path: all twelve grouped weight-gradient launches behind the LAST data gradient instead of inside each block's chain.  "auto"
# (default): deferred in a single process (nothing waits for a block's gradients before the optimizer: 19.96 -> 19.83 ms per step, A/B on one
# box), inline under a process group (a block's bucket must be final as early as possible: its all-reduce overlaps the rest of the backward).
# "1" / "0" force either plan.  Deferring keeps every block's gradient temporaries alive until the end of the backward (~0.45 GB per ViT-S block).
# "auto" also checks the device's free memory against what the deferred plan keeps alive (depth x the block's bf16 temporaries + the saved
# activations no longer released block by block: ~5.4 GB more at the end of the backward for ViT-S at B = 128) and stays inline when that
# would not leave a quarter of the free memory.
WGRAD_DEFER = os.environ.get("DIG_WGRAD_DEFER", "auto").strip().lower()
if WGRAD_DEFER not in ("auto", "0", "1"):
    raise ValueError(f"DIG_WGRAD_DEFER={WGRAD_DEFER!r}: one of auto, 0, 1")
# Block-call path, single process: the blocks' parameter-gradient reductions (five small launches per block on the second stream: 61 per step, each
# taking CU slots from the chip-owning kernel of the data-gradient chain that runs beside it) held back and folded in ONE
# dig_colsum_partials_multi launch behind the last data gradient (108 segments; the same sums).  "0": per block, on the second stream.
RED_DEFER = os.environ.get("DIG_RED_DEFER", "1") != "0"
BWD_SINGLE_STREAM = os.environ.get("DIG_BWD_SINGLE", "0") == "1"    # lab switch: the whole backward on the caller's stream (sum of solo kernel times)


# Lab: GPU time stamps at the phase boundaries of a step without a profiler (tools/gpu_step_phases.py sets PHASE_MARKS = []): events on the
# caller's stream, resolved by the tool after a synchronise.
PHASE_MARKS = None


def _mark(name, dev):
    if PHASE_MARKS is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(dev))
        PHASE_MARKS.append((name, ev))


# the head stacks of the two branches: (arena, pix_projector, patch_extractor, projection layer, predictor)
ONLINE_HEADS = ("online", "pix_projector", "patch_extractor", "encoder_projection_layer", "predictor")
MOMENTUM_HEADS = ("momentum", "pix_projector_m", "momentum_patch_extractor", "momentum_projection_layer", None)


class _EncWeights:
    """Per-encoder (online / momentum) accessors resolved once per arena binding."""

    def __init__(self, model, prefix, arena):
        f32, g32 = model._f32, model._g32 if arena == "online" else {}
        self.blocks = enc_block_views(model.specs, prefix, model.depth, model.D, model._flat[arena], model.shadow(arena),
                                      model._flat["grad"] if g32 else None)
        self.pe_w = f32[prefix + "patch_embed.proj.weight"].view(model.D, 48)
        self.pe_b = f32[prefix + "patch_embed.proj.bias"]
        self.mask_token = f32[prefix + "mask_token"].view(model.D)
        if g32:
            self.g_pe_w = g32[prefix + "patch_embed.proj.weight"].view(model.D, 48)
            self.g_pe_b = g32[prefix + "patch_embed.proj.bias"]
            self.g_mask_token = g32[prefix + "mask_token"].view(model.D)


def _weights(model):
    cache = getattr(model, "_wcache", None)
    mom = getattr(model, "use_moco_target", True)
    if cache is None or cache[0] != model._views_version or model._shadow.get("online") is None or (mom and model._shadow.get("momentum") is None):
        model.shadow("online")
        if mom:
            model.shadow("momentum")
        model._w16 = None
        cache = (model._views_version, _EncWeights(model, "encoder.", "online"),
                 _EncWeights(model, "momentum_encoder.", "momentum") if mom else None)
        model._wcache = cache
    return cache[1], cache[2]


class _Step:
    def __init__(self, model):
        self._keep = []                             # tensors the side stream still reads (see _on_side)
        self._keep_marks = []                       # (event on the side stream, length of _keep it covers): see _release_kept
        self.m = model
        self.comm = model.comm or LOCAL

    # ------------------------------------------------------------------ encoder
    def _path_specs(self, plan, site_off):
        """[(attention-branch DropSpec, MLP-branch DropSpec) or None per block] for stochastic depth under `plan` (dropout.DropPlan)."""
        from . import dropout as DR
        M = self.m
        out = []
        for i, p in enumerate(M.dpr):
            if not p:
                out.append(None)
                continue
            out.append((plan.spec(0, 0.0, path_site=DR.enc_site(i + site_off, 2), path_p=p, rows_per_sample=M.N),
                        plan.spec(0, 0.0, path_site=DR.enc_site(i + site_off, 4), path_p=p, rows_per_sample=M.N)))
        return out

    def encoder_forward(self, ew, images, aug, mask_u8, save, views=2, path=None):
        """views = 1: the encoder over `images` only (Gen-only models with only_mim_on_ori_img: the samples of a ViT batch are independent, and
        nothing downstream reads the augmented view's rows).  path: per-block stochastic-depth specs (_path_specs) or None."""
        M = self.m
        B, D, H, N = images.shape[0], M.D, M.H, M.N
        R = views * B * N
        x = torch.empty((R, D), device=images.device, dtype=BF16)
        for half, im in enumerate((images, aug)[:views]):
            ops.L.call("dig_patch_embed_fwd", ops.L.ptr(im), ops.L.ptr(ew.pe_w), ops.L.ptr(ew.pe_b),
                       ops.L.ptr(mask_u8[half * B:(half + 1) * B]), ops.L.ptr(ew.mask_token), ops.L.ptr(M._pos),
                       ops.L.ptr(x[half * B * N:(half + 1) * B * N]), B, M.gh, M.gw, D, ops.L.stream())
        chain = ops.mlp_chain_supported(D, M.F, R) and bool(ops.MLP_CHAIN_MASK & (2 if save else 1))
        plan = EB.Plan(chain=chain, chain_ln=chain and ops.MLP_CHAIN_LN and M.F <= 2048,
                       attn_block=ops.attn_block_supported(H, D, B if views == 1 else None))
        if plan.chain_ln and ops.BLOCK_CALLS and D == H * 64 and path is None:
            return BC.forward(ew.blocks, x, views * B, H, M.F, M.ln_eps, save, fuse_attn=plan.attn_block)
        drops = [ds and (None, ds[0], ds[1]) for ds in path] if path is not None else None
        x, saved, _ = EB.forward(plan, ew.blocks, x, views * B, H, M.ln_eps, save, drops=drops)
        return x, saved

    def mlp_weight_transposes(self, ew, fresh=False):
        """K-contiguous copies of the MLP weights for the fused backward (W2^T [F, D], W1^T [D, F]; 1.2 MB each) and of the projection weight.
        Normally the previous step's optimizer launch has written them (dig_adamw_step_tr, MoCo_ViT.transposed_weight_table): `fresh` ->
        no launch at all.  Otherwise (first step, after load_state_dict / .to(), under graph capture, DIG_ADAMW_FOLD=0) three launches
        rebuild them from this step's bf16 weight shadow, into the same persistent buffers where the model has them."""
        tr = self.m.transposed_weight_table() if hasattr(self.m, "transposed_weight_table") else None
        self.head_wT = {}
        if tr is not None and fresh:
            self.head_wT = tr[6]
            return tr[4]
        outs = tr[4] if tr is not None else None
        w2t = ops.transpose_bf16_multi([b["mlp.fc2.weight"] for b in ew.blocks], [o[0] for o in outs] if outs else None)   # one launch per weight shape
        w1t = ops.transpose_bf16_multi([b["mlp.fc1.weight"] for b in ew.blocks], [o[1] for o in outs] if outs else None)
        projt = ops.transpose_bf16_multi([b["attn.proj.weight"] for b in ew.blocks], [o[2] for o in outs] if outs else None)
        qkvt = ops.transpose_bf16_multi([b["attn.qkv.weight"] for b in ew.blocks], [o[3] for o in outs] if outs else None)   # (direct-form qkv data gradient)
        if tr is not None:                                              # (the heads' copies: one small launch each, only behind a foreign write)
            w16 = self.m._w("online")
            for name, dst in tr[6].items():
                ops.transpose_bf16(w16[name], dst)
            self.head_wT = tr[6]
        return list(zip(w2t, w1t, projt, qkvt))

    def _backward_transposes(self, ew, training, rows, fresh):
        """mlp_weight_transposes where the backward over `rows` encoder rows reads them (the fused MLP backward's operands; the direct-form data
        gradients), else None."""
        M = self.m
        if training and ((ops.mlp_chain_supported(M.D, M.F, rows) and (ops.MLP_CHAIN_MASK & 4)) or (ops.DGRAD_DIRECT and rows >= 8192)):
            return self.mlp_weight_transposes(ew, fresh)
        return None

    # ------------------------------------------------------------------ two-stream helpers (backward)
    def _streams(self, dev):
        M = self.m
        main = torch.cuda.current_stream(dev)
        side = M._bwd_side_stream(dev) if (getattr(M, "overlap_streams", True) and not BWD_SINGLE_STREAM) else main
        return main, side

    def _on_side(self, dev, fn, *tensors):
        """Run fn (weight-gradient GEMMs, column sums: consumers of tensors the main chain has just produced) on the side
        stream, after everything the main stream has queued so far."""
        main, side = self._streams(dev)
        if side is main:
            fn()
            return
        side.wait_stream(main)
        with torch.cuda.stream(side):
            fn()
        # the side stream reads tensors of the caller's stream's pool: instead of record_stream (an event on the side stream per block when
        # it is released: ~120 per backward, 0.5+ ms of queue time) they are kept alive until backward() has joined the two streams
        self._keep.extend(tensors)

    def _mark_kept(self, dev):
        """Everything _on_side() has kept so far is dead once the side stream passes this point."""
        main, side = self._streams(dev)
        if side is main or not self._keep:
            return
        ev = torch.cuda.Event()
        ev.record(side)
        self._keep_marks.append((ev, len(self._keep)))

    def _release_kept(self, dev, lag=2):
        """Drop the kept tensors of marks at least `lag` marks old: the caller's stream waits for that mark (the side stream is never two
        encoder blocks behind, so the wait is already satisfied when it is reached) and the blocks go back to its pool -- without this
        every block's gradient temporaries stayed resident until the end of backward (~0.7 GB per ViT-S block at B = 256)."""
        main, side = self._streams(dev)
        while len(self._keep_marks) > lag:
            ev, n = self._keep_marks.pop(0)
            main.wait_event(ev)
            del self._keep[:n]
            self._keep_marks = [(e, m - n) for e, m in self._keep_marks]

    def _grad_ready(self, dev, key):
        """Bucket `key` is final once both streams pass this point.  With a process group the all-reduce is issued from the
        side stream after it has waited for the main chain, so the main chain never stalls on a collective."""
        main, side = self._streams(dev)
        if side is not main and (self.comm.world > 1 or getattr(self.comm, "world_override", False)):
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self.comm.grad_ready(self.m, key)
        else:
            self.comm.grad_ready(self.m, key)

    def _backward_plan(self, chain, have_wT, rows, path):
        """The per-entry-point backward's plan (encoder_blocks.Plan) from this module's and ops' switches as they stand NOW.
        Grouped weight gradients: shapes the grouped kernel does not take (tiny test models) keep the per-layer launches.  red_defer: single
        process (the 512-wide model, single-view encoders): the blocks' bias / LayerNorm column-sum launches held back as in
        the block-call backward -- collected over ALL blocks and folded in one dig_colsum_partials_multi launch behind the walk."""
        D, Fh = self.m.D, self.m.F
        grouped = (ops.WGRAD_GROUP and WGRAD_GROUPING != "off" and
                   all(ops.wgrad_group_route(o, i_, rows) is not None for o, i_ in ((Fh, D), (D, Fh), (3 * D, D), (D, D))))
        return EB.Plan(chain_bwd=chain, chain_every=CHAIN_BWD_EVERY, chain_phase=CHAIN_BWD_PHASE, chain_lnb=ops.MLP_CHAIN_LNB,
                       chain_proj=ops.MLP_CHAIN_PROJ, direct=have_wT, fused_qv=FUSED_QV_BIAS_SUMS,
                       attn_proj=bool(ops.ATTN_BWD_PROJ and FUSED_QV_BIAS_SUMS and have_wT and ops.attn_bwd_proj_supported(D)
                                      and not ops.attn_bwd_mode()),
                       grouping=WGRAD_GROUPING if grouped else "off", inline=WGRAD_INLINE, batch_reduce=BATCH_REDUCE,
                       red_defer=bool(RED_DEFER and self.comm is LOCAL and path is None and not BATCH_REDUCE and PHASE_MARKS is None))

    def _block_call_plan(self, dev, n_img, R):
        """The block-call backward's plan (block_calls.Plan) from this module's and ops' switches as they stand NOW.  defer "auto": see
        WGRAD_DEFER -- a single process, and the device has the memory for what the deferred plan keeps alive."""
        M, local = self.m, self.comm is LOCAL
        kept = M.depth * ops.block_bwd_layout(R, M.D, M.F, n_img)[1]
        defer = WGRAD_DEFER == "1" or (WGRAD_DEFER == "auto" and local and BC.defer_fits(M.__dict__.setdefault("_defer_fits_cache", {}), dev, kept))
        return BC.Plan(defer=defer, red_defer=bool(RED_DEFER and defer and local and ops.MLP_CHAIN_LNB and M.depth * 9 <= ops.COLSUM_MAX_SEGS),
                       tile_direct=ops.dgrad_direct_tile_code(R, M.D),
                       attn_proj=bool(ops.ATTN_BWD_PROJ and ops.attn_bwd_proj_supported(M.D) and not ops.attn_bwd_mode()),
                       fuse_ln2=bool(ops.MLP_CHAIN_LNB), chain_proj=bool(ops.MLP_CHAIN_LNB and ops.MLP_CHAIN_PROJ))

    @staticmethod
    def _takes_block_calls(plan, path, saved, dx):
        """Whether the block-call backward (block_calls.backward) computes what `plan` asks for: it is the default plan -- one grouped launch
        per block in the chain, the fused MLP backward in every block, fused q / v bias sums -- without stochastic depth, batched reductions
        or phase marks, behind a block-call forward."""
        return (ops.BLOCK_CALLS and plan.grouping == "block" and plan.inline and plan.chain_bwd and plan.chain_every == 1 and plan.fused_qv
                and path is None and not plan.batch_reduce and PHASE_MARKS is None and all(isinstance(s_, BC._BlockSaved) for s_ in saved)
                and dx.is_contiguous())

    def encoder_backward(self, ew, saved, dx, images, aug, mask_u8, views=2):
        """dx: bf16 [R, D] gradient w.r.t. the encoder output (consumed).
        The data-gradient chain (dgrad GEMMs, attention backward, LayerNorm backward) runs on the caller's stream; the
        weight-gradient GEMMs and bias column sums only consume (dy, saved activation) pairs, so they are issued on a
        second HIP stream and overlap the chain (both are latency-bound kernels that leave CU resources idle)."""
        M = self.m
        B, D, H, N = images.shape[0], M.D, M.H, M.N
        dev = dx.device
        main, side = self._streams(dev)
        n_img, R = views * B, views * B * N
        chain = ops.mlp_chain_supported(D, M.F, R) and bool(ops.MLP_CHAIN_MASK & 4)
        wT = getattr(self, "wT", None)
        if chain and wT is None:
            wT = self.mlp_weight_transposes(ew)
        elif wT is not None:
            for pair_ in wT:                                            # made on the side stream in forward(), read here on the main one
                for t in pair_:
                    t.record_stream(main)
        path = getattr(self, "path_on", None)
        plan = self._backward_plan(chain, wT is not None, R, path)
        grad_ready = functools.partial(self._grad_ready, dev)

        def block_done():
            self._mark_kept(dev)
            self._release_kept(dev)
        wplan = ops.wgrad_block_plan(dev, R, D, M.F) if self._takes_block_calls(plan, path, saved, dx) else None
        if wplan is not None:
            dx = BC.backward(self._block_call_plan(dev, n_img, R), ew.blocks, saved, dx, wT, wplan, n_img, H, M.F,
                             ctypes.c_void_p(side.cuda_stream), keep=self._keep.append if side is not main else None,
                             block_done=block_done, grad_ready=grad_ready)
        else:
            drops = [ds and (None, ds[0], ds[1]) for ds in path] if path is not None else None
            # views == 1: only view 0 carries a gradient (zero contrastive weight): rows [0, B*N) of everything.  A bucket's all-reduce is issued
            # from the side stream after it has waited for the main chain (_grad_ready), so the main chain never stalls on the collective
            dx = EB.backward(plan, ew.blocks, saved, dx, wT, n_img, H, functools.partial(self._on_side, dev), drops=drops, rows=R if views == 1 else None,
                             block_done=block_done, grad_ready=grad_ready, mark=_mark)
        for half, im in enumerate((images, aug)[:views]):
            ops.patch_embed_bwd_mfma(dx[half * B * N:(half + 1) * B * N], im, mask_u8[half * B:(half + 1) * B], ew.g_pe_w, ew.g_pe_b,
                                     ew.g_mask_token, D, M.gh, M.gw)
        main.wait_stream(side)
        self.comm.grad_ready(M, "encoder.embed")

    # ------------------------------------------------------------------ BN-MLP heads
    def mlp_forward(self, stacks):
        """_build_mlp stacks (modeling_pretrain_moco_mim_ori.py:463-482: Linear(no bias) -> BN(train, cross-rank stats) -> ReLU ... ; the last BN
        has no affine parameters) of the same layer widths, given as [(x, prefix, arena, save)] and run layer by layer in lock step: the
        cross-rank BatchNorm statistics of a layer travel in ONE all-reduce ([stacks, 2, C]) -- with the online head and its momentum twin as
        the two stacks, 14 -> 8 latency-bound collectives per forward, all issued from one stream in program order (the all-reduce is
        elementwise: the same arithmetic per stack as on its own).  What the backward of a `save` stack needs is kept in
        self.saved_heads[prefix].  Returns the stacks' outputs."""
        M = self.m
        dims = M.mlps[stacks[0][1]]
        assert all(M.mlps[pre] == dims for _, pre, _, _ in stacks)
        xs = [x for x, _, _, _ in stacks]
        saved = [[] for _ in stacks]
        for l in range(len(dims)):
            last = l == len(dims) - 1
            hs = [ops.linear_fwd(x, M._w(arena)[f"{pre}.{3 * l}.weight"]) for x, (_, pre, arena, _) in zip(xs, stacks)]
            outs = bn_forward(self, hs, [f"{pre}.{3 * l + 1}" for _, pre, _, _ in stacks], relu=not last, affine=not last)
            for k, (y, mean, rstd) in enumerate(outs):
                if stacks[k][3]:
                    saved[k].append((xs[k], hs[k], mean, rstd))
                xs[k] = y
        self.saved_heads.update({pre: kept for (_, pre, _, save), kept in zip(stacks, saved) if save})
        return xs

    def mlp_backward(self, dy, pre, need_dx=True, dx_out=None):
        M = self.m
        dims, saved = M.mlps[pre], self.saved_heads[pre]
        w16, g32 = M._w("online"), M._g32
        for l in reversed(range(len(dims))):
            last = l == len(dims) - 1
            x, h, mean, rstd = saved[l]
            dh = bn_backward(self, dy, h, mean, rstd, f"{pre}.{3 * l + 1}", relu=not last, affine=not last)
            # (every head weight is used once per forward: right after zero_grad() its gradient can be written instead of added)
            asg = getattr(self, "_assign", False)
            self._on_side(dy.device, lambda: ops.linear_wgrad(dh, x, g32[f"{pre}.{3 * l}.weight"], assign=asg), dh, x)
            if l > 0 or need_dx:
                wt = getattr(self, "head_wT", {}).get(f"{pre}.{3 * l}.weight") if ops.HEAD_DGRAD_DIRECT else None
                if wt is not None:
                    # direct form on the K-contiguous copy the optimizer launch left (the forward's tile plan for this shape)
                    dy = ops.linear_fwd(dh, wt, out=dx_out if l == 0 else None)
                else:
                    dy = ops.linear_dgrad(dh, w16[f"{pre}.{3 * l}.weight"], out=dx_out if l == 0 else None)
        return dy

    # ------------------------------------------------------------------ full forward
    def forward(self, images, aug, mask_b2n, m, mim_views=1, training=False):
        """training: a backward will follow (set by the autograd node: inside its forward() autograd's grad mode is off, so
        torch.is_grad_enabled() says nothing).
        mim_views: 1 = only_mim_on_ori_img (the README recipe: the decoder runs on view 0's masked rows), 2 = both views' masked rows
        (modeling_pretrain_moco_mim_ori.py:572-577)."""
        M = self.m
        dev = images.device
        B, D, N, nw = images.shape[0], M.D, M.N, M.num_windows
        comm = self.comm
        self.B = B
        self._bn_touched = []
        self.saved_heads = {}                       # prefix of a head stack -> what its backward needs (mlp_forward, patch_extractor)
        images = images.contiguous().float()
        aug = aug.contiguous().float()
        if mask_b2n.dtype == torch.uint8 and mask_b2n.dim() == 2 and tuple(mask_b2n.shape) == (2 * B, N):
            mask_u8 = mask_b2n if mask_b2n.is_contiguous() else mask_b2n.contiguous()      # prepared by the engine: view-major rows already
        else:
            mask_u8 = mask_b2n.permute(1, 0, 2).reshape(2 * B, N).to(torch.uint8).contiguous()    # rows 0..B-1 = view 0 (:497)
        if not M.use_pixel_target:
            # Dis-only: `if not self.use_pixel_target: vis_mask_pos = None` (modeling_pretrain_moco_mim_ori.py:493-494) -- no token is replaced
            zm = getattr(M, "_zero_mask", None)
            if zm is None or zm.shape != (2 * B, N) or zm.device != dev:
                zm = M._zero_mask = torch.zeros((2 * B, N), device=dev, dtype=torch.uint8)
            mask_u8 = zm
        self.images, self.aug, self.mask_u8 = images, aug, mask_u8
        ew_on, ew_mo = _weights(M)
        pp = M.has_pix_projector
        _mark("forward: start", dev)
        # the bf16 operand shadow of the online arena (and the transposed weight copies below): left by the previous step's optimizer launch
        # unless something else has written the parameters since (MoCo_ViT.weights_fresh)
        fresh = M.weights_fresh() and not torch.cuda.is_current_stream_capturing()
        if not fresh:
            ops.cast_f32_to_bf16(M._flat["online"], M.shadow("online"))
        # stochastic depth (--drop_path): this step's keys; the online encoder's specs are kept for the backward
        self.path_on = self.path_mo = None
        if M.drop_path_rate > 0 and M.training:
            from . import dropout as DR
            plan = DR.DropPlan(M.drop_seed, M.drop_step)
            M.drop_step += 1
            self.path_on, self.path_mo = self._path_specs(plan, 0), self._path_specs(plan, 64)
        if not M.use_moco_target:
            return self._forward_gen_only(ew_on, images, aug, mask_u8, mim_views, training, fresh)
        # ---- momentum branch (no grad) on a second HIP stream: it depends only on the pre-step online weights (fp32
        # arena, read-only here) and the inputs, so it overlaps the online forward.  EMA with the current online weights
        # comes first (:526).
        main = torch.cuda.current_stream(dev)
        side = M._fwd_stream(dev) if (getattr(M, "overlap_streams", True) and FWD_MODE != "serial") else main
        dist_mode = comm.world > 1 or getattr(comm, "world_override", False)
        mode = FWD_MODE if (not dist_mode and side is not main) else "side"

        regular = M.patchnet == 'regular'

        def extract(masked, enc_rows, pre, arena, save):
            """patch_extractor (PatchNet.forward, :189-205): the pooled windows of [masked view | augmented view]; with --patchnet_name regular
            they then attend over all tokens of their image (dig_amd/patchnet.py)."""
            if M.patchnet == 'conv':
                # ConvPatchNet (:207-260): no window pooling in front -- the token maps of both views through the convolution stack, one row per image
                from . import convpatchnet
                feat = torch.cat([masked, enc_rows[B * N:]]) if masked.data_ptr() != enc_rows.data_ptr() else enc_rows
                return convpatchnet.forward(self, feat, pre, arena, 2 * B, save)
            pooled = torch.empty((2 * B * nw, D), device=dev, dtype=BF16)
            ops.window_pool_fwd(masked, pooled[:B * nw], B, M.gh, M.gw, nw, D)
            ops.window_pool_fwd(enc_rows[B * N:], pooled[B * nw:], B, M.gh, M.gw, nw, D)
            if not regular:
                return pooled, None
            from . import patchnet
            # (the image tokens of both views as one [2 B N, D] matrix: without a pix_projector that is the encoder output itself)
            feat = torch.cat([masked, enc_rows[B * N:]]) if masked.data_ptr() != enc_rows.data_ptr() else enc_rows
            return patchnet.forward(self, feat, pooled, pre, arena, 2 * B, save)

        def heads(encs, branches):
            """The head pipeline (:500-558) of `branches` (ONLINE_HEADS / MOMENTUM_HEADS) over their encoders' outputs, stage by stage in lock
            step (mlp_forward): pix_projector -> patch_extractor -> projection layer, then the predictor where a branch has one.  Returns q / k
            per branch."""
            def stage(xs, j):
                return self.mlp_forward([(x, br[j], br[0], br[0] == "online") for x, br in zip(xs, branches)])
            # (`if hasattr(self, 'pix_projector')`, :500-510: the Dis-only models pool the encoder's own rows of both views)
            xs = stage([enc[:B * N] for enc in encs], 1) if pp else [enc[:B * N] for enc in encs]
            pooled = []
            for x, enc, br in zip(xs, encs, branches):
                y, kept = extract(x, enc, br[2], br[0], br[0] == "online")
                if br[0] == "online":
                    self.saved_heads[br[2]] = kept
                pooled.append(y)
            outs = stage(pooled, 3)
            return [self.mlp_forward([(x, br[4], br[0], True)])[0] if br[4] else x for x, br in zip(outs, branches)]

        def momentum_branch(with_heads=True):
            ops.ema_update(M._flat["momentum"], M._flat["online"], M.shadow("momentum"), M.n_ema, m)
            # K-contiguous copies of the online weights for the backward: left by the optimizer launch, or rebuilt here in front of the momentum
            # encoder from this step's shadow
            self.wT = self._backward_transposes(ew_on, training, 2 * B * N, fresh)
            enc_m, _ = self.encoder_forward(ew_mo, images, aug, mask_u8, False, path=self.path_mo)
            return enc_m, (heads([enc_m], [MOMENTUM_HEADS])[0] if with_heads else None)

        def decoder():
            # SimMIM decoder on the masked tokens (:560-570; the reference decodes all rows then selects): view 0 only, or both views
            return self._decoder_forward(mask_u8, images, mim_views), None

        vis_out = None
        if mode == "flip":
            # The big forward kernels own the whole chip one at a time (persistent GEMM tiles and the fused MLP chain: one workgroup per CU
            # with all of its LDS / registers), so the two branches serialise kernel by kernel whatever streams they are on, and the question
            # is only WHO goes first: the online branch on the HIGH-priority stream, the momentum branch on the caller's (23.76 -> 23.58 ms).
            # Workgroup dispatch is strictly by priority: the momentum branch's first kernel starts when the online branch is ~0.5 ms into its
            # ~60 head kernels (rocprofv3 timeline).  Measured alternatives, same box: both encoders on one stream with the online heads and
            # the SimMIM decoder on the other at higher (24.32 ms), equal (24.33) or lower (24.21) priority against 23.74 -- a small kernel
            # that holds a few CUs when a persistent one-workgroup-per-CU kernel starts delays that whole kernel by its own length, 72 times.
            hi_st = M._side_stream(dev)
            hi_st.wait_stream(main)
            with torch.cuda.stream(hi_st):
                enc, self.saved_enc = self.encoder_forward(ew_on, images, aug, mask_u8, True, path=self.path_on)
                self.enc = enc
                qs = heads([enc], [ONLINE_HEADS])[0]
            # (Measured and not kept, round 4: the SimMIM decoder right behind the online heads instead of after the join: 21.06 vs 21.07 ms.)
            # (Measured and not kept, round 4: the online heads + SimMIM decoder held back until both encoders are done, so that they run
            #  beside the momentum heads instead of between the encoders: 21.84 vs 21.77 ms, two A/B pairs.)
            enc_m, ks = momentum_branch()
            del enc_m
            main.wait_stream(hi_st)
        else:
            # momentum branch (no grad) on a second HIP stream: it depends only on the pre-step online weights (fp32 arena, read-only
            # here) and the inputs.  EMA with the current online weights comes first (:526).
            side.wait_stream(main)
            with torch.cuda.stream(side):
                enc_m, ks = momentum_branch(with_heads=not dist_mode)
            enc, self.saved_enc = self.encoder_forward(ew_on, images, aug, mask_u8, True, path=self.path_on)
            self.enc = enc
            if not dist_mode:
                qs = heads([enc], [ONLINE_HEADS])[0]
                main.wait_stream(side)
                if side is not main:
                    ks.record_stream(main)
                del enc_m
            else:
                # with a process group the heads of both branches run together on this stream, after both encoders: one BatchNorm-
                # statistics all-reduce per layer PAIR, issued in program order (no collective of the momentum branch in front of the
                # online branch's first one on RCCL's in-order stream)
                main.wait_stream(side)
                enc_m.record_stream(main)
                qs, ks = heads([enc, enc_m], [ONLINE_HEADS, MOMENTUM_HEADS])
                del enc_m
        _mark("forward: both encoders + heads joined", dev)
        M._flat["bn_count"] += 1                                            # all 14 (Dis-only: 8) BatchNorm layers ran once
        # ---- InfoNCE (:444-461): q1 vs gathered k2, q2 vs gathered k1, labels = arange + n*rank
        n = B * M.n_patch                                                   # rows of q1 / q2
        dim = M.moco_dim
        qf = torch.empty((2 * n, dim), device=dev, dtype=F32)
        kf = torch.empty((2 * n, dim), device=dev, dtype=F32)
        ops.cast_bf16_to_f32(qs, qf)
        ops.cast_bf16_to_f32(ks, kf)
        qn, self.q_inv = ops.l2norm_fwd(qf)
        kn, _ = ops.l2norm_fwd(kf)
        self.qn = qn
        if dist_mode:
            kall = comm.all_gather_cat(kn.view(1, 2, n, dim))               # [W, 2, n, dim], rank order (:586-590)
            k1_all = kall[:, 0].reshape(comm.world * n, dim).contiguous()
            k2_all = kall[:, 1].reshape(comm.world * n, dim).contiguous()
        else:
            k1_all, k2_all = kn[:n], kn[n:]
        mk = comm.world * n
        stats = torch.zeros((2, 3), device=dev, dtype=F32)
        self.dqn = torch.empty((2 * n, dim), device=dev, dtype=F32)
        gs = 2.0 * M.T / n                                                  # d(mean CE * 2T)/dlogits scale
        for half, kk in ((0, k2_all), (1, k1_all)):
            logits = torch.empty((n, mk), device=dev, dtype=F32)
            ops.sgemm(qn[half * n:(half + 1) * n], kk, logits, n, mk, dim, False, 1.0 / M.T)
            ops.ce_rows(logits, n * comm.rank, gs, stats[half])
            ops.sgemm(logits, kk, self.dqn[half * n:(half + 1) * n], n, dim, mk, True, 1.0 / M.T)
        contra, accs = ops.infonce_finish(stats, 2.0 * M.T / n, 100.0 / n)   # accs: q1_acc1, q1_acc5, q2_acc1, q2_acc5
        if not M.use_pixel_target:
            vis_out = torch.empty((0, 0, M.dec_classes), device=dev, dtype=F32)     # (no 'vis_out' key for a Dis-only model: dig_forward)
            self.mim_views = 0
        elif vis_out is None:
            vis_out, _ = decoder()
        _mark("forward: InfoNCE + SimMIM decoder done", dev)
        return contra, accs, vis_out

    def _decoder_forward(self, mask_u8, images, mim_views):
        """pix_decoder on the masked rows of self.enc (modeling_pretrain_moco_mim_ori.py:560-570; the reference decodes all rows, then selects)."""
        M = self.m
        B, N, dev = images.shape[0], M.N, images.device
        per = M._mask_count(mask_u8, B)
        Mrows = mim_views * B * per
        Mp = (Mrows + 63) // 64 * 64
        idx, cnt = ops.mask_to_index(mask_u8[:mim_views * B], per)
        M._last_mask_counts, M._last_idx, M._last_images = cnt, idx[:B], images
        M._last_idx_views = [idx[:B]] + ([(idx[B:] - B * N).clamp_min_(0)] if mim_views == 2 else [])
        self.idx, self.Mrows, self.Mp, self.per, self.mim_views = idx, Mrows, Mp, per, mim_views
        w16, f32 = M._w("online"), M._f32
        gath = ops.gather_rows(self.enc, idx, Mrows, Mp)
        h0 = ops.linear_fwd(gath, w16["pix_decoder.0.weight"])
        h1 = ops.linear_fwd(h0, w16["pix_decoder.1.weight"])
        h2, mu, rs = ops.layernorm_fwd(h1, f32["pix_decoder.2.weight"], f32["pix_decoder.2.bias"], M.ln_eps, gelu=True)
        pred = torch.empty((Mp, 64), device=dev, dtype=F32)
        C = M.dec_classes
        ops.gemm(h2, w16["pix_decoder.4.weight"], Mp, C, M.dec_dim, out=pred, out_kind=ops.OUT_F32, bias=f32["pix_decoder.4.bias"], ldc=64)
        self.saved_dec = (gath, h0, h1, h2, mu, rs)
        return pred[:Mrows, :C].reshape(mim_views * B, per, C)

    def _forward_gen_only(self, ew_on, images, aug, mask_u8, mim_views, training, fresh):
        """MoCo_ViT.forward of a Gen-only model (use_moco_target=False: pretrain_simmim_ori_*, modeling_pretrain_moco_mim_ori.py:655-681):
        encoder -> its final LayerNorm (modeling_pretrain_vit.py:104; the moco branch is what replaces it by nn.Identity) -> pix_decoder on
        the masked rows.  The reference runs the augmented view through the encoder as well and reads none of its rows when
        only_mim_on_ori_img: the samples of a ViT batch are independent, so that view is not launched here (3 F per sample instead of 6)."""
        M = self.m
        dev = images.device
        views = mim_views
        self.gen_views = views
        self.wT = self._backward_transposes(ew_on, training, views * self.B * M.N, fresh)
        enc_raw, self.saved_enc = self.encoder_forward(ew_on, images, aug, mask_u8, True, views=views, path=self.path_on)
        f32 = M._f32
        self.enc, mu, rs = ops.layernorm_fwd(enc_raw, f32["encoder.norm.weight"], f32["encoder.norm.bias"], M.ln_eps)
        self.saved_norm = (enc_raw, mu, rs)
        vis_out = self._decoder_forward(mask_u8, images, mim_views)
        # (no 'contra_loss' / accuracy keys for a Gen-only model: dig_forward drops these two; an operator's outputs must not alias each other)
        return torch.zeros((), device=dev, dtype=F32), torch.zeros(4, device=dev, dtype=F32), vis_out

    # ------------------------------------------------------------------ full backward
    def backward(self, g_contra, g_vis):
        M = self.m
        B, D, N, nw = self.B, M.D, M.N, M.num_windows
        dev = self.enc.device
        w16, f32, g32 = M._w("online"), M._f32, M._g32
        # ---- contrastive path.  g_contra is None when the loss did not use contra_loss (zero contrastive weight: epochs before
        # contrast_start_epoch, BASELINE config 2): every gradient of that branch -- predictor, projector, pix_projector and
        # the whole augmented view -- is exactly zero in the reference, so nothing is launched for it and the encoder
        # backward runs on view 0's rows only (the gradient arena was zero-filled by optimizer.zero_grad()).
        contrast = g_contra is not None and M.use_moco_target
        if g_vis is not None and not M.use_pixel_target:
            g_vis = None
        # the arena is known to be zero only right after optimizer.zero_grad(): a second backward() without it accumulates, as torch does
        self._assign, M._grads_fresh = bool(getattr(M, "_grads_fresh", False)), False
        _mark("backward: start (loss, MSE, autograd entry done)", dev)
        views = 2 if (contrast or (g_vis is not None and self.mim_views == 2)) else 1      # encoder rows that carry a gradient
        # (Dis-only: no pix_projector writes view 0's rows -- both halves come from the pooling gradient, which overwrites)
        d_enc = torch.empty_like(self.enc) if contrast else torch.zeros((views * B * N, D), device=dev, dtype=BF16)
        n = B * M.n_patch
        if contrast:
            dqn = self.dqn
            ops.scale_by_device_scalar(dqn, g_contra.reshape(1).float())
            dq = ops.l2norm_bwd(dqn, self.qn, self.q_inv)
            dq16 = torch.empty(dq.shape, device=dev, dtype=BF16)
            ops.cast_f32_to_bf16(dq, dq16)
            dproj = self.mlp_backward(dq16, "predictor")
            self._grad_ready(dev, "predictor")
            dpool = self.mlp_backward(dproj, "encoder_projection_layer")
            self._grad_ready(dev, "encoder_projection_layer")
            acc = False
            if M.patchnet == 'regular':
                # the patch transformer's backward: d(pooled windows) and the gradient w.r.t. the image tokens through both blocks' keys /
                # values -- [masked view | augmented view] rows, written where the pooling gradient is then ADDED
                from . import patchnet
                dpool, dfeat = patchnet.backward(self, dpool, "patch_extractor", self.saved_heads["patch_extractor"], 2 * B)
                self._grad_ready(dev, "patch_extractor")
                d_enc, acc = dfeat, True
            if M.patchnet == 'conv':
                # ConvPatchNet's backward hands the gradient w.r.t. the token maps of [masked view | augmented view] straight back
                from . import convpatchnet
                d_enc = convpatchnet.backward(self, dpool, "patch_extractor", self.saved_heads["patch_extractor"], 2 * B)
                self._grad_ready(dev, "patch_extractor")
                if M.has_pix_projector:
                    self.mlp_backward(d_enc[:B * N], "pix_projector", dx_out=d_enc[:B * N])
                    self._grad_ready(dev, "pix_projector")
            elif M.has_pix_projector:
                dmasked2 = d_enc[:B * N] if acc else torch.empty((B * N, D), device=dev, dtype=BF16)
                ops.window_pool_bwd(dpool[:n], dmasked2, B, M.gh, M.gw, nw, D, acc)
                ops.window_pool_bwd(dpool[n:], d_enc[B * N:], B, M.gh, M.gw, nw, D, acc)
                # (regular: the incoming gradient lives in d_enc's own first half; the stack's last data gradient overwrites it when it is done with it)
                self.mlp_backward(dmasked2, "pix_projector", dx_out=d_enc[:B * N])
                self._grad_ready(dev, "pix_projector")
            else:
                ops.window_pool_bwd(dpool[:n], d_enc[:B * N], B, M.gh, M.gw, nw, D, acc)
                ops.window_pool_bwd(dpool[n:], d_enc[B * N:], B, M.gh, M.gw, nw, D, acc)
        elif M.use_moco_target:
            for name in (("predictor", "encoder_projection_layer") + (("patch_extractor",) if M.patchnet != 'no_patchtrans' else ())
                         + (("pix_projector",) if M.has_pix_projector else ())):
                self.comm.grad_ready(M, name)
        # ---- SimMIM decoder path
        if g_vis is not None:
            gath, h0, h1, h2, mu, rs = self.saved_dec
            Mrows, Mp, C, Dd = self.Mrows, self.Mp, M.dec_classes, M.dec_dim
            dpred = torch.empty((Mp, 64), device=dev, dtype=BF16)
            ops.pad_cast_rows(g_vis.reshape(Mrows, C).contiguous().float(), dpred, Mrows, C)
            self._on_side(dev, lambda: (ops.wgrad(dpred, h2, g32["pix_decoder.4.weight"], C, Dd, Mp),
                                        ops.colsum(dpred, g32["pix_decoder.4.bias"], cols=C)), dpred, h2)
            dh2 = ops.gemm(dpred, w16["pix_decoder.4.weight"], Mp, Dd, 64, tb=True, b_rows=C)
            dh1 = ops.layernorm_bwd(dh2, h1, f32["pix_decoder.2.weight"], f32["pix_decoder.2.bias"], mu, rs, None,
                                    g32["pix_decoder.2.weight"], g32["pix_decoder.2.bias"], gelu=True)
            self._on_side(dev, lambda: ops.linear_wgrad(dh1, h0, g32["pix_decoder.1.weight"]), dh1, h0)
            dh0 = ops.linear_dgrad(dh1, w16["pix_decoder.1.weight"])
            self._on_side(dev, lambda: ops.linear_wgrad(dh0, gath, g32["pix_decoder.0.weight"]), dh0, gath)
            dgath = ops.linear_dgrad(dh0, w16["pix_decoder.0.weight"])
            ops.scatter_rows_add(dgath, self.idx, d_enc, Mrows)
        if M.use_pixel_target:
            self._grad_ready(dev, "pix_decoder")
        if M.has_final_norm:
            # Gen-only: the encoder's final LayerNorm between the blocks and the decoder (modeling_pretrain_vit.py:104)
            if g_vis is not None:
                enc_raw, mu, rs = self.saved_norm
                d_enc = ops.layernorm_bwd(d_enc, enc_raw, f32["encoder.norm.weight"], f32["encoder.norm.bias"], mu, rs, None,
                                          g32["encoder.norm.weight"], g32["encoder.norm.bias"])
            self._grad_ready(dev, "encoder.norm")
            self.saved_norm = None
        # ---- encoder
        ew_on, _ = _weights(M)
        _mark("backward: heads + decoder done", dev)
        if views == 2 or g_vis is not None:
            self.encoder_backward(ew_on, self.saved_enc, d_enc, self.images, self.aug, self.mask_u8, views=views)
        else:
            for i in reversed(range(M.depth)):
                self.comm.grad_ready(M, f"encoder.blocks.{i}")
            self.comm.grad_ready(M, "encoder.embed")
        main, side = self._streams(dev)
        if side is not main:
            main.wait_stream(side)                  # every gradient is final on the caller's stream (grad norm / AdamW follow)
        _mark("backward: encoder done, streams joined", dev)
        self._keep.clear()                          # (blocks go back to the caller's stream's pool: its later work is ordered behind the join)
        self._keep_marks.clear()
        self.saved_enc = self.saved_heads = self.saved_dec = self.saved_norm = self.wT = None


class _DigFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, images, aug, mask, m, mim_views):
        step = _Step(model)
        contra, accs, vis_out = step.forward(images, aug, mask, m, mim_views, training=True)
        ctx.step = step
        ctx.set_materialize_grads(False)          # an unused output arrives as None, not as a zero tensor (host-visible)
        ctx.mark_non_differentiable(accs)
        return contra, accs, vis_out

    @staticmethod
    def backward(ctx, g_contra, g_accs, g_vis):
        step, ctx.step = ctx.step, None
        step.backward(g_contra, g_vis)
        return None, None, None, None, None, None, None


# ---- the step as registered PyTorch operators ---------------------------------------------------------------------------------------------
# `dig::pretrain_step_fwd` / `dig::pretrain_step_bwd` (torch.library): what MoCo_ViT.forward dispatches and what its autograd formula calls.
# The operators take the online parameter arena and the gradient arena as tensor arguments, the model object (and with it the state its
# forward updates: momentum parameters, BatchNorm running statistics) through a registry key, and hand the activations from forward to backward
# through a step handle.  They are
# the same code the autograd.Function form runs (DIG_STEP_OPS=0) -- one dispatcher hop per direction (~40 us of host time per step).
# No fake (meta) implementation: the SimMIM output's row count is the number of masked tokens, a value read from the mask on the host.
STEP_OPS = os.environ.get("DIG_STEP_OPS", "1") != "0"
_MODELS = weakref.WeakValueDictionary()
_LIVE_STEPS = {}
_handles = itertools.count(1)


@torch.library.custom_op("dig::pretrain_step_fwd", mutates_args=(), device_types="cuda")
def pretrain_step_fwd(anchor: torch.Tensor, online: torch.Tensor, images: torch.Tensor, aug: torch.Tensor, mask: torch.Tensor, m: float,
                      m_dev: Optional[torch.Tensor], mim_views: int, model_key: int, handle: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(contra_loss, [q1_acc1, q1_acc5, q2_acc1, q2_acc5], vis_out) of MoCo_ViT.forward (modeling_pretrain_moco_mim_ori.py:484-592).
    handle != 0: a backward will follow; the step's saved activations wait under that handle.
    Like the reference's forward (`_momentum_update_key_encoder` :526, BatchNorm running statistics) it updates MODULE STATE -- the momentum
    arena and the running statistics of the model behind `model_key` -- which is not part of the operator's argument list (torch.library
    registers autograd formulas for operators without mutated ARGUMENTS only)."""
    step = _Step(_MODELS[model_key])
    contra, accs, vis_out = step.forward(images, aug, mask, m_dev if m_dev is not None else m, mim_views, training=handle != 0)
    if handle:
        _LIVE_STEPS[handle] = step
    return contra, accs, vis_out


@torch.library.custom_op("dig::pretrain_step_bwd", mutates_args=("grads",), device_types="cuda")
def pretrain_step_bwd(grads: torch.Tensor, g_contra: Optional[torch.Tensor], g_vis: Optional[torch.Tensor], handle: int) -> None:
    """Accumulates the gradients of every online parameter into `grads` (the flat arena the parameters' .grad are views of)."""
    _LIVE_STEPS.pop(handle).backward(g_contra, g_vis)


def _step_setup_context(ctx, inputs, output):
    ctx.handle, ctx.model_key = inputs[-1], inputs[-2]
    ctx.step = _LIVE_STEPS.pop(ctx.handle, None)  # the saved activations live and die with the autograd graph, not with the table
    ctx.set_materialize_grads(False)              # an unused output arrives as None, not as a zero tensor (host-visible)
    ctx.mark_non_differentiable(output[1])


def _step_backward(ctx, g_contra, g_accs, g_vis):
    step, ctx.step = ctx.step, None
    if step is None:
        raise RuntimeError("dig::pretrain_step_fwd: backward called twice (the step's activations are released by the first backward)")
    _LIVE_STEPS[ctx.handle] = step
    torch.ops.dig.pretrain_step_bwd(_MODELS[ctx.model_key].flat_grads, g_contra, g_vis, ctx.handle)
    return (None,) * 10


pretrain_step_fwd.register_autograd(_step_backward, setup_context=_step_setup_context)


def dig_forward(model, image, aug_image, vis_mask_pos, m, only_mim_on_ori_img=True):
    if not image.is_cuda:
        raise RuntimeError("dig_amd.MoCo_ViT runs on an MI355X (cuda device) only; there is no CPU fallback")
    if model._flat["online"].device != image.device:
        raise RuntimeError("model and inputs are on different devices (call model.to(device))")
    mim_views = 1 if only_mim_on_ori_img else 2
    mask = vis_mask_pos
    if mask.dim() == 2 and not (mask.dtype == torch.uint8 and tuple(mask.shape) == (2 * image.shape[0], model.N)):
        mask = mask.view(image.shape[0], -1, model.N)           # ([2 B, N] uint8 = the engine's prepared view-major rows: taken as they are)
    m = m if isinstance(m, torch.Tensor) else float(m)          # a device [m, 1-m] pair under graph capture (step_graph.py)
    anchor = getattr(model, "_anchor", None)
    if anchor is None or anchor.device != image.device:
        anchor = model._anchor = torch.zeros(1, device=image.device, requires_grad=True)
    if STEP_OPS:
        # The operator is EAGER-ONLY: it updates module state that is not in its argument list (momentum arena, BatchNorm statistics, the
        # bf16 weight shadows) and its third output's shape depends on the mask, so a tracing compiler must neither dedupe / reorder it nor
        # see it at all.
        if torch.compiler.is_compiling():
            raise RuntimeError("dig::pretrain_step_fwd is an eager-only operator (it updates the momentum encoder and the BatchNorm statistics "
                               "of the module): call the model outside torch.compile")
        key = id(model)
        _MODELS[key] = model
        handle = next(_handles) if torch.is_grad_enabled() else 0
        try:
            contra, accs, vis_out = torch.ops.dig.pretrain_step_fwd(
                anchor, model._flat["online"], image, aug_image, mask,
                0.0 if isinstance(m, torch.Tensor) else m, m if isinstance(m, torch.Tensor) else None, mim_views, key, handle)
        finally:
            _LIVE_STEPS.pop(handle, None)           # (normally taken over by the autograd context in _step_setup_context: never left behind)
    elif torch.is_grad_enabled():
        contra, accs, vis_out = _DigFn.apply(anchor, model, image, aug_image, mask, m, mim_views)
    else:
        contra, accs, vis_out = _Step(model).forward(image, aug_image, mask, m, mim_views)
    B = image.shape[0]
    out = {}
    if model.use_moco_target:               # (the reference fills these keys only `if self.use_moco_target`, modeling_pretrain_moco_mim_ori.py:512-558)
        out.update({"contra_loss": contra, "q1_acc1": accs[0:1], "q1_acc5": accs[1:2], "q2_acc1": accs[2:3], "q2_acc5": accs[3:4]})
    if model.use_pixel_target:              # (:560-577)
        out["vis_out"] = [vis_out] if mim_views == 1 else [vis_out[:B], vis_out[B:]]
    return out
