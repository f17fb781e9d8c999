"""Fine-tune TRAINING step of the recognition models on the MI355X -- SURVEY.md 8(f) row N1.  What every head shares is here once:
`EncoderTrain`, the class between `recognizer.RecEncoder` and the three models (gradient arena, drop rates, initialisation, freezing, the
`.train()` forward, the evaluation start of the heads without a decode graph), and `_EncoderStep` (arena lookups, the two streams, the encoder
both ways, the classifier's backward).  `RecModelTrain` = `EncoderTrain` + `RecModel` and `_DecoderStep` are the transformer decoder's; the GRU
attention head and the CTC head derive theirs in attn_recognizer.py / ctc_recognizer.py.

Mirrors (label smoothing 0, as in README.md:92-118), including the stochastic regularisers `--drop`, `--attn_drop_rate`,
`--drop_path` of the encoder and the recognition decoder's own dropout (0.1, hard-wired by models/decoder.py:13-18,141) -- masks
come from a keyed counter hash instead of torch's generator, see dig_amd/dropout.py:
  * `RecModel.forward` in train mode (models/model_builder.py:124-160) -> `TFDecoder.forward_train` (models/decoder.py:196-222):
    `model((images, targets, tgt_lens))` returns the logits [B, max_len, nb_classes] (+ three Nones, as the reference does);
  * `SeqCrossEntropyLoss` (loss/seqCrossEntropyLoss.py) with its gradient;
  * `create_optimizer(args, model, get_num_layer=..., get_layer_scale=...)` (optim_factory.py:33-100, layer-wise lr decay as in
    run_class_finetuning.py:471-520) as one fused AdamW launch over a flat parameter arena.
Parameters, gradients, Adam moments and the bf16 GEMM operands live in flat arenas (dig_amd/arena.py: each tensor padded to the granule) whose
layout keeps q|k|v (and k|v) projection weights adjacent, so the fused projections are views.  The whole model is ONE autograd
node with a hand-written backward on the hot-path kernels (encoder: the pre-training kernels; decoder: `dig_seq_attn_*_hd` at the decoder's head dim (24 / 48 / 64),
`dig_seq_embed_*`, `dig_gemm_bf16`, `dig_layernorm_*`).  The decoder's cross-attention over the encoder memory has three forms -- the encoder's
MFMA kernel on a few query rows, the sequence kernels, the folded text-conditional one -- and the step knows none of them: the model picked
one when it was built (`model.cross`, dig_amd/decoder_cross.py), and the layer loops below hand it norm2's output on the way up and the
gradient behind enc_attn.fc on the way down.  The CPU checker of this step lives with the tests."""
import ctypes
import math
import os
from collections import OrderedDict, namedtuple

import torch

from . import _lib as L
from . import arena
from . import dropout as DR
from . import encoder_blocks as EB
from . import ops
from .recognizer import RecEncoder, RecModel, SeqCrossEntropyLoss, SeqLabelSmoothingCrossEntropyLoss  # noqa: F401  (the criteria of this step)

BF16, F32 = torch.bfloat16, torch.float32
cf = ctypes.c_float
FT_FUSED_QV = os.environ.get("DIG_FT_FUSED_QV", "1") != "0"
# the encoder's MLP half as the pre-training step's fused launches: norm2 -> fc1 -> GELU -> fc2 -> Mlp.drop / drop_path -> + residual -> next norm1 in
# one forward launch (dig_mlp_chain_fwd_ln_dropout), both data gradients in one backward launch (dig_mlp_chain_bwd on the masked gradient)
FT_MLP_CHAIN = os.environ.get("DIG_FT_MLP_CHAIN", "1") != "0"
FT_BATCH_REDUCE = os.environ.get("DIG_FT_BATCH_REDUCE", "0") == "1"      # opt-in: fewer launches, ~0.3 ms slower per step
CLS_PAD = 128                     # classifier rows padded to a multiple of 64 (it is a non-transposed GEMM operand in backward)


def encoder_plan(M, rows):
    """The encoder walk of a fine-tune forward over `rows` token rows: with the chain, the LayerNorm behind a block (the next norm1 / the final
    norm) rides along."""
    return EB.Plan(chain_ln=FT_MLP_CHAIN and M.F <= 2048 and ops.mlp_chain_supported(M.D, M.F, rows))


def _rate(name, value):
    if not 0.0 <= float(value) < 1.0:
        raise ValueError(f"{name} must be in [0, 1), got {float(value)}")
    return float(value)


class EncoderTrain(RecEncoder):
    """The training layer of every recognition model: `RecEncoder` with a gradient arena beside its parameter arena, the encoder's stochastic
    regularisers, the reference's initialisation and the `.train()` forward, one autograd node around the head's step object (`_step_cls`)."""
    _step_cls = None                                    # the forward / backward of one step: every head sets its own
    _LAYER_NORMS = ()                                   # name prefixes of a head's LayerNorms that no "norm" in their module name tells
    _ARENAS = ("flat_params", "flat_grads")

    def __init__(self, args=None, *, drop_rate=None, attn_drop_rate=None, drop_path_rate=None, drop_seed=None, **kw):
        """Drop rates: from `args` (--drop / --attn_drop_rate / --drop_path, run_class_finetuning.py:69-74 -> create_model,
        :300-313) unless given.  drop_seed: base seed of the mask keys (default: torch.initial_seed())."""
        super().__init__(args, **kw)
        self.drop_rate = _rate("drop_rate", getattr(args, "drop", 0.0) if drop_rate is None else drop_rate)
        self.attn_drop_rate = _rate("attn_drop_rate", getattr(args, "attn_drop_rate", 0.0) if attn_drop_rate is None else attn_drop_rate)
        self.drop_path_rate = _rate("drop_path_rate", getattr(args, "drop_path", 0.0) if drop_path_rate is None else drop_path_rate)
        # stochastic depth decay rule (modeling_finetune.py:273)
        self.dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.drop_seed = torch.initial_seed() if drop_seed is None else int(drop_seed)
        self.drop_step = 0                              # training forwards so far: every step draws fresh keys
        self.frozen = set()                             # names with requires_grad = False (`fix_encoder_layers`)
        self.frozen_blocks = 0                          # encoder blocks 0 .. frozen_blocks-1 (and patch_embed) take no gradient
        self.init_weights()

    def init_weights(self):
        """The reference's initialisation, drawn from torch's CPU generator: encoder Linear weights xavier-uniform with zero
        biases and LayerNorm (1, 0) (`PretrainVisionTransformerEncoder._init_weights`, modeling_pretrain_vit.py:66-74); the
        patch-embed convolution and the heads keep PyTorch's defaults (nn.Conv2d / nn.Linear: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for
        weight and bias; what else a head holds: its own `_init_tensor`); mask_token, q_bias, v_bias zero.  Fine-tuning then overwrites
        the encoder from the pre-training checkpoint (`load_pretrained`)."""
        sd = OrderedDict((k, self._init_tensor(k, shp)) for k, shp in self.param_shapes().items())
        self.load_state_dict(sd)

    def _init_tensor(self, k, shp):
        enc = k.startswith("encoder.")
        if k.endswith("mask_token") or k.endswith("q_bias") or k.endswith("v_bias"):
            return torch.zeros(shp)
        if "norm" in k.split(".")[-2] and len(shp) == 1 or k.startswith(self._LAYER_NORMS):
            return torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
        if k.endswith(".weight"):                                              # xavier_uniform_ / kaiming_uniform_(a=sqrt(5))
            a = math.sqrt(6.0 / (shp[0] + shp[1])) if enc and len(shp) == 2 else 1.0 / math.sqrt(math.prod(shp[1:]))
            return (torch.rand(shp) * 2 - 1) * a
        if enc and "patch_embed" not in k:                                     # biases
            return torch.zeros(shp)
        return (torch.rand(shp) * 2 - 1) / math.sqrt(math.prod(self.param_shapes()[k[:-4] + "weight"][1:]))

    def load_pretrained(self, checkpoint, model_key="model|module", prefix=""):
        """run_class_finetuning.py:362-440 for the simmim_vit encoders: pick `checkpoint[model_key]`, strip a `backbone.` prefix,
        load what matches (`encoder.*` of the pre-training model IS this model's `encoder.*`), report the rest.  Returns
        (missing, unexpected) as the reference's `utils.load_state_dict` prints them."""
        from .utils import load_state_dict
        ck = None
        for key in model_key.split("|"):
            if key in checkpoint:
                ck = checkpoint[key]
                break
        if ck is None:
            ck = checkpoint
        new = OrderedDict((k[9:] if k.startswith("backbone.") else k, v) for k, v in ck.items())
        return load_state_dict(self, new, prefix=prefix)

    # ------------------------------------------------------------------ state
    def fix_encoder_layers(self, fixed_encoder_layers):
        """`--fixed_encoder_layers k` (run_class_finetuning.py:500-518): k >= 1 freezes `encoder.patch_embed`, k > 1 also the encoder
        blocks with index < k - 1 (k capped at depth + 1).  Call BEFORE `create_optimizer` (frozen parameters are not listed there, as
        `get_parameter_groups` skips `requires_grad = False`).  The backward stops above the last frozen block: nothing below it is
        computed.  Returns the frozen names (what the reference prints)."""
        k = int(fixed_encoder_layers)
        self.frozen, self.frozen_blocks = set(), 0
        if k >= 1:
            self.frozen |= {n for n in self._offsets if "encoder.patch_embed" in n}
        if k > 1:
            k = min(k, self.depth + 1)
            self.frozen_blocks = k - 1
            self.frozen |= {n for n in self._offsets if n.startswith("encoder.blocks.") and int(n.split(".")[2]) < k - 1}
        return [n for n in self._offsets if n in self.frozen]

    def named_parameters(self, *a, **k):
        for n in self._offsets:
            if n == "encoder.mask_token":
                continue
            p = self._view(self.flat_params, n)
            p.grad = self._view(self.flat_grads, n)
            yield n, p

    def parameters(self, *a, **k):
        for _, p in self.named_parameters():
            yield p

    def get_num_layers(self):
        return self.depth

    def no_weight_decay(self):
        return {"encoder.pos_embed", "encoder.cls_token"}

    def _own_arenas(self, flat_params):
        super()._own_arenas(flat_params)
        self.flat_grads = torch.zeros_like(flat_params)
        self._side = self.comm = None

    def _side_stream(self, dev):
        st = self._side
        if st is None or st.device != dev:
            st = self._side = torch.cuda.Stream(device=dev, priority=-1)   # (as the pre-training side stream)
        return st

    def _build_views(self):
        self._train_blocks = arena.enc_block_views(self._offsets, "encoder.", self.depth, self.D, self.flat_params, self._shadow, self.flat_grads)
        return super()._build_views()

    def enc_blocks(self):
        """The eval forward's per-block accessors plus "g": the same names in the gradient arena (kept out of `_w`: that holds weights only)."""
        self._views()
        return self._train_blocks

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        if not self.training:
            return super().forward(x)
        images = self._device_images(x)
        _, targets, lens = x
        if self._dev != images.device or self._shadow is None:
            self._bind(images.device)
        anchor = getattr(self, "_anchor", None)
        if anchor is None or anchor.device != images.device:
            anchor = self._anchor = torch.zeros(1, device=images.device, requires_grad=True)
        logits = _RecTrainFn.apply(anchor, self, images, targets.to(images.device), lens.to(images.device))
        return logits, None, None, None

    def eval_tokens(self, images):
        """What the evaluation of a head that has no decode graph starts with: a step object on freshly cast weights and the encoder's
        tokens from the training step's walk without dropout keys (and, like it, with the blocks' activations kept)."""
        if self._dev != images.device or self._shadow is None:
            self._bind(images.device)
        step = self._step_cls(self)
        self.refresh_shadow()
        return step, self.encoder_front(images, encoder_plan(self, images.shape[0] * self.N), True, frozen=self.frozen_blocks)[0]


class ModelEma:
    """timm.utils.ModelEma as run_class_finetuning.py:456-462 / engine_for_finetuning.py:136-139 use it (`--model_ema`): an exponential
    moving average of every state-dict tensor, `ema = decay * ema + (1 - decay) * model` after each optimizer step -- one `dig_ema_update`
    launch over the flat parameter arena.  `.ema` is a model object of the same class whose parameters are the averaged ones (for
    `evaluate(data_loader, model_ema.ema, ...)` and for the `model_ema` entry of checkpoints)."""

    def __init__(self, model, decay=0.9999, device='', resume=''):
        import copy
        if resume:
            raise NotImplementedError("ModelEma(resume=...) is not built: load the checkpoint's 'model_ema' into .ema.load_state_dict")
        self.decay = float(decay)
        self.ema = copy.copy(model)                                            # shares configuration, owns its arenas
        self.ema._own_arenas(model.flat_params.detach().clone())
        self.ema.train(False)

    def update(self, model):
        e = self.ema
        if e.flat_params.device != model.flat_params.device:
            e.flat_params = e.flat_params.to(model.flat_params.device)
        if e.flat_params.is_cuda:
            ops.ema_update(e.flat_params, model.flat_params, None, e.flat_params.numel(), self.decay)
        else:
            e.flat_params.mul_(self.decay).add_(model.flat_params, alpha=1.0 - self.decay)
        e.weights_changed()


class FlatGradComm:
    """Data parallelism for the fine-tune step: one all-reduce of the flat gradient arena after the backward (the hook
    `NativeScalerWithGradNormCount` calls), parameters broadcast from rank 0 at construction -- what DistributedDataParallel does
    for the reference (run_class_finetuning.py:522-526)."""

    def __init__(self, model, process_group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, process_group
        self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        dist.broadcast(model.flat_params, src=0, group=process_group)
        model.weights_changed()              # the arena was just overwritten behind torch's back
        # every rank draws its own dropout masks (the reference seeds each rank with args.seed + rank, run_class_finetuning.py:262-264)
        model.drop_seed = (int(model.drop_seed) + 0x9E3779B97F4A7C15 * self.rank) & ((1 << 64) - 1)

    def finish_grad_sync(self, model):
        # (the mean: the scaler seeds every backward with loss / world, see parallel.DistComm.finish_grad_sync)
        self.dist.all_reduce(model.flat_grads, group=self.group)


class _EncoderStep:
    """What one forward / backward of every recognition model shares: lookups by name in the three arenas, the two streams of the backward,
    the encoder both ways and the padded classifier's backward.  A head's step class adds `forward` and `backward`; all activations
    needed by the backward are kept on this object."""

    def __init__(self, model):
        self.m = model

    def p(self, name):
        return self.m._view(self.m.flat_params, name)

    def w(self, name):
        return self.m._view(self.m._shadow, name)

    def g(self, name):
        return self.m._view(self.m.flat_grads, name)

    def g_of(self, w):
        """The gradient-arena twin of a bound view `w` of the shadow (same element offsets): for the fused q|k|v and k|v projections."""
        return self.m.flat_grads[w.storage_offset():w.storage_offset() + w.numel()].view(w.shape)

    # ---------------------------------------------------------------- two streams (backward)
    def begin_backward(self, dev):
        """Two HIP streams, as in the pre-training backward (engine_core.encoder_backward): the data-gradient chain (dgrad GEMMs,
        attention / LayerNorm backward) stays on the caller's stream; weight-gradient GEMMs and bias column sums only consume
        (dy, saved activation) pairs and run on a second stream, joined before the optimizer."""
        M = self.m
        self._main = torch.cuda.current_stream(dev)
        self._side_st = M._side_stream(dev) if getattr(M, "overlap_streams", True) else self._main
        return self._main, self._side_st

    def side(self, fn, *tensors):
        if self._side_st is self._main:
            fn()
            return
        self._side_st.wait_stream(self._main)
        with torch.cuda.stream(self._side_st):
            fn()
        for t in tensors:
            t.record_stream(self._side_st)

    def encoder_forward(self, images):
        """RecEncoder.encoder_front under this step's dropout / drop-path keys; returns the normalised tokens [B*N, D] (bf16) and keeps what
        `encoder_backward` needs."""
        M = self.m
        M.refresh_shadow()
        N = M.N
        self.B = images.shape[0]
        # dropout / drop-path keys of this step (dig_amd/dropout.py); every spec is None when its rate is 0
        plan = self.plan = DR.DropPlan(M.drop_seed, M.drop_step)
        M.drop_step += 1
        pe, pa = M.drop_rate, M.attn_drop_rate
        self.ds_enc = [(plan.spec(DR.enc_site(i, 0), pa),                                            # (attention, proj branch, MLP branch)
                        plan.spec(DR.enc_site(i, 1), pe, DR.enc_site(i, 2), M.dpr[i], N),
                        plan.spec(DR.enc_site(i, 3), pe, DR.enc_site(i, 4), M.dpr[i], N)) for i in range(M.depth)]
        # x + drop_path(proj_drop(proj(.))) / x + drop_path(drop(fc2(.))) (modeling_finetune.py:120,59,156-158): GEMM epilogues.  No gradient flows
        # into a frozen block: nothing of it is kept
        eplan = encoder_plan(M, self.B * N)
        self.use_chain = eplan.chain_ln
        enc, (self.images, self.zmask, self.enc_saved, self.enc_last) = M.encoder_front(images, eplan, True, drops=self.ds_enc, frozen=M.frozen_blocks)
        return enc

    def encoder_backward(self, denc):
        """denc: bf16 [B*N, D] gradient w.r.t. the tokens `encoder_forward` returned (call `begin_backward` first)."""
        M = self.m
        dev = denc.device
        D, H, N = M.D, M.H, M.N
        x_last, emu, ers, enc = self.enc_last
        dx = ops.layernorm_bwd(denc, x_last, self.p("encoder.norm.weight"), self.p("encoder.norm.bias"), emu, ers, None, self.g("encoder.norm.weight"),
                               self.g("encoder.norm.bias"))
        # ---- encoder blocks (encoder_blocks.backward: one view, no masking; frozen blocks are a prefix: the chain stops above them).  The four
        # weight gradients of a block as ONE grouped launch on the second stream, every reduction handed over as it becomes ready
        blocks = M.enc_blocks()
        grouped = (ops.WGRAD_GROUP and not FT_BATCH_REDUCE and
                   all(ops.wgrad_group_route(o, i_, self.B * N) is not None for o, i_ in ((M.F, D), (D, M.F), (3 * D, D), (D, D))))
        wT = None
        if getattr(self, "use_chain", False) and M.frozen_blocks < M.depth:
            # K-contiguous copies of the MLP weights for the fused backward (one launch per weight shape, 1.2 MB per matrix)
            live = blocks[M.frozen_blocks:]
            wT = [None] * M.frozen_blocks + list(zip(ops.transpose_bf16_multi([b_["mlp.fc2.weight"] for b_ in live]),
                                                     ops.transpose_bf16_multi([b_["mlp.fc1.weight"] for b_ in live])))
        plan = EB.Plan(chain_bwd=wT is not None, fused_qv=FT_FUSED_QV, grouping="block" if grouped else "off", side_each=True,
                       batch_reduce=FT_BATCH_REDUCE)
        dx = EB.backward(plan, blocks, self.enc_saved, dx, wT, self.B, H, self.side, first=M.frozen_blocks, drops=self.ds_enc)
        if "encoder.patch_embed.proj.weight" in M.frozen:
            return
        gtok = torch.zeros(D, device=dev, dtype=F32)                          # mask_token takes no part at fine-tune: gradient discarded
        ops.patch_embed_bwd_mfma(dx, self.images, self.zmask, self.g("encoder.patch_embed.proj.weight").view(D, 48),
                                 self.g("encoder.patch_embed.proj.bias"), gtok, D, M.gh, M.gw)

    def classifier_backward(self, dl, o, weight, bias, out_kind=ops.OUT_BF16, classes=None):
        """The backward of the classifier zero-padded to CLS_PAD rows (self.cls_w): dl bf16 [rows, CLS_PAD], the gradient of its logits with
        zero pad columns; o [rows, d], its input; classes: its true rows (default nb_classes).  Weight and bias gradients on the second stream
        (the column sums through a padded vector); returns the gradient w.r.t. o, bf16 or (out_kind = ops.OUT_F32) fp32."""
        C, (rows, d) = classes or self.m.nb_classes, o.shape
        self.side(lambda: ops.wgrad(dl, o, self.g(weight), C, d, rows), dl, o)
        cs = torch.zeros(CLS_PAD, device=dl.device, dtype=F32)
        self.side(lambda: (ops.colsum(dl, cs, cols=CLS_PAD), self.g(bias).add_(cs[:C])), dl, cs)
        return ops.gemm(dl, self.cls_w, rows, d, CLS_PAD, tb=True, out_kind=out_kind)


# what a decoder layer's backward reads of its forward; cross: the saved state of the cross-attention form, opaque here
_LayerSaved = namedtuple("_LayerSaved", "x h1 m1 r1 qkv a lse1 x1 m2 r2 cross a2 x2 h3 m3 r3 pre u")


class _DecoderStep(_EncoderStep):
    """One forward / backward of `RecModelTrain`: linear_norm and the transformer decoder under teacher forcing."""

    def forward(self, images, targets, lens):
        M = self.m
        dev = images.device
        enc = self.encoder_forward(images)
        B = self.B
        mem, (self.mem_in, h, mmu, mrs) = M.linear_norm(enc)
        self.ln_saved = (h, mmu, mrs, mem)
        T, d, nh, dk = M.max_len, M.d, M.nh, M.dk
        hk = nh * dk
        plan = self.plan
        pd = M.decoder_dropout
        self.ds_tgt = plan.spec(DR.DEC_TGT, pd)
        self.ds_dec = [dict(sattn=plan.spec(DR.dec_site(i, 0), pd), sproj=plan.spec(DR.dec_site(i, 1), pd),
                            cattn=plan.spec(DR.dec_site(i, 2), pd), cproj=plan.spec(DR.dec_site(i, 3), pd),
                            act=plan.spec(DR.dec_site(i, 4), pd), out=plan.spec(DR.dec_site(i, 5), pd)) for i in range(M.n_layers)]
        # ---- decoder, teacher forcing (decoder.py:196-222)
        bos = torch.full((B, 1), M.start_idx, device=dev, dtype=torch.int64)
        query = torch.cat([bos, targets.long()], dim=-1)[:, :-1].contiguous()
        self.query, self.targets, self.lens = query, targets.long().contiguous(), lens.long().contiguous()
        x = torch.empty((B * T, d), device=dev, dtype=BF16)
        L.call("dig_seq_embed_fwd", L.ptr(query), L.ptr(self.p("decoder.trg_word_emb.weight")), L.ptr(M._w["pos"]), L.ptr(x), B, T, d,
               M.nb_classes + 1, L.stream())
        x = ops.dropout_apply(x, self.ds_tgt, out=x)                            # decoder.py:180
        sc = dk ** -0.5
        self.dec_saved = []
        self.mem = mem
        self.prepare_memory(dev)
        for i in range(M.n_layers):
            p = f"decoder.layer_stack.{i}."
            ds = self.ds_dec[i]
            h1, m1, r1 = ops.layernorm_fwd(x, self.p(p + "norm1.weight"), self.p(p + "norm1.bias"), 1e-5)
            qkv = ops.linear_fwd(h1, M._w[p]["qkv"])
            a, lse1 = ops.seq_attn_fwd(qkv, qkv[:, hk:], qkv[:, 2 * hk:], B, nh, T, T, dk, sc, True, self.lens, ds["sattn"])
            x1 = ops.linear_fwd(a, self.w(p + "self_attn.fc.weight"), resid=x, drop=ds["sproj"])
            h2, m2, r2 = ops.layernorm_fwd(x1, self.p(p + "norm2.weight"), self.p(p + "norm2.bias"), 1e-5)
            a2, cross = M.cross.forward(self, p, h2, ds["cattn"])
            x2 = ops.linear_fwd(a2, self.w(p + "enc_attn.fc.weight"), resid=x1, drop=ds["cproj"])
            h3, m3, r3 = ops.layernorm_fwd(x2, self.p(p + "norm3.weight"), self.p(p + "norm3.bias"), 1e-5)
            pre = torch.empty((B * T, M.d_inner), device=dev, dtype=BF16)
            u = ops.linear_fwd(h3, self.w(p + "mlp.w_1.weight"), bias=self.p(p + "mlp.w_1.bias"), act=1, pre=pre, drop=ds["act"])
            x3 = ops.linear_fwd(u, self.w(p + "mlp.w_2.weight"), bias=self.p(p + "mlp.w_2.bias"), resid=x2, drop=ds["out"])
            self.dec_saved.append(_LayerSaved(x, h1, m1, r1, qkv, a, lse1, x1, m2, r2, cross, a2, x2, h3, m3, r3, pre, u))
            x = x3
        o, fm, fr = ops.layernorm_fwd(x, self.p("decoder.layer_norm.weight"), self.p("decoder.layer_norm.bias"), 1e-6)
        self.fin_saved = (x, fm, fr, o)
        C = M.nb_classes
        self.cls_w, cb = M.padded_classifier("decoder.classifier.weight", "decoder.classifier.bias", CLS_PAD)
        logits = torch.empty((B * T, CLS_PAD), device=dev, dtype=F32)
        ops.gemm(o, self.cls_w, B * T, CLS_PAD, d, out=logits, out_kind=ops.OUT_F32, bias=cb)
        return logits[:, :C].reshape(B, T, C)

    @staticmethod
    def padded_rows(rows, cols, dev):
        """bf16 [rows, cols] with one zero row behind it: an operand whose 64-column head slices are read in 128-column tiles by the
        weight-gradient GEMM (the last head's tile runs 64 columns past the last row)."""
        buf = torch.empty((rows + 1, cols), device=dev, dtype=BF16)
        buf[rows:].zero_()
        return buf[:rows]

    def add_dmem(self, dm):
        if self._dmem is None:
            self._dmem = dm
        else:
            ops.add_bf16(self._dmem, dm, self._dmem)

    def prepare_memory(self, dev):
        """What the cross-attention form computes from the encoder memory alone depends on no decoder state: every layer's is issued on the
        second stream now and overlaps the (small, latency-bound) self-attention kernels of the decoder chain; one event per layer."""
        M, mem = self.m, self.mem
        self._prepared = {}
        if not M.cross.prepares_memory:
            return
        main = torch.cuda.current_stream(dev)
        sd = M._side_stream(dev) if getattr(M, "overlap_streams", True) else main
        sd.wait_stream(main)
        with torch.cuda.stream(sd):
            for i in range(M.n_layers):
                p = f"decoder.layer_stack.{i}."
                kept = M.cross.prepare(mem, M._w[p])
                ev = torch.cuda.Event()
                ev.record(sd)
                for t_ in kept:
                    t_.record_stream(main)
                self._prepared[p] = (kept, ev)
        mem.record_stream(sd)

    def prepared(self, p):
        """The tensors `prepare_memory` made for layer p, the current stream made to wait for them."""
        kept, ev = self._prepared[p]
        torch.cuda.current_stream(self.mem.device).wait_event(ev)
        return kept

    def backward(self, dlogits_btc):
        """dlogits_btc: fp32 [B, T, C] gradient w.r.t. the returned logits."""
        M = self.m
        dev = dlogits_btc.device
        main, sd = self.begin_backward(dev)
        side = self.side
        B, T, d, nh, dk, C, D = self.B, M.max_len, M.d, M.nh, M.dk, M.nb_classes, M.D
        hk = nh * dk
        rows = B * T
        dl = torch.zeros((rows, CLS_PAD), device=dev, dtype=BF16)
        dl[:, :C] = dlogits_btc.reshape(rows, C).to(BF16)
        x, fm, fr, o = self.fin_saved
        do = self.classifier_backward(dl, o, "decoder.classifier.weight", "decoder.classifier.bias")
        dx = ops.layernorm_bwd(do, x, self.p("decoder.layer_norm.weight"), self.p("decoder.layer_norm.bias"), fm, fr, None,
                               self.g("decoder.layer_norm.weight"), self.g("decoder.layer_norm.bias"))
        self._dmem = None
        sc = dk ** -0.5
        for i in reversed(range(M.n_layers)):
            p = f"decoder.layer_stack.{i}."
            s, self.dec_saved[i] = self.dec_saved[i], None
            ds = self.ds_dec[i]
            # feed-forward (every dropped branch: its gradient is the residual gradient under the same mask)
            dz = ops.dropout_apply(dx, ds["out"])
            side(lambda: ops.linear_wgrad(dz, s.u, self.g(p + "mlp.w_2.weight")), dz, s.u)
            side(lambda: ops.colsum(dz, self.g(p + "mlp.w_2.bias")), dz)
            du, bparts = ops.linear_dgrad(dz, self.w(p + "mlp.w_2.weight"), gelu_pre=s.pre, colsum=True, drop=ds["act"])
            side(lambda: ops.colsum_partials(bparts, self.g(p + "mlp.w_1.bias")), bparts)
            side(lambda: ops.linear_wgrad(du, s.h3, self.g(p + "mlp.w_1.weight")), du, s.h3)
            dh3 = ops.linear_dgrad(du, self.w(p + "mlp.w_1.weight"))
            dx2 = ops.layernorm_bwd(dh3, s.x2, self.p(p + "norm3.weight"), self.p(p + "norm3.bias"), s.m3, s.r3, dx, self.g(p + "norm3.weight"),
                                    self.g(p + "norm3.bias"))
            # cross-attention over the encoder memory
            dz = ops.dropout_apply(dx2, ds["cproj"])
            side(lambda: ops.linear_wgrad(dz, s.a2, self.g(p + "enc_attn.fc.weight")), dz, s.a2)
            dh2 = M.cross.backward(self, p, dz, s.cross)
            dx1 = ops.layernorm_bwd(dh2, s.x1, self.p(p + "norm2.weight"), self.p(p + "norm2.bias"), s.m2, s.r2, dx2, self.g(p + "norm2.weight"),
                                    self.g(p + "norm2.bias"))
            # masked self-attention
            dz = ops.dropout_apply(dx1, ds["sproj"])
            side(lambda: ops.linear_wgrad(dz, s.a, self.g(p + "self_attn.fc.weight")), dz, s.a)
            da = ops.linear_dgrad(dz, self.w(p + "self_attn.fc.weight"))
            qkv, dqkv = s.qkv, torch.empty_like(s.qkv)
            ops.seq_attn_bwd(qkv, qkv[:, hk:], qkv[:, 2 * hk:], da, s.lse1, dqkv, dqkv[:, hk:], dqkv[:, 2 * hk:], B, nh, T, T, dk, sc, True, self.lens,
                             ds["sattn"])
            side(lambda: ops.linear_wgrad(dqkv, s.h1, self.g_of(M._w[p]["qkv"])), dqkv, s.h1)
            dh1 = ops.linear_dgrad(dqkv, M._w[p]["qkv"])
            dx = ops.layernorm_bwd(dh1, s.x, self.p(p + "norm1.weight"), self.p(p + "norm1.bias"), s.m1, s.r1, dx1, self.g(p + "norm1.weight"),
                                   self.g(p + "norm1.bias"))
        dx = ops.dropout_apply(dx, self.ds_tgt, out=dx)
        L.call("dig_seq_embed_bwd_lens", L.ptr(self.query), L.ptr(dx), L.ptr(self.g("decoder.trg_word_emb.weight")), rows, d, C + 1, T,
               L.ptr(self.lens), L.stream())
        # ---- linear_norm
        h, mmu, mrs, _ = self.ln_saved
        enc = self.mem_in
        main.wait_stream(sd)                                                    # the memory gradient was summed on the second stream
        dmem, self._dmem = self._dmem, None
        dmem.record_stream(main)
        dh = ops.layernorm_bwd(dmem, h, self.p("linear_norm.1.weight"), self.p("linear_norm.1.bias"), mmu, mrs, None, self.g("linear_norm.1.weight"),
                               self.g("linear_norm.1.bias"))
        side(lambda: ops.linear_wgrad(dh, enc, self.g("linear_norm.0.weight")), dh, enc)
        side(lambda: ops.colsum(dh, self.g("linear_norm.0.bias")), dh)
        denc = ops.linear_dgrad(dh, self.w("linear_norm.0.weight"))
        if M.use_1d_attdec:                                                     # every token of a column gets 1/gh of the column's gradient
            dfull = torch.empty((B * M.N, D), device=dev, dtype=BF16)
            ops.window_pool_bwd(denc, dfull, B, M.gh, M.gw, M.gw, D, False)
            denc = dfull
        self.encoder_backward(denc)
        main.wait_stream(sd)


class RecModelTrain(EncoderTrain, RecModel):
    """The training form of `RecModel`.  `.train()` forward = teacher-forced logits with autograd; `.eval()` = greedy decode on the same
    weights.  `decoder_dropout` = 0.1 is what `create_decoder` builds (models/decoder.py:13-18: TFDecoder's default, not configurable in the
    reference)."""
    _step_cls, _LAYER_NORMS = _DecoderStep, ("linear_norm.1.",)

    def __init__(self, args=None, *, decoder_dropout=0.1, **kw):
        self.decoder_dropout = _rate("decoder_dropout", decoder_dropout)
        super().__init__(args, **kw)

    def _init_tensor(self, k, shp):
        """The decoder and `linear_norm` keep PyTorch's defaults (models/model_builder.py:78-89 adds nothing); nn.Embedding: N(0, 1)."""
        return torch.randn(shp) if k.endswith("trg_word_emb.weight") else super()._init_tensor(k, shp)


class _RecTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, images, targets, lens):
        step = model._step_cls(model)
        logits = step.forward(images, targets, lens)
        ctx.step = step
        return logits

    @staticmethod
    def backward(ctx, g):
        step, ctx.step = ctx.step, None
        step.backward(g.contiguous().float())
        return None, None, None, None, None


# -------------------------------------------------------------------------------------------------- optimizer
def get_num_layer_for_vit(var_name, num_max_layer):
    """optim_factory.py:33-45."""
    if var_name in ("cls_token", "mask_token", "pos_embed") or var_name.startswith("patch_embed"):
        return 0
    if var_name.startswith("rel_pos_bias"):
        return num_max_layer - 1
    if var_name.startswith("blocks"):
        return int(var_name.split('.')[1]) + 1
    return num_max_layer - 1


class LayerDecayValueAssigner:
    """optim_factory.py:48-57."""

    def __init__(self, values):
        self.values = values

    def get_scale(self, layer_id):
        return self.values[layer_id]

    def get_layer_id(self, var_name):
        return get_num_layer_for_vit(var_name, len(self.values))


class FineTuneAdamW:
    """custom_optim AdamW over `RecModelTrain`'s arena with the reference's parameter groups (get_parameter_groups,
    optim_factory.py:57-100): `param_groups` carries lr / weight_decay / lr_scale per group exactly as the reference's list does (the
    engine rewrites lr = schedule * lr_scale and weight_decay every step); the update itself is one launch."""

    def __init__(self, model, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, get_num_layer=None, get_layer_scale=None, skip_list=()):
        self.model = model
        groups = OrderedDict()
        self._name_group = {}
        # every registered parameter in registration order -- `encoder.mask_token` included: the reference's optimizer lists it
        # (requires_grad) although the fine-tune forward never gives it a gradient, so it holds an index but no state
        self._stateless = set()
        for name in model._offsets:
            if name in getattr(model, "frozen", ()):
                continue                                                    # requires_grad = False: not listed (optim_factory.py:66-67)
            p = model._view(model.flat_params, name)
            if name == "encoder.mask_token":
                self._stateless.add(name)
            if p.ndim == 1 or name.endswith(".bias") or name in skip_list:
                gname, wd = "no_decay", 0.0
            else:
                gname, wd = "decay", weight_decay
            if get_num_layer is not None:
                lid = get_num_layer(name.replace('encoder.', '') if name.startswith('encoder') else name)
                gname = "layer_%d_%s" % (lid, gname)
            else:
                lid = None
            if gname not in groups:
                groups[gname] = {"weight_decay": wd, "names": [], "params": [], "lr_scale": get_layer_scale(lid) if get_layer_scale is not None else 1.0,
                                 "lr": lr, "betas": betas, "eps": eps}
            groups[gname]["names"].append(name)
            groups[gname]["params"].append(p)
            self._name_group[name] = gname
        self.param_groups = list(groups.values())
        self._gnames = list(groups.keys())
        self._step = 0
        self.exp_avg = self.exp_avg_sq = None
        self._tab_dev = None

    def zero_grad(self, set_to_none=False):
        ops.fill_f32(self.model.flat_grads, 0.0) if self.model.flat_grads.is_cuda else self.model.flat_grads.zero_()

    def _tables(self):
        M = self.model
        dev = M.flat_params.device
        if self._tab_dev == dev:
            return
        idx = torch.full((M.n_flat // arena.ALIGN,), 255, dtype=torch.uint8)   # 255 = no gradient (mask_token, padding)
        for gi, g in enumerate(self.param_groups):
            for n in g["names"]:
                if n in self._stateless:
                    continue                                                    # no gradient: the update leaves it alone (index 255)
                s = M._offsets[n]
                idx[s.offset // arena.ALIGN:arena.round_up(s.offset + s.numel) // arena.ALIGN] = gi   # (a v_bias may start inside a granule)
        self._idx = idx.to(dev)
        pin = (lambda t: t.pin_memory()) if dev.type == "cuda" else (lambda t: t)
        self._host_ring = [pin(torch.empty(2, 256, dtype=F32)) for _ in range(8)]   # the host may run steps ahead
        self._dev_tab = torch.empty(2, 256, device=dev, dtype=F32)
        self.exp_avg = torch.zeros(M.n_flat, device=dev, dtype=F32)
        self.exp_avg_sq = torch.zeros(M.n_flat, device=dev, dtype=F32)
        self._tab_dev = dev

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0, finite_gate=None):
        self._tables()
        M = self.model
        ng = len(self.param_groups)
        assert ng < 255
        host = self._host_ring[self._step % len(self._host_ring)]
        for gi, g in enumerate(self.param_groups):                              # whatever the engine wrote into the groups this step
            host[0, gi] = float(g["lr"])
            host[1, gi] = float(g["weight_decay"])
        self._dev_tab.copy_(host, non_blocking=True)
        g0 = self.param_groups[0]
        self._step += 1
        L.call("dig_adamw_step_groups", L.ptr(M.flat_params), L.ptr(M.flat_grads), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), None,
               ctypes.c_longlong(M.n_flat), L.ptr(self._idx), L.ptr(self._dev_tab[0]), L.ptr(self._dev_tab[1]), cf(g0["betas"][0]),
               cf(g0["betas"][1]), cf(g0["eps"]), self._step, cf(grad_scale), L.ptr(finite_gate), L.stream())
        M.weights_changed()

    # ---- checkpoints: torch.optim's per-parameter layout (what utils.save_model / auto_load_model exchange, utils/utils.py:546-651)
    def _ordered_names(self):
        return arena.group_names(self.param_groups)

    def _moments(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}

    def state_dict(self):
        return arena.optimizer_state_dict(self._moments(), self.model._offsets, self.param_groups, self._step, self._stateless)

    def load_state_dict(self, sd):
        self._tables()
        self._step = arena.load_optimizer_state(self._moments(), self.model._offsets, self.param_groups, sd)
        for g, lg in zip(self.param_groups, sd["param_groups"]):
            for key in ("lr", "weight_decay", "lr_scale", "betas", "eps"):
                if key in lg:
                    g[key] = lg[key]


def create_optimizer(args, model, get_num_layer=None, get_layer_scale=None, filter_bias_and_bn=True, skip_list=None):
    """optim_factory.create_optimizer for `--opt adamw` on a RecModelTrain."""
    if args.opt.lower() != "adamw":
        raise NotImplementedError("only --opt adamw is built")
    skip = skip_list if skip_list is not None else (model.no_weight_decay() if hasattr(model, "no_weight_decay") else ())
    betas = tuple(args.opt_betas) if getattr(args, "opt_betas", None) else (0.9, 0.999)
    return FineTuneAdamW(model, args.lr, args.weight_decay, betas, getattr(args, "opt_eps", 1e-8) or 1e-8, get_num_layer, get_layer_scale, skip)
