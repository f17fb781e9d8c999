"""Recognition forward + greedy decode on the MI355X -- the eval path of the reference's fine-tune model
(`RecModel.forward` with `self.training == False`, models/model_builder.py:124-160; `TFDecoder.forward_test`,
models/decoder.py:224-252; encoder factory `simmim_vit_small_patch4_32x128`, modeling_pretrain_vit.py:123-128).

    model = RecModel(args)                      # args.model / decoder_name / nb_classes / max_len as in run_class_finetuning.py
    model.load_state_dict(checkpoint["model"])  # the reference's fine-tune state_dict (encoder.*, linear_norm.*, decoder.*)
    probs, _, _, attn_maps = model((images, None, None))     # probs [B, max_len, nb_classes], attn_maps [B, max_len, 256]

What differs from the reference: the decoder keeps a K/V cache (one token per step instead of re-running all 26 positions 25
times -- same result, position t only depends on tokens <= t) and the cross-attention keys/values of the encoder memory are
projected once per layer -- or whatever else the decoder's cross-attention form caches of it: the forms, their extra parameters and their parts
of training and evaluation live in dig_amd/decoder_cross.py, and the constructor picks one.  `RecEncoder` is the encoder with its arenas, the base
of every recognition model (the GRU attention and CTC heads derive from it through dig_amd/finetune.py, not from `RecModel`); its encoder front and
`RecModel`'s memory projection are written once here for evaluation and for the fine-tune training step, which passes its own plan and dropout
keys; the sequence losses at the end carry their gradient.  There is no CPU fallback."""
import ctypes
import types
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import arena
from . import decoder_cross
from . import encoder_blocks as EB
from . import ops

BF16, F32 = torch.bfloat16, torch.float32
cf = ctypes.c_float

ENCODERS = {"simmim_vit_tiny_patch4_32x128": (192, 3), "simmim_vit_small_patch4_32x128": (384, 6), "simmim_vit_base_patch4_32x128": (512, 8)}
DECODERS = {"tf_decoder": dict(n_layers=6, d_model=512, n_head=8, d_k=64, d_inner=256),
            "small_tf_decoder": dict(n_layers=2, d_model=384, n_head=6, d_k=64, d_inner=192),
            # the decoders "consistent to the encoder" (models/decoder.py:35-72): 8 heads of d_model / 8, d_inner = 4 * d_model
            "corres_tiny_tf_decoder": dict(n_layers=6, d_model=192, n_head=8, d_k=24, d_inner=768),
            "corres_small_tf_decoder": dict(n_layers=6, d_model=384, n_head=8, d_k=48, d_inner=1536),
            "corres_base_tf_decoder": dict(n_layers=6, d_model=512, n_head=8, d_k=64, d_inner=2048)}
HEAD_DIMS = (24, 48, 64)          # the decoder head dims the attention kernels are built for (csrc/seq_attn.hip, csrc/decode.hip)


def _sinusoid(n_position, d_hid):
    """PositionalEncoding._get_sinusoid_encoding_table (models/transformer_layer.py:409-423)."""
    den = torch.Tensor([1.0 / np.power(10000, 2 * (j // 2) / d_hid) for j in range(d_hid)]).view(1, -1)
    tab = torch.arange(n_position).unsqueeze(-1).float() * den
    tab[:, 0::2] = torch.sin(tab[:, 0::2])
    tab[:, 1::2] = torch.cos(tab[:, 1::2])
    return tab


class RecEncoder(torch.nn.Module):
    """The fine-tune encoder with its arenas, whatever reads its tokens: configuration, the placed parameter arena and its bf16 shadow, the
    state dict, the bound views and the encoder forward.  A recognition head derives from it and names the parameters behind the encoder
    (`head_shapes`, in state-dict order) and, if its forward reads bound views, those (`head_views`)."""
    gh, gw, N = 8, 32, 256
    beam_width = 0                                      # (the autoregressive --beam_width: RecModel's decoder alone has one)
    _ARENAS = ("flat_params",)

    def __init__(self, args=None, *, embed_dim=None, depth=12, num_heads=None, nb_classes=97, max_len=25):
        super().__init__()
        if args is not None:                                                # as in run_class_finetuning.py
            (embed_dim, num_heads), nb_classes, max_len = ENCODERS[args.model], args.nb_classes, args.max_len
        if embed_dim // num_heads != 64:
            raise NotImplementedError("encoder head dimension 64 only")
        self.D, self.H, self.depth, self.F = embed_dim, num_heads, depth, 4 * embed_dim
        self.nb_classes, self.max_len = nb_classes, max_len
        # ONE weight store: an fp32 arena laid out by arena.place (each tensor padded to the granule, q|k|v and k|v projection weights
        # adjacent, so the fused projections are views) and its bf16 shadow, the GEMM operands; everything the kernels read is a view of the two
        self._offsets = OrderedDict(self.param_shapes())
        self.n_flat = arena.place(self._offsets)
        self._loaded, self._dev, self._tables = False, None, {}
        self._own_arenas(torch.zeros(self.n_flat, dtype=F32))

    # ------------------------------------------------------------------ state
    def param_shapes(self):
        return OrderedDict([*arena.encoder_shapes("encoder.", self.D, self.F, self.depth, True).items(), *self.head_shapes().items()])

    def head_shapes(self):
        raise NotImplementedError("a recognition head names its parameters")

    def head_views(self, w, p, s):
        """Add to `w` what the head's forward reads; p / s: name -> view of the fp32 arena / of the bf16 shadow."""

    def _view(self, flat, k):
        return arena.view(flat, self._offsets[k])

    def load_state_dict(self, state_dict, strict=True):
        """Accepts the reference RecModel's state_dict: buffers (`decoder.position_enc.position_table`) and the aliases RecModel
        registers (`patch_embed.*` = `encoder.patch_embed.*`, model_builder.py:92-93) are ignored."""
        shapes = self._offsets
        missing = [k for k in shapes if k not in state_dict]
        if missing and strict:
            raise KeyError(f"missing keys in state_dict: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        extra = [k for k in state_dict if k not in shapes and not k.endswith("position_table") and not k.startswith("patch_embed.")]
        if extra and strict:
            raise KeyError(f"unexpected keys in state_dict: {extra[:5]}")
        for k, slot in shapes.items():
            if k in state_dict and tuple(state_dict[k].shape) != slot.shape:
                raise ValueError(f"{k}: shape {tuple(state_dict[k].shape)} != {slot.shape}")
        for k in shapes:
            if k in state_dict:
                self._view(self.flat_params, k).copy_(state_dict[k].detach())
        self._loaded = True
        self.weights_changed()

    def state_dict(self, *a, **k):
        return OrderedDict((n, self._view(self.flat_params, n).detach().to("cpu", copy=True)) for n in self._offsets)

    def to(self, device=None, *a, **k):
        if device is not None:
            for name in self._ARENAS:
                setattr(self, name, getattr(self, name).to(torch.device(device)))
        return self

    def _own_arenas(self, flat_params):
        """Make `flat_params` this object's weight store: no shadow, unbound views, an empty HIP-graph cache (a shallow copy of a model
        becomes a model of its own with this)."""
        self.flat_params, self._shadow = flat_params, None
        self._bound = self._w = self._fresh = None
        self._weights_version = 0
        self._graphs = {}

    def weights_changed(self):
        """Whoever writes the parameter arena through a kernel (FineTuneAdamW.step, ModelEma.update, a broadcast) calls this; the next eval
        forward then refreshes what is derived from it.  (torch in-place writes are seen through the arena's own version counter.)"""
        self._weights_version += 1

    def refresh_shadow(self):
        ops.cast_f32_to_bf16(self.flat_params, self._shadow)

    def padded_classifier(self, weight, bias, rows, out=None):
        """The classifier zero-padded to `rows` rows (bf16 weight from the shadow, fp32 bias), written into `out` = (weight, bias) if given."""
        w, b = self._view(self._shadow, weight), self._view(self.flat_params, bias)
        cw = torch.zeros((rows, w.shape[1]), device=w.device, dtype=BF16) if out is None else out[0]
        cb = torch.zeros(rows, device=w.device, dtype=F32) if out is None else out[1]
        cw[:w.shape[0]].copy_(w)
        cb[:w.shape[0]].copy_(b)
        return cw, cb

    def _table(self, key, make):
        """A constant table on the arenas' device, made once per device (own storage: it is no parameter)."""
        dev = self.flat_params.device
        if key not in self._tables or self._tables[key][0] != dev:
            self._tables[key] = (dev, make().to(dev).contiguous())
        return self._tables[key][1]

    def _build_views(self):
        """Everything the forward reads, as views of the fp32 arena (vectors, embeddings) and of the bf16 shadow (GEMM operands); own
        storage only for the position tables and what a head pads."""
        P, S, D = self.flat_params, self._shadow, self.D
        p, s = (lambda k: self._view(P, k)), (lambda k: self._view(S, k))
        w = {"enc_blocks": arena.enc_block_views(self._offsets, "encoder.", self.depth, D, P, S)}
        w["pe_w"], w["pe_b"] = p("encoder.patch_embed.proj.weight").view(D, 48), p("encoder.patch_embed.proj.bias")
        w["mask_token"] = p("encoder.mask_token").view(D)
        w["enc_pos"] = self._table("enc_pos", lambda: arena.encoder_pos_table(self.N, D))
        w["enc_nw"], w["enc_nb"] = p("encoder.norm.weight"), p("encoder.norm.bias")
        self.head_views(w, p, s)
        return w

    def _views(self):
        """self._w, rebuilt when an arena has been re-made (.to(), another device, a copy of the model with arenas of its own): the one
        place where addresses change, so the captured decode graphs go with it."""
        arenas = (self.flat_params, getattr(self, "flat_grads", None), self._shadow)
        if self._bound is None or any(a is not b for a, b in zip(self._bound, arenas)):
            self._bound, self._w = arenas, self._build_views()
            self._fresh, self._graphs = None, {}
        return self._w

    def _bind(self, dev):
        """Arenas and shadow on `dev`, views bound."""
        if self.flat_params.device != dev:
            self.to(dev)
        if self._shadow is None or self._shadow.device != dev:
            self._shadow = torch.empty(self.n_flat, device=dev, dtype=BF16)
        self._dev = dev
        return self._views()

    def _device_images(self, x):
        images = x[0] if isinstance(x, (tuple, list)) else x
        if not images.is_cuda:
            raise RuntimeError(f"dig_amd.{type(self).__name__} runs on an MI355X (cuda device) only; there is no CPU fallback")
        return images

    # ------------------------------------------------------------------ forward pieces
    def enc_blocks(self):
        return self._w["enc_blocks"]

    def encoder_front(self, images, plan, save, drops=None, frozen=0):
        """PretrainVisionTransformerEncoder.forward (modeling_pretrain_vit.py:89-112, mask=None) on the pre-training hot-path kernels: patch
        embedding -> the blocks under `plan` (encoder_blocks.Plan; drops / frozen: see encoder_blocks.forward) -> encoder.norm, which rides
        behind the last block where the plan's chain makes it.  Returns the normalised tokens, bf16 [B*256, D], and what the backward reads:
        (fp32 images, the all-zero token mask, the blocks' saved activations, (x behind the last block, mean, rstd, tokens))."""
        w = self._w
        B = images.shape[0]
        images = images.contiguous().float()
        zmask = torch.zeros((B, self.N), device=images.device, dtype=torch.uint8)
        x = ops.patch_embed_fwd(images, w["pe_w"], w["pe_b"], zmask, w["mask_token"], w["enc_pos"], self.D, self.gh, self.gw)
        x, saved, ln_next = EB.forward(plan, self.enc_blocks(), x, B, self.H, 1e-6, save, drops=drops, tail=(w["enc_nw"], w["enc_nb"]), frozen=frozen)
        enc, mu, rs = ln_next if ln_next is not None else ops.layernorm_fwd(x, w["enc_nw"], w["enc_nb"], 1e-6)
        return enc, (images, zmask, saved, (x, mu, rs, enc))

    def encoder_features(self, images):
        """PretrainVisionTransformerEncoder.forward_features(x, mask=None): bf16 [B*256, D] -- the plain form, nothing kept."""
        return self.encoder_front(images, EB.Plan(), False)[0]


class RecModel(RecEncoder):
    """The encoder followed by `linear_norm` and the transformer decoder: greedy decode and beam search on a K/V cache."""

    def __init__(self, args=None, *, n_layers=None, d_model=None, n_head=None, d_k=64, d_inner=None, n_position=200, use_1d_attdec=False,
                 text_cond_vis=False, **encoder):
        if args is not None:
            if args.decoder_name == "decoupled_tf_decoder":
                raise NotImplementedError("decoupled_tf_decoder is not built: DecoupledTransformerDecoderLayer.forward reads cls_query_attn_maps.size(), "
                                          "and RecModel.forward passes None for it with every encoder factory of the reference")
            dk = DECODERS[args.decoder_name]
            n_layers, d_model, n_head, d_k, d_inner = dk["n_layers"], dk["d_model"], dk["n_head"], dk["d_k"], dk["d_inner"]
            use_1d_attdec = bool(getattr(args, "use_1d_attdec", False))
            text_cond_vis = bool(getattr(args, "text_cond_vis", False))
            if getattr(args, "insert_sem", False):
                raise NotImplementedError("semantic insertion (--insert_sem) is not built: no encoder factory of the reference enables it")
        if d_k not in HEAD_DIMS:
            raise NotImplementedError(f"decoder head dimension {d_k}: the attention kernels are built for {HEAD_DIMS}")
        # --use_1d_attdec (run_class_finetuning.py:89, model_builder.py:145-148): the decoder attends over the gw column means of the
        # token grid instead of all gh*gw tokens
        self.use_1d_attdec = bool(use_1d_attdec)
        self.n_mem = self.gw if self.use_1d_attdec else self.N
        # --text_cond_vis (run_class_finetuning.py, models/decoder.py:13-73): the decoder's cross-attention is the text-conditional one.
        # Which form of the cross-attention runs (dig_amd/decoder_cross.py) is decided here and nowhere else
        self.text_cond_vis = bool(text_cond_vis)
        self.cross = decoder_cross.choose(self.text_cond_vis, self.n_mem, d_model, n_head, d_k)
        self.n_layers, self.d, self.nh, self.dk, self.d_inner, self.n_position = n_layers, d_model, n_head, d_k, d_inner, n_position
        super().__init__(args, **encoder)                                   # (lays the arena out: the decoder's shapes are known by now)
        self.start_idx = self.nb_classes                                    # decoder.py:149
        self.use_hip_graph = True
        self.beam_width = int(getattr(args, "beam_width", 0) or 0) if args is not None else 0      # model_builder.py:110
        self.eos = 94                                                       # TFDecoder.beam_search's default (decoder.py:254)

    def head_shapes(self):
        D, d, hk, o = self.D, self.d, self.nh * self.dk, OrderedDict()
        o["decoder.trg_word_emb.weight"] = (self.nb_classes + 1, d)
        for i in range(self.n_layers):
            p = f"decoder.layer_stack.{i}."
            for n in ("norm1", "norm2", "norm3"):
                o[p + n + ".weight"] = (d,); o[p + n + ".bias"] = (d,)
            for a in ("self_attn", "enc_attn"):
                for w in ("linear_q", "linear_k", "linear_v"):
                    o[p + a + "." + w + ".weight"] = (hk, hk)
                o[p + a + ".fc.weight"] = (d, hk)
            o.update(self.cross.extra_shapes(p + "enc_attn."))
            o[p + "mlp.w_1.weight"] = (self.d_inner, d); o[p + "mlp.w_1.bias"] = (self.d_inner,)
            o[p + "mlp.w_2.weight"] = (d, self.d_inner); o[p + "mlp.w_2.bias"] = (d,)
        o["decoder.layer_norm.weight"] = (d,); o["decoder.layer_norm.bias"] = (d,)
        o["decoder.classifier.weight"] = (self.nb_classes, d); o["decoder.classifier.bias"] = (self.nb_classes,)
        o["linear_norm.0.weight"] = (d, D); o["linear_norm.0.bias"] = (d,)
        o["linear_norm.1.weight"] = (d,); o["linear_norm.1.bias"] = (d,)
        return o

    def head_views(self, w, p, s):
        """linear_norm, the decoder layers (fused q|k|v and k|v projections as views) and, with storage of their own, the sinusoid position
        table and the classifier padded to a multiple of 8 rows."""
        S, dev = self._shadow, self.flat_params.device
        fused = lambda first, count: arena.fused(S, self._offsets, first, count)
        w["pos"] = self._table("pos", lambda: _sinusoid(self.n_position, self.d))
        w["ln_w"], w["ln_b"] = s("linear_norm.0.weight"), p("linear_norm.0.bias")
        w["ln_nw"], w["ln_nb"] = p("linear_norm.1.weight"), p("linear_norm.1.bias")
        w["emb"] = p("decoder.trg_word_emb.weight")
        for i in range(self.n_layers):
            l = f"decoder.layer_stack.{i}."
            w[l] = dict(n1w=p(l + "norm1.weight"), n1b=p(l + "norm1.bias"), n2w=p(l + "norm2.weight"), n2b=p(l + "norm2.bias"),
                        n3w=p(l + "norm3.weight"), n3b=p(l + "norm3.bias"), qkv=fused(l + "self_attn.linear_q.weight", 3),
                        fc=s(l + "self_attn.fc.weight"), q2=s(l + "enc_attn.linear_q.weight"),
                        kv2=fused(l + "enc_attn.linear_k.weight", 2), fc2=s(l + "enc_attn.fc.weight"),
                        w1=s(l + "mlp.w_1.weight"), b1=p(l + "mlp.w_1.bias"), w2=s(l + "mlp.w_2.weight"), b2=p(l + "mlp.w_2.bias"))
            w[l].update(self.cross.views(l + "enc_attn.", p, s))
        w["fnw"], w["fnb"] = p("decoder.layer_norm.weight"), p("decoder.layer_norm.bias")
        w["Cp"] = (self.nb_classes + 7) // 8 * 8
        w["cls_w"], w["cls_b"] = torch.zeros((w["Cp"], self.d), device=dev, dtype=BF16), torch.zeros(w["Cp"], device=dev, dtype=F32)

    # ------------------------------------------------------------------ forward pieces
    def _prepare(self, dev):
        """Ready for the eval forward on `dev`: views bound, and what is derived from the fp32 arena -- the bf16 shadow (one cast launch) and
        the padded classifier -- refreshed IN PLACE if the arena was written since.  No address changes, so a captured decode graph stays
        valid across weight updates: the refresh is ordered before the replay on the caller's stream."""
        w = self._bind(dev)
        ver = (self._weights_version, self.flat_params._version)
        if self._fresh != ver:
            self.refresh_shadow()
            self.padded_classifier("decoder.classifier.weight", "decoder.classifier.bias", w["Cp"], out=(w["cls_w"], w["cls_b"]))
            self._fresh = ver

    def linear_norm(self, enc):
        """linear_norm (model_builder.py:86-89): Linear + LayerNorm(eps 1e-5) on the feature map, or with use_1d_attdec on the column means of
        the gh x gw grid (model_builder.py:145-148: enc_x.view(B, gh, gw, C).mean(1), [B*gw, D]).  Returns the memory the decoder attends over
        and what the backward reads: (the Linear's input, its output, mean, rstd)."""
        w = self._w
        if self.use_1d_attdec:
            B = enc.shape[0] // self.N
            cols = torch.empty((B * self.gw, self.D), device=enc.device, dtype=enc.dtype)
            ops.window_pool_fwd(enc, cols, B, self.gh, self.gw, self.gw, self.D)
            enc = cols
        h = ops.linear_fwd(enc, w["ln_w"], bias=w["ln_b"])
        m, mu, rs = ops.layernorm_fwd(h, w["ln_nw"], w["ln_nb"], 1e-5)
        return m, (enc, h, mu, rs)

    def memory(self, enc):
        return self.linear_norm(enc)[0]

    def _decode_state(self, mem, n_mem, slots_per_mem=1):
        """Buffers of a K/V-cached decode over S = B * slots_per_mem sequences (greedy: 1 slot per sample; beam search: beam_width
        slots that share their sample's projected memory)."""
        w, d, nh, dk, T = self._w, self.d, self.nh, self.dk, self.max_len
        hk = nh * dk
        dev = mem.device
        S = (mem.shape[0] // n_mem) * slots_per_mem
        st = types.SimpleNamespace(S=S, n_mem=n_mem, spm=slots_per_mem)
        self.cross.decode_state(st, mem, [w[f"decoder.layer_stack.{i}."] for i in range(self.n_layers)])    # the memory as its form caches it
        st.cache = [torch.zeros((S, T, 3 * hk), device=dev, dtype=BF16) for _ in range(self.n_layers)]
        st.x = torch.empty((S, d), device=dev, dtype=BF16)
        st.a = torch.empty((S, hk), device=dev, dtype=BF16)
        st.logits = torch.empty((S, w["Cp"]), device=dev, dtype=F32)
        return st

    def _decode_step(self, st, t, tok):
        """Feed token `tok` [S] at position t through the decoder stack; leaves the classifier logits in st.logits [S, Cp] and the
        last layer's cross-attention weights where self.cross.attn_map finds them."""
        w, d, nh, dk, T, C = self._w, self.d, self.nh, self.dk, self.max_len, self.nb_classes
        hk = nh * dk
        S = st.S
        scale = dk ** -0.5
        s_ = L.stream()
        x = st.x
        L.call("dig_decode_embed", L.ptr(tok), L.ptr(w["emb"]), L.ptr(w["pos"][t]), L.ptr(x), S, d, C + 1, s_)
        for i in range(self.n_layers):
            p = w[f"decoder.layer_stack.{i}."]
            h, _, _ = ops.layernorm_fwd(x, p["n1w"], p["n1b"], 1e-5)
            row = st.cache[i][:, t]                                                # [S, 3hk] view, row stride T*3hk
            ops.gemm(h, p["qkv"], S, 3 * hk, d, out=row, ldc=T * 3 * hk)
            L.call("dig_decode_self_attn", L.ptr(st.cache[i]), L.ptr(st.a), S, T, nh, dk, t, cf(scale), s_)
            x = ops.linear_fwd(st.a, p["fc"], resid=x)
            h, _, _ = ops.layernorm_fwd(x, p["n2w"], p["n2b"], 1e-5)
            self.cross.decode_step(st, i, p, h, i == self.n_layers - 1)             # -> st.a
            x = ops.linear_fwd(st.a, p["fc2"], resid=x)
            h, _, _ = ops.layernorm_fwd(x, p["n3w"], p["n3b"], 1e-5)
            u = ops.linear_fwd(h, p["w1"], bias=p["b1"], act=1)
            x = ops.linear_fwd(u, p["w2"], bias=p["b2"], resid=x)
        o, _, _ = ops.layernorm_fwd(x, w["fnw"], w["fnb"], 1e-6)
        ops.gemm(o, w["cls_w"], S, w["Cp"], d, out=st.logits, out_kind=ops.OUT_F32, bias=w["cls_b"])

    def greedy_decode(self, mem, n_mem, force_tokens=None):
        """TFDecoder.forward_test with a K/V cache.  mem: bf16 [B*n_mem, d].  force_tokens ([B, max_len] int64, optional) feeds
        the given tokens instead of the arg-max (teacher forcing, for parity tests).  Returns (probs [B,T,C] fp32,
        attn_maps [B,T,n_mem] fp32, tokens [B,T] int64)."""
        w, T, C = self._w, self.max_len, self.nb_classes
        dev = mem.device
        st = self._decode_state(mem, n_mem)
        B = st.S
        tok = torch.full((B,), self.start_idx, device=dev, dtype=torch.int64)
        probs = torch.empty((B, T, C), device=dev, dtype=F32)
        maps = torch.empty((B, T, n_mem), device=dev, dtype=F32)
        toks = torch.empty((B, T), device=dev, dtype=torch.int64)
        step_probs = torch.empty((B, C), device=dev, dtype=F32)
        for t in range(T):
            self._decode_step(st, t, tok)
            L.call("dig_softmax_argmax", L.ptr(st.logits), w["Cp"], L.ptr(step_probs), L.ptr(tok), B, C, L.stream())
            probs[:, t] = step_probs
            maps[:, t] = self.cross.attn_map(st)
            toks[:, t] = tok
            if force_tokens is not None:
                tok = force_tokens[:, t].contiguous()
        return probs, maps, toks

    def beam_search(self, mem, n_mem, beam_width, eos=None, force_logits=None, return_logits=False, force_tokens=None):
        """TFDecoder.beam_search (models/decoder.py:254-370) on the K/V-cached decode kernels.  As in the reference the token history
        of beam slot k is what slot k emitted (decoder.py:307 never re-orders it by predecessor), so the per-slot K/V cache is
        exactly the reference's recomputation; only scores and back-pointers are re-ranked (`dig_beam_step`, one launch per step),
        and the final back-tracking runs on the host over the [T, B*beam_width] decisions (one device -> host copy).
        Returns token ids [B, max_len] int64 (the best hypothesis per sample, decoder.py:369).  force_logits ([T, S, C] fp32,
        optional): use these classifier outputs instead of the decoder's (parity tests of the bookkeeping); return_logits: also
        return the decoder's classifier outputs [T, S, C] of every step; force_tokens ([T, S] int64, optional): feed these symbols back to the decoder instead
        of the ranked ones (step-by-step parity of the classifier outputs)."""
        w, T, C = self._w, self.max_len, self.nb_classes
        eos = self.eos if eos is None else eos
        dev = mem.device
        bw = int(beam_width)
        st = self._decode_state(mem, n_mem, slots_per_mem=bw)
        S = st.S
        B = S // bw
        tok = torch.full((S,), self.start_idx, device=dev, dtype=torch.int64)
        seq_scores = torch.full((S,), float("-inf"), device=dev, dtype=F32)
        seq_scores[::bw] = 0.0                                              # only slot 0 of a sample is live at step 0 (:272-274)
        syms = torch.empty((T, S), device=dev, dtype=torch.int64)
        preds = torch.empty((T, S), device=dev, dtype=torch.int64)
        scores = torch.empty((T, S), device=dev, dtype=F32)
        kept = []
        for t in range(T):
            if force_logits is None:
                self._decode_step(st, t, tok)
                lg, ld = st.logits, w["Cp"]
                if return_logits:
                    kept.append(st.logits[:, :C].clone())
            else:
                lg, ld = force_logits[t].contiguous(), force_logits.shape[-1]
            L.call("dig_beam_step", L.ptr(lg), ld, L.ptr(seq_scores), B, bw, C, eos, L.ptr(syms[t]), L.ptr(preds[t]), L.ptr(scores[t]), L.stream())
            tok = syms[t] if force_tokens is None else force_tokens[t].contiguous()
        ids = beam_backtrack(scores.cpu().numpy(), preds.cpu().numpy(), syms.cpu().numpy(), B, bw, eos).to(dev)
        return (ids, torch.stack(kept)) if return_logits else ids

    def forward(self, x):
        if self.training:
            raise NotImplementedError("the fine-tune training step (SURVEY.md 8f row N1) is not built; call .eval()")
        images = self._device_images(x)
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        self._prepare(images.device)
        with torch.no_grad():
            if self.beam_width > 0:
                # RecModel.forward -> TFDecoder.forward(..., beam_width) (model_builder.py:151-158, decoder.py:101-102): token ids
                # [B, max_len] and an all-ones tensor in place of (probabilities, attention maps)
                ids = self.beam_search(self.memory(self.encoder_features(images)), self.n_mem, self.beam_width)
                return ids, None, None, torch.ones_like(ids)
            if not self.use_hip_graph:
                probs, maps, _ = self._recognize(images)
                return probs, None, None, maps
            # The decode loop is ~2 200 launches of microsecond kernels per batch: launch-bound.  It is captured once per batch
            # shape into a HIP graph (inputs / outputs live in static buffers) and replayed.
            key = (tuple(images.shape), images.device)
            ent = self._graphs.get(key)
            if ent is None:
                static_in = images.detach().clone().float().contiguous()
                side = torch.cuda.Stream(device=images.device)
                side.wait_stream(torch.cuda.current_stream(images.device))
                with torch.cuda.stream(side):
                    self._recognize(static_in)                               # warm-up outside capture (lazy init, attributes)
                torch.cuda.current_stream(images.device).wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    probs, maps, toks = self._recognize(static_in)
                ent = self._graphs[key] = (graph, static_in, probs, maps, toks)
            graph, static_in, probs, maps, toks = ent
            static_in.copy_(images)
            graph.replay()
            return probs.clone(), None, None, maps.clone()

    def _recognize(self, images):
        enc = self.encoder_features(images)
        mem = self.memory(enc)
        return self.greedy_decode(mem, self.n_mem)


def beam_backtrack(scores, preds, syms, B, bw, eos):
    """The back-tracking that ends TFDecoder.beam_search (models/decoder.py:311-369): numpy [T, B*bw] decisions -> int64 [B, T].
    Walk the back-pointers from the best final beams; a hypothesis that emitted EOS at step t takes over a slot of its sample from
    the back (worst live beam first) with the score it had when it ended; finally re-sort by score and keep beam 0."""
    import numpy as np
    T = syms.shape[0]
    base = (np.arange(B) * bw)[:, None]
    last = scores[-1].reshape(B, bw)
    order = np.argsort(-last, axis=1, kind="stable")
    s = np.take_along_axis(last, order, 1).copy()
    t_pred = (order + base).reshape(-1)
    found = [0] * B
    rows = []
    for t in range(T - 1, -1, -1):
        cur = syms[t][t_pred].copy()
        t_pred = preds[t][t_pred].copy()
        ended = np.nonzero(syms[t] == eos)[0]
        for idx in ended[::-1]:
            b = int(idx) // bw
            k = bw - (found[b] % bw) - 1
            found[b] += 1
            t_pred[b * bw + k] = preds[t][idx]
            cur[b * bw + k] = syms[t][idx]
            s[b, k] = scores[t][idx]
        rows.append(cur)
    best = np.argsort(-s, axis=1, kind="stable")[:, 0] + base[:, 0]
    out = np.stack([r[best] for r in reversed(rows)], axis=1)
    return torch.from_numpy(out.astype(np.int64))


def class_canon(voc):
    """canonical code per class for `Accuracy` (evaluation_metric/metrics.py:14-16,19-62): digits / letters -> 1 + index in
    '0-9a-z' (case-folded); everything else (punctuation, EOS, PADDING, UNKNOWN) -> 0 = dropped."""
    import string
    keep = string.digits + string.ascii_lowercase
    return torch.tensor([1 + keep.index(c.lower()) if (len(c) == 1 and c.lower() in keep) else 0 for c in voc], dtype=torch.uint8)


def accuracy(pred_tokens, target_tokens, voc):
    """`Accuracy(output, target, dataset)` of the reference on device tensors [B, T] of class ids; returns a 0-dim tensor."""
    B, T = pred_tokens.shape
    dev = pred_tokens.device
    canon = class_canon(voc).to(dev)
    match = torch.empty(B, device=dev, dtype=torch.uint8)
    pred, targ = pred_tokens.contiguous(), target_tokens.to(dev).contiguous()
    L.call("dig_string_match", L.ptr(pred), L.ptr(targ), L.ptr(canon), len(voc), voc.index("EOS"), B, T, L.ptr(match), L.stream())
    return match.float().mean()


def recognition_f_measure(pred_tokens, target_tokens, voc):
    """`recognition_f_measure` (evaluation_metric/metrics.py:83-100) on device tensors; returns a 0-dim float64 tensor."""
    B, T = pred_tokens.shape
    dev = pred_tokens.device
    f = torch.empty(B, device=dev, dtype=torch.float64)
    pred, targ, canon = pred_tokens.contiguous(), target_tokens.to(dev).contiguous(), class_canon(voc).to(dev)   # (named: alive across the call)
    L.call("dig_char_fmeasure", L.ptr(pred), L.ptr(targ), L.ptr(canon), len(voc), voc.index("EOS"), B, T, L.ptr(f), L.stream())
    return f.mean()


class _SeqCEFn(torch.autograd.Function):
    """The sequence cross-entropy launch and its gradient; smoothing None: dig_seq_cross_entropy, else dig_seq_ls_cross_entropy (one more scalar)."""

    @staticmethod
    def forward(ctx, logits, target, length, smoothing):
        B, T, C = logits.shape
        x = logits.detach().float().contiguous()
        name, extra = ("dig_seq_cross_entropy", ()) if smoothing is None else ("dig_seq_ls_cross_entropy", (cf(smoothing),))
        rows = torch.empty((1 + len(extra)) * B * T, device=x.device, dtype=F32)
        loss = torch.empty(1, device=x.device, dtype=F32)
        L.call(name, L.ptr(x), L.ptr(target), L.ptr(length), B, T, C, *extra, L.ptr(rows), L.ptr(loss), L.stream())
        ctx.save_for_backward(x, target, length)
        ctx.entry = (name + "_bwd", extra)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, target, length = ctx.saved_tensors
        B, T, C = x.shape
        Cp = (C + 7) // 8 * 8
        dl = torch.empty((B * T, Cp), device=x.device, dtype=BF16)
        gs = g.reshape(1).float().contiguous()                         # (named: a converted copy must outlive the call)
        name, extra = ctx.entry
        L.call(name, L.ptr(x), C, L.ptr(target), L.ptr(length), L.ptr(gs), B, T, C, *extra, L.ptr(dl), Cp, L.stream())
        return dl[:, :C].float().reshape(B, T, C), None, None, None


class SeqCrossEntropyLoss(torch.nn.Module):
    """loss/seqCrossEntropyLoss.py (sample_normalize) with its gradient: forward(input [B,T,C] fp32, target [B,T], length [B]) -> 0-dim loss."""
    smoothing = None

    def forward(self, input, target, length):
        return _SeqCEFn.apply(input, target.to(input.device).long().contiguous(), length.to(input.device).long().contiguous(), self.smoothing)


class SeqLabelSmoothingCrossEntropyLoss(SeqCrossEntropyLoss):
    """loss/seqLabelSmoothingCrossEntropyLoss.py (sample_normalize), the criterion `--smoothing > 0` selects
    (run_class_finetuning.py:538-541), with the value the reference really computes: its smoothing term broadcasts to a [BT, BT]
    matrix (include/dig_hip.h `dig_seq_ls_cross_entropy`), which this class reproduces."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        if not 0.0 <= smoothing <= 1.0:
            raise ValueError("smoothing must be in [0, 1]")
        self.smoothing = float(smoothing)
