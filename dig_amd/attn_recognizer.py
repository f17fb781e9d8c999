"""`AttnRecModel` on the MI355X -- SURVEY.md 8(f) row N1, the second decoder (`--decoder_type attention`,
run_class_finetuning.py:352-353): the fine-tune encoder followed by the GRU attention recognition head.

Mirrors models/model_builder.py:40-72 (`AttnRecModel`: encoder tokens [B, 256, D] straight into the head, no `linear_norm`) and
models/attn_decoder.py:11-78,197-272 (`AttentionRecognitionHead.forward_train` -- max(lengths) teacher-forced steps, outputs
zero-padded to max_len -- and the greedy `sample`; `DecoderUnit` = additive attention + target embedding + one nn.GRU cell + classifier).
Same state-dict keys as the reference (`decoder.decoder.attention_unit.{sEmbed,xEmbed,wEmbed}.*`, `decoder.decoder.tgt_embedding.weight`,
`decoder.decoder.gru.{weight,bias}_{ih,hh}_l0`, `decoder.decoder.fc.*`).  Flat arenas, one autograd node, the encoder on the
pre-training hot-path kernels (model and step on dig_amd.finetune.EncoderTrain / _EncoderStep); the head's steps run on `dig_gemm_bf16` + `dig_addattn_*` +
`dig_gru_cell_*` (csrc/gru_attn.hip), weight gradients as ONE GEMM per weight over the stacked steps.  Evaluation decodes greedily (`sample`)
or, with `--beam_width K` (1..8), by the head's `beam_search` (attn_decoder.py:84-200, which the reference carries and never reaches): the K
hypotheses of a sample share one copy of its tokens (`dig_addattn_fwd_slots`) and `dig_attn_beam_advance` closes every step."""
import math
import types

import torch

from . import _lib as L
from . import ops
from .finetune import EncoderTrain, _EncoderStep, CLS_PAD

BF16, F32 = torch.bfloat16, torch.float32
PRE = "decoder.decoder."
MAX_BEAM_WIDTH = 8                                      # dig_addattn_fwd_slots / dig_attn_beam_advance: the slots of a sample in one workgroup


class _AttnTrainStep(_EncoderStep):
    """Forward / backward of one AttnRecModel step (teacher forcing)."""

    def _w(self):
        M = self.m
        return M.attDim, M.sDim, M.D, M.attDim, M.nb_classes                 # A, S, X, E, C

    def head_inputs(self, x):
        """What every step of the head reads: the encoder tokens x [B*N, X], xEmbed(x) [B*N, A], the wEmbed vector [A], and the sEmbed / GRU
        weights, looked up once."""
        p, w = self.p, self.w
        xproj = ops.linear_fwd(x, w(PRE + "attention_unit.xEmbed.weight"), bias=p(PRE + "attention_unit.xEmbed.bias"))
        wv = p(PRE + "attention_unit.wEmbed.weight").reshape(self.m.attDim).contiguous()
        return types.SimpleNamespace(x=x, xproj=xproj, wv=wv, ws=w(PRE + "attention_unit.sEmbed.weight"), bs=p(PRE + "attention_unit.sEmbed.bias"),
                                     wih=w(PRE + "gru.weight_ih_l0"), bih=p(PRE + "gru.bias_ih_l0"),
                                     whh=w(PRE + "gru.weight_hh_l0"), bhh=p(PRE + "gru.bias_hh_l0"))

    def gru_attention_step(self, hd, sbf, s_prev, inp, sproj, alpha, s_new, sbf_new, gates, slots=0):
        """One DecoderUnit step (attn_decoder.py:236-272) from the state sbf (bf16; s_prev: the same in fp32, None = zeros): sEmbed(state) ->
        additive attention over the tokens, whose context lands in inp[:, E:] behind the target embedding the caller put into inp[:, :E] ->
        the two gate GEMMs -> the GRU cell.  Writes sproj, alpha, gates and the new state (s_new fp32, sbf_new bf16).  slots = K > 0 (beam
        search): the rows are the K hypotheses of every sample over that sample's one copy of the tokens, and alpha may be None."""
        A, S, X, E, _ = self._w()
        B, N = sbf.shape[0], self.m.N
        ops.linear_fwd(sbf, hd.ws, bias=hd.bs, out=sproj)
        if slots:
            L.call("dig_addattn_fwd_slots", L.ptr(hd.xproj), L.ptr(sproj), L.ptr(hd.wv), L.ptr(hd.x), L.ptr(alpha), L.ptr(inp[:, E:]), E + X, B // slots, N, A,
                   X, slots, L.stream())
        else:
            L.call("dig_addattn_fwd", L.ptr(hd.xproj), L.ptr(sproj), L.ptr(hd.wv), L.ptr(hd.x), L.ptr(alpha), L.ptr(inp[:, E:]), E + X, B, N, A, X, L.stream())
        gi = ops.linear_fwd(inp, hd.wih, bias=hd.bih)
        gh = ops.linear_fwd(sbf, hd.whh, bias=hd.bhh)
        L.call("dig_gru_cell_fwd", L.ptr(gi), L.ptr(gh), L.ptr(s_prev), L.ptr(s_new), L.ptr(sbf_new), L.ptr(gates), B, S, L.stream())

    def forward(self, images, targets, lens):
        M = self.m
        dev = images.device
        x = self.encoder_forward(images)                                      # [B*N, X] bf16
        B, N = self.B, M.N
        A, S, X, E, C = self._w()
        hint = getattr(M, "_steps_hint", None)                                # max(lengths) read from the host copy of tgt_lens (no device sync)
        steps = hint if hint is not None else (int(lens.max().item()) if lens.numel() else 0)
        steps = max(0, min(steps, M.max_len))
        self.steps, self.x = steps, x
        self.targets, self.lens = targets.long().contiguous(), lens.long().contiguous()
        logits = torch.zeros((B, M.max_len, C), device=dev, dtype=F32)
        if steps == 0:
            return logits
        hd = self.head_inputs(x)
        # teacher forcing: every step's previous token is known up front (attn_decoder.py:46-50): <BOS> = num_classes, then targets[:, i-1]
        yprev = torch.cat([torch.full((B, 1), C, device=dev, dtype=torch.int64), self.targets[:, :steps - 1]], 1).t().contiguous()   # [steps, B]
        inp = torch.empty((steps, B, E + X), device=dev, dtype=BF16)          # GRU inputs [yProj | context] of every step
        L.call("dig_embed_rows", L.ptr(yprev), L.ptr(self.p(PRE + "tgt_embedding.weight")), L.ptr(inp), E + X, steps * B, E, C + 1, L.stream())
        s_all = torch.empty((steps, B, S), device=dev, dtype=F32)
        sbf_all = torch.empty((steps + 1, B, S), device=dev, dtype=BF16)      # sbf_all[t] = state BEFORE step t (row 0 = zeros)
        sbf_all[0].zero_()
        sproj_all = torch.empty((steps, B, A), device=dev, dtype=BF16)
        alpha_all = torch.empty((steps, B, N), device=dev, dtype=F32)
        gates_all = torch.empty((steps, B, 4 * S), device=dev, dtype=F32)
        for t in range(steps):
            self.gru_attention_step(hd, sbf_all[t], s_all[t - 1] if t else None, inp[t], sproj_all[t], alpha_all[t], s_all[t], sbf_all[t + 1], gates_all[t])
        # classifier for all steps at once (rows (t, b))
        self.cls_w, cb = M.padded_classifier(PRE + "fc.weight", PRE + "fc.bias", CLS_PAD)
        out = torch.empty((steps * B, CLS_PAD), device=dev, dtype=F32)
        ops.gemm(sbf_all[1:].reshape(steps * B, S), self.cls_w, steps * B, CLS_PAD, S, out=out, out_kind=ops.OUT_F32, bias=cb)
        logits[:, :steps] = out.view(steps, B, CLS_PAD)[:, :, :C].transpose(0, 1)
        self.saved = (hd.xproj, hd.wv, yprev, inp, s_all, sbf_all, sproj_all, alpha_all, gates_all)
        return logits

    def backward(self, dlogits_btc):
        M = self.m
        dev = dlogits_btc.device
        main, sd = self.begin_backward(dev)
        side = self.side
        B, N, steps = self.B, M.N, self.steps
        A, S, X, E, C = self._w()
        x = self.x
        if steps == 0:
            self.encoder_backward(torch.zeros_like(x))
            main.wait_stream(sd)
            return
        xproj, wv, yprev, inp, s_all, sbf_all, sproj_all, alpha_all, gates_all = self.saved
        p, w, g = self.p, self.w, self.g
        rows = steps * B
        # classifier (all steps): dout rows (t, b)
        dl = torch.zeros((rows, CLS_PAD), device=dev, dtype=BF16)
        dl.view(steps, B, CLS_PAD)[:, :, :C] = dlogits_btc[:, :steps].transpose(0, 1).to(BF16)
        # classifier path into every step's new state
        ds_fc = self.classifier_backward(dl, sbf_all[1:].reshape(rows, S), PRE + "fc.weight", PRE + "fc.bias", out_kind=ops.OUT_F32)
        ds_fc = ds_fc.view(steps, B, S)
        wih, whh, ws_ = w(PRE + "gru.weight_ih_l0"), w(PRE + "gru.weight_hh_l0"), w(PRE + "attention_unit.sEmbed.weight")
        dgi_all = torch.empty((steps, B, 3 * S), device=dev, dtype=BF16)
        dgh_all = torch.empty((steps, B, 3 * S), device=dev, dtype=BF16)
        dinp_all = torch.empty((steps, B, E + X), device=dev, dtype=BF16)
        dsproj_all = torch.empty((steps, B, A), device=dev, dtype=BF16)
        dv_all = torch.empty((steps, B, N), device=dev, dtype=F32)
        dw_acc = torch.zeros((B, A), device=dev, dtype=F32)
        dz = torch.empty((B, S), device=dev, dtype=F32)                       # z * ds of the later step
        d1 = torch.empty((B, S), device=dev, dtype=F32)                       # dgh @ W_hh of the later step
        d2 = torch.empty((B, S), device=dev, dtype=F32)                       # dsproj @ W_s of the later step
        for t in reversed(range(steps)):
            last = t == steps - 1
            L.call("dig_gru_cell_bwd", L.ptr(ds_fc[t]), None if last else L.ptr(dz), None if last else L.ptr(d1), None if last else L.ptr(d2),
                   L.ptr(gates_all[t]), L.ptr(s_all[t - 1]) if t else None, L.ptr(dgi_all[t]), L.ptr(dgh_all[t]), L.ptr(dz), B, S, L.stream())
            ops.gemm(dgi_all[t], wih, B, E + X, 3 * S, tb=True, out=dinp_all[t])            # d[yProj | context]
            L.call("dig_addattn_bwd", L.ptr(xproj), L.ptr(sproj_all[t]), L.ptr(wv), L.ptr(x), L.ptr(alpha_all[t]), L.ptr(dinp_all[t][:, E:]), E + X,
                   L.ptr(dv_all[t]), L.ptr(dsproj_all[t]), L.ptr(dw_acc), B, N, A, X, L.stream())
            if t:
                ops.gemm(dgh_all[t], whh, B, S, 3 * S, tb=True, out=d1, out_kind=ops.OUT_F32)
                ops.gemm(dsproj_all[t], ws_, B, S, A, tb=True, out=d2, out_kind=ops.OUT_F32)
        # ---- weight gradients: one GEMM per weight over the stacked steps (rows (t, b)); state before step t = sbf_all[t]
        sprev = sbf_all[:steps].reshape(rows, S)
        dgi2, dgh2, dsp2, inp2 = dgi_all.view(rows, 3 * S), dgh_all.view(rows, 3 * S), dsproj_all.view(rows, A), inp.view(rows, E + X)
        side(lambda: ops.linear_wgrad(dgi2, inp2, g(PRE + "gru.weight_ih_l0")), dgi2, inp2)
        side(lambda: ops.colsum(dgi2, g(PRE + "gru.bias_ih_l0")), dgi2)
        side(lambda: ops.linear_wgrad(dgh2, sprev, g(PRE + "gru.weight_hh_l0")), dgh2, sprev)
        side(lambda: ops.colsum(dgh2, g(PRE + "gru.bias_hh_l0")), dgh2)
        side(lambda: ops.linear_wgrad(dsp2, sprev, g(PRE + "attention_unit.sEmbed.weight")), dsp2, sprev)
        side(lambda: ops.colsum(dsp2, g(PRE + "attention_unit.sEmbed.bias")), dsp2)
        side(lambda: ops.colsum_partials(dw_acc, g(PRE + "attention_unit.wEmbed.weight").view(A)), dw_acc)   # (wEmbed.bias: softmax-invariant, gradient 0)
        dyp = dinp_all.view(rows, E + X)[:, :E].contiguous()
        side(lambda: L.call("dig_seq_embed_bwd", L.ptr(yprev), L.ptr(dyp), L.ptr(g(PRE + "tgt_embedding.weight")), rows, E, C + 1, L.stream()), dyp)
        # ---- token gradients: sums over the steps, then the xEmbed Linear
        dxproj = torch.empty_like(xproj)
        dx = torch.empty_like(x)
        L.call("dig_addattn_bwd_tokens", L.ptr(xproj), L.ptr(sproj_all), L.ptr(wv), L.ptr(dv_all), L.ptr(alpha_all), L.ptr(dinp_all.view(rows, E + X)[:, E:]),
               E + X, L.ptr(dxproj), L.ptr(dx), steps, B, N, A, X, L.stream())
        side(lambda: ops.linear_wgrad(dxproj, x, g(PRE + "attention_unit.xEmbed.weight")), dxproj, x)
        side(lambda: ops.colsum(dxproj, g(PRE + "attention_unit.xEmbed.bias")), dxproj)
        dx2 = ops.linear_dgrad(dxproj, w(PRE + "attention_unit.xEmbed.weight"))
        ops.add_bf16(dx, dx2, dx)
        self.encoder_backward(dx)
        main.wait_stream(sd)


class AttnRecModelTrain(EncoderTrain):
    """models.model_builder.AttnRecModel: `.train()` forward = teacher-forced logits [B, max_len, nb_classes] (+ three Nones),
    `.eval()` forward = greedy `sample` probabilities, both as the reference returns them; built with args.beam_width = K in 1..8 the
    `.eval()` forward is `beam_search`: token ids [B, max_len] (+ None, None, ones), as RecModel returns them under its beam."""
    _step_cls = _AttnTrainStep

    def __init__(self, args=None, *, sDim=512, attDim=512, **kw):
        # the reference never reaches AttentionRecognitionHead.beam_search: AttnRecModel.forward (model_builder.py:66-72) calls the head's
        # __call__ (forward_train / sample) whatever args.beam_width says, and the method itself indexes with the float result of
        # `candidates / num_classes` (attn_decoder.py:126-127).  Here args.beam_width = K > 0 makes the `.eval()` forward run that method,
        # with the division an integer one; 0 keeps the greedy sample().
        bw = int(getattr(args, "beam_width", 0) or 0)
        if not 0 <= bw <= MAX_BEAM_WIDTH:
            raise ValueError(f"beam_width {bw}: 0 (greedy sample) or a beam search of width 1..{MAX_BEAM_WIDTH}")
        self.sDim, self.attDim = sDim, attDim
        super().__init__(args, **kw)
        self.beam_width = bw
        self.eos = self.nb_classes - 3                                      # a vocabulary ends in EOS, PADDING, UNKNOWN (datasets.find_classes)
        if attDim % 8 or attDim > 1024 or sDim % 64 or (attDim + self.D) % 64:
            raise NotImplementedError("attDim must be a multiple of 8 (<= 1024), sDim and attDim + embed_dim multiples of 64")

    def head_shapes(self):
        D, A, S, C, o = self.D, self.attDim, self.sDim, self.nb_classes, {}
        o[PRE + "attention_unit.sEmbed.weight"] = (A, S); o[PRE + "attention_unit.sEmbed.bias"] = (A,)
        o[PRE + "attention_unit.xEmbed.weight"] = (A, D); o[PRE + "attention_unit.xEmbed.bias"] = (A,)
        o[PRE + "attention_unit.wEmbed.weight"] = (1, A); o[PRE + "attention_unit.wEmbed.bias"] = (1,)
        o[PRE + "tgt_embedding.weight"] = (C + 1, A)
        o[PRE + "gru.weight_ih_l0"] = (3 * S, D + A); o[PRE + "gru.weight_hh_l0"] = (3 * S, S)
        o[PRE + "gru.bias_ih_l0"] = (3 * S,); o[PRE + "gru.bias_hh_l0"] = (3 * S,)
        o[PRE + "fc.weight"] = (C, S); o[PRE + "fc.bias"] = (C,)
        return o

    def _init_tensor(self, k, shp):
        """Head: PyTorch defaults, which AttnRecModel keeps (the `init_weights` methods of attn_decoder.py are commented out,
        :206,249): nn.Linear U(+-1/sqrt(fan_in)), nn.Embedding N(0,1), nn.GRU U(+-1/sqrt(sDim)) for all four tensors."""
        if not k.startswith(PRE):
            return super()._init_tensor(k, shp)
        if "tgt_embedding" in k:
            return torch.randn(shp)
        if ".gru." in k:
            return (torch.rand(shp) * 2 - 1) / math.sqrt(self.sDim)
        fan_in = self.param_shapes()[k.rsplit(".", 1)[0] + ".weight"][1]
        return (torch.rand(shp) * 2 - 1) / math.sqrt(fan_in)

    # ------------------------------------------------------------------ eval: greedy sample (attn_decoder.py:58-78)
    @torch.no_grad()
    def sample(self, images):
        dev, B, N = images.device, images.shape[0], self.N
        step, x = self.eval_tokens(images)
        A, S, X, E, C = step._w()
        hd = step.head_inputs(x)
        cls_w, cb = self.padded_classifier(PRE + "fc.weight", PRE + "fc.bias", CLS_PAD)
        probs = torch.empty((B, self.max_len, C), device=dev, dtype=F32)
        s = torch.zeros((B, S), device=dev, dtype=F32)
        sbf = torch.zeros((B, S), device=dev, dtype=BF16)
        y = torch.full((B,), C, device=dev, dtype=torch.int64)
        inp = torch.empty((B, E + X), device=dev, dtype=BF16)
        alpha = torch.empty((B, N), device=dev, dtype=F32)
        gates = torch.empty((B, 4 * S), device=dev, dtype=F32)
        logit = torch.empty((B, CLS_PAD), device=dev, dtype=F32)
        tok = torch.empty((B,), device=dev, dtype=torch.int64)
        pbuf = torch.empty((B, C), device=dev, dtype=F32)
        emb = step.p(PRE + "tgt_embedding.weight")
        for t in range(self.max_len):
            L.call("dig_embed_rows", L.ptr(y), L.ptr(emb), L.ptr(inp), E + X, B, E, C + 1, L.stream())
            s_new, sbf_new, sproj = torch.empty_like(s), torch.empty_like(sbf), torch.empty((B, A), device=dev, dtype=BF16)
            step.gru_attention_step(hd, sbf, s, inp, sproj, alpha, s_new, sbf_new, gates)
            s, sbf = s_new, sbf_new
            ops.gemm(sbf, cls_w, B, CLS_PAD, S, out=logit, out_kind=ops.OUT_F32, bias=cb)
            L.call("dig_softmax_argmax", L.ptr(logit), CLS_PAD, L.ptr(pbuf), L.ptr(tok), B, C, L.stream())
            probs[:, t] = pbuf
            y = tok.clone()
        return probs

    # ------------------------------------------------------------------ eval: beam search (attn_decoder.py:84-200)
    @torch.no_grad()
    def beam_search(self, images, beam_width, eos=None, force_logits=None, force_decisions=None, return_logits=False):
        """AttentionRecognitionHead.beam_search with `predecessors` an integer division (the reference's float result cannot index on a
        current torch).  The K = beam_width hypotheses of a sample are rows b*K .. b*K + K - 1 of every per-step tensor and share the
        sample's encoder tokens and xEmbed(x), which stay one copy per sample (`dig_addattn_fwd_slots`).  A step is 7 launches: the sEmbed
        GEMM, the K-slot attention, the two gate GEMMs, the GRU cell, the classifier GEMM and `dig_attn_beam_advance`, which ranks the K*C
        candidates by dig_beam_step's rule, moves every slot's recurrent state to that of its predecessor (attn_decoder.py:127-128; the
        transformer decoder's beam never re-orders its slots) and writes the emitted symbols' embeddings for the next step.  The decisions
        [T, B*K] go to the host once, into `recognizer.beam_backtrack` (the rule of :140-200).  Returns ids [B, max_len] int64.
        Parity hooks: force_logits ([T, B*K, C] fp32) stand in for the classifier's outputs in the ranking; force_decisions ([T, B, K]
        int64 candidate indices k*C + c) stand in for the top-K; return_logits also returns (logits [T, B*K, C], scores, predecessors,
        symbols [T, B*K]) of the run."""
        from .recognizer import beam_backtrack
        K = int(beam_width)
        if not 1 <= K <= MAX_BEAM_WIDTH:
            raise ValueError(f"beam_width {beam_width}: a width of 1..{MAX_BEAM_WIDTH}")
        eos = self.eos if eos is None else int(eos)
        dev, B, N, T = images.device, images.shape[0], self.N, self.max_len
        step, x = self.eval_tokens(images)
        A, S, X, E, C = step._w()
        hd = step.head_inputs(x)
        cls_w, cb = self.padded_classifier(PRE + "fc.weight", PRE + "fc.bias", CLS_PAD)
        emb = step.p(PRE + "tgt_embedding.weight")
        R = B * K
        s, sbf = torch.zeros((R, S), device=dev, dtype=F32), torch.zeros((R, S), device=dev, dtype=BF16)     # step 0: zero state (:97)
        s_new, sbf_new = torch.empty_like(s), torch.empty_like(sbf)
        inp = torch.empty((R, E + X), device=dev, dtype=BF16)
        sproj = torch.empty((R, A), device=dev, dtype=BF16)
        gates = torch.empty((R, 4 * S), device=dev, dtype=F32)
        logit = torch.empty((R, CLS_PAD), device=dev, dtype=F32)
        seq_scores = torch.full((R,), float("-inf"), device=dev, dtype=F32)
        seq_scores[::K] = 0.0                                                # only slot 0 of a sample is live at step 0 (:101-103)
        syms = torch.empty((T, R), device=dev, dtype=torch.int64)
        preds = torch.empty((T, R), device=dev, dtype=torch.int64)
        scores = torch.empty((T, R), device=dev, dtype=F32)
        forced = None if force_decisions is None else force_decisions.to(dev).long().reshape(T, R).contiguous()
        flog = None if force_logits is None else force_logits.to(dev).float().contiguous()
        kept = []
        bos = torch.full((R,), C, device=dev, dtype=torch.int64)             # <BOS> = num_classes (:107)
        L.call("dig_embed_rows", L.ptr(bos), L.ptr(emb), L.ptr(inp), E + X, R, E, C + 1, L.stream())
        for t in range(T):
            step.gru_attention_step(hd, sbf, s, inp, sproj, None, s_new, sbf_new, gates, slots=K)
            ops.gemm(sbf_new, cls_w, R, CLS_PAD, S, out=logit, out_kind=ops.OUT_F32, bias=cb)
            if return_logits:
                kept.append(logit[:, :C].clone())
            lg, ld = (logit, CLS_PAD) if flog is None else (flog[t], flog.shape[-1])
            L.call("dig_attn_beam_advance", L.ptr(lg), ld, L.ptr(seq_scores), B, K, C, eos, L.ptr(syms[t]), L.ptr(preds[t]), L.ptr(scores[t]),
                   L.ptr(forced[t]) if forced is not None else None, L.ptr(s_new), L.ptr(sbf_new), L.ptr(s), L.ptr(sbf), S, L.ptr(emb), E,
                   L.ptr(inp), E + X, L.stream())
        # one device -> host copy: float64 holds the fp32 scores (-inf included) and the small integers exactly
        host = torch.stack([scores.double(), preds.double(), syms.double()]).cpu().numpy()
        ids = beam_backtrack(host[0], host[1].astype("int64"), host[2].astype("int64"), B, K, eos).to(dev)
        return (ids, torch.stack(kept), scores, preds, syms) if return_logits else ids

    def forward(self, x):
        if self.training:
            lens = x[2]
            self._steps_hint = int(lens.max()) if (torch.is_tensor(lens) and not lens.is_cuda and lens.numel()) else None
            return super().forward(x)
        if self.beam_width > 0:
            # token ids and an all-ones tensor in place of (probabilities, attention maps), as RecModel.forward returns them under a beam
            ids = self.beam_search(self._device_images(x), self.beam_width)
            return ids, None, None, torch.ones_like(ids)
        return self.sample(self._device_images(x)), None, None, None
