"""The recognition decoders with head dim 24 and 48 (`corres_tiny_tf_decoder`, `corres_small_tf_decoder`; `corres_base_tf_decoder` is head dim
64): the attention kernels at every head dim against fp32 torch on both builds of the ABI, the oracles and the model against the fixture written
from the unmodified reference (tools/gen_corres_decoder_golden.py), the model surface, and one full-size step on the device."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import decode_oracle as D
import dig_oracle as O
import finetune_oracle as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
cf = ctypes.c_float
POISON = 768.0                    # (exact in bf16)
CORRES = {"corres_tiny_tf_decoder": (192, 8, 24, 768), "corres_small_tf_decoder": (384, 8, 48, 1536), "corres_base_tf_decoder": (512, 8, 64, 2048)}


def _sample_index(numel, k=8):
    if numel <= k:
        return np.arange(numel)
    return (np.arange(k, dtype=np.int64) * 2654435761 + 12345) % numel


def _samples(t):
    return np.resize(t.reshape(-1)[_sample_index(t.numel())].numpy(), 8)


# ------------------------------------------------------------------------------------------------ 1. sequence attention kernels
def _seq_case(dev, dk, Lq, Lk, causal, seed):
    """q|k|v as views of one [B*L + 2, 3*hk + 16] buffer (self-attention) or q of one and k|v of another (cross): non-contiguous leading dimensions,
    16 pad columns and 2 pad rows that the kernels must not touch."""
    g = torch.Generator().manual_seed(seed)
    B, H = 2, 3
    hk = H * dk
    pad = 16
    if Lq == Lk:
        buf = torch.randn(B * Lk + 2, 3 * hk + pad, generator=g).bfloat16().to(dev)
        q, k, v = buf[:B * Lq, :hk], buf[:B * Lk, hk:2 * hk], buf[:B * Lk, 2 * hk:3 * hk]
    else:
        qb = torch.randn(B * Lq + 2, hk + pad, generator=g).bfloat16().to(dev)
        buf = torch.randn(B * Lk + 2, 3 * hk + pad, generator=g).bfloat16().to(dev)
        q, k, v = qb[:B * Lq, :hk], buf[:B * Lk, hk:2 * hk], buf[:B * Lk, 2 * hk:3 * hk]
    dout = torch.randn(B * Lq, hk, generator=g).bfloat16().to(dev)
    lens = torch.tensor([1, Lk], device=dev) if causal else None
    return B, H, hk, q, k, v, dout, lens


def _seq_run(L, name_suffix, dk, B, H, Lq, Lk, scale, causal, q, k, v, dout, lens, drop):
    """Forward + backward through the entry points `dig_seq_attn_{fwd,bwd}<name_suffix>`; outputs are views of poisoned buffers (rows past B*L,
    columns outside the heads), returned with the buffers."""
    dev, hk = q.device, H * dk
    ob = torch.full((B * Lq + 2, hk + 16), POISON, device=dev).bfloat16()
    gb = torch.full((B * Lk + 2, 3 * hk + 16), POISON, device=dev).bfloat16()
    lse = torch.empty(B, H, Lq, device=dev)
    out = ob[:B * Lq, 8:8 + hk]                                           # 16-byte aligned, columns [8, 8 + hk) of hk + 16
    dq, dkk, dv = gb[:B * Lq, :hk], gb[:B * Lk, hk:2 * hk], gb[:B * Lk, 2 * hk:3 * hk]
    ld = lambda t: t.stride(0)
    tail = (ctypes.byref(drop) if drop is not None else None,) if name_suffix != "" else ()
    hd = (dk,) if name_suffix == "_hd" else ()
    L.call("dig_seq_attn_fwd" + name_suffix, L.ptr(q), ld(q), L.ptr(k), ld(k), L.ptr(v), ld(v), L.ptr(out), ld(out), L.ptr(lse), B, H, Lq, Lk, cf(scale),
           int(causal), L.ptr(lens), *tail, *hd, L.stream())
    L.call("dig_seq_attn_bwd" + name_suffix, L.ptr(q), ld(q), L.ptr(k), ld(k), L.ptr(v), ld(v), L.ptr(dout), ld(dout), L.ptr(lse), L.ptr(dq), ld(dq),
           L.ptr(dkk), ld(dkk), L.ptr(dv), ld(dv), B, H, Lq, Lk, cf(scale), int(causal), L.ptr(lens), *tail, *hd, L.stream())
    return out, lse, dq, dkk, dv, ob, gb


def _seq_ref(dk, B, H, Lq, Lk, scale, causal, q, k, v, dout, lens, keep=None):
    """fp32 torch on the bf16 operands; keep: [B, H, Lq, Lk] factors of the attention dropout (0 or 1 / (1 - p)), or None."""
    heads = lambda t, Ln: t.float().reshape(B, Ln, H, dk).permute(0, 2, 1, 3).clone().requires_grad_(True)
    qh, kh, vh = heads(q, Lq), heads(k, Lk), heads(v, Lk)
    logits = qh @ kh.transpose(-1, -2) * scale
    if causal:
        dev = q.device
        mask = (torch.arange(Lk, device=dev)[None, :] < lens[:, None])[:, None, :] & torch.tril(torch.ones(Lq, Lk, device=dev)).bool()[None]
        logits = logits.masked_fill(~mask[:, None], float("-inf"))
    w = logits.softmax(-1)
    if keep is not None:
        w = w * keep
    ref = (w @ vh).permute(0, 2, 1, 3).reshape(B * Lq, H * dk)
    ref.backward(dout.float())
    back = lambda t, Ln: t.permute(0, 2, 1, 3).reshape(B * Ln, H * dk)
    return ref.detach(), torch.logsumexp(logits.detach(), -1), back(qh.grad, Lq), back(kh.grad, Lk), back(vh.grad, Lk)


def _untouched(ob, gb, B, Lq, Lk, hk):
    """The poison outside the written views is still there: rows past B*L, columns outside the heads' range."""
    p = torch.tensor(POISON).bfloat16().item()
    assert bool((ob[B * Lq:] == p).all()) and bool((ob[:, :8] == p).all()) and bool((ob[:, 8 + hk:] == p).all())
    assert bool((gb[B * Lk:] == p).all()) and bool((gb[:, 3 * hk:] == p).all())
    if Lq < Lk:
        assert bool((gb[B * Lq:, :hk] == p).all())


@pytest.mark.parametrize("Lq,Lk", [(5, 5), (25, 25), (32, 64), (25, 65), (25, 256)])
@pytest.mark.parametrize("dk", [24, 48, 64])
def test_seq_attention_hd_vs_torch(abi_dev, dk, Lq, Lk):
    """dig_seq_attn_fwd_hd / _bwd_hd at head dim 24 / 48 / 64, three heads (a wrong head stride lands in another head's columns), both sides of
    the Lk <= 64 switch, causal with lens (one sample with lens = 1) where Lq == Lk and plain otherwise; tolerances of the head-64 tests in
    tests/test_finetune.py (a 24- or 48-term bf16 dot product has no more error than a 64-term one).  At head dim 64 bit-equal to the entry
    points without a head-dim argument."""
    from dig_amd import _lib as L
    dev = abi_dev
    causal = Lq == Lk
    scale = dk ** -0.5
    B, H, hk, q, k, v, dout, lens = _seq_case(dev, dk, Lq, Lk, causal, 100 + dk + Lk)
    out, lse, dq, dkk, dv, ob, gb = _seq_run(L, "_hd", dk, B, H, Lq, Lk, scale, causal, q, k, v, dout, lens, None)
    ref, rlse, rdq, rdk, rdv = _seq_ref(dk, B, H, Lq, Lk, scale, causal, q, k, v, dout, lens)
    rel = lambda a, b: ((a.float() - b).norm() / (b.norm() + 1e-12)).item()
    errs = ((out.float() - ref).abs().max().item(), (lse - rlse).abs().max().item(), rel(dq, rdq), rel(torch.cat([dkk, dv], 1), torch.cat([rdk, rdv], 1)))
    print(f"head dim {dk}, {Lq} x {Lk}: out {errs[0]:.3e}, lse {errs[1]:.3e}, dq {errs[2]:.3e}, dk|dv {errs[3]:.3e}")
    assert errs[0] < 3e-2 and errs[1] < 1e-3 and errs[2] < 2e-2 and errs[3] < 2e-2
    _untouched(ob, gb, B, Lq, Lk, hk)
    if dk == 64:
        for suffix in ("", "_dropout"):
            o2, l2, dq2, dk2, dv2, _, _ = _seq_run(L, suffix, dk, B, H, Lq, Lk, scale, causal, q, k, v, dout, lens, None)
            assert torch.equal(o2, out) and torch.equal(l2, lse) and torch.equal(dq2, dq) and torch.equal(dk2, dkk) and torch.equal(dv2, dv)


@pytest.mark.parametrize("dk", [24, 48, 64])
def test_seq_attention_hd_dropout_vs_torch_with_oracle_masks(abi_dev, dk):
    """Attention dropout on: the keyed mask rule of include/dig_hip.h (element ((query << 16) | key, sample * heads + head)), restated by
    finetune_oracle.DropOracle; bounds of test_finetune.py::test_attention_dropout_kernels_vs_torch_with_oracle_masks."""
    from dig_amd import _lib as L, dropout as DR
    dev = abi_dev
    dr = F.DropOracle(5, 11, attn_drop=0.1, decoder_dropout=0.1)
    plan = DR.DropPlan(5, 11)
    for Lq, Lk, causal, kind in ((8, 8, True, 0), (8, 72, False, 2)):
        scale = dk ** -0.5
        B, H, hk, q, k, v, dout, lens = _seq_case(dev, dk, Lq, Lk, causal, 7 + dk)
        sp = plan.spec(DR.dec_site(1, kind), 0.1)
        out, lse, dq, dkk, dv, ob, gb = _seq_run(L, "_hd", dk, B, H, Lq, Lk, scale, causal, q, k, v, dout, lens, sp)
        keep = dr.attn(F.dec_site(1, kind), torch.ones(B, H, Lq, Lk), 0.1).to(dev)
        assert 0.02 < (keep == 0).float().mean().item() < 0.25
        ref, _, rdq, rdk, rdv = _seq_ref(dk, B, H, Lq, Lk, scale, causal, q, k, v, dout, lens, keep)
        assert (out.float() - ref).abs().max() < 3e-2 * ref.abs().max()
        for got, want in ((dq, rdq), (dkk, rdk), (dv, rdv)):
            assert (got.float() - want).abs().max() < 4e-2 * want.abs().max() + 1e-3
        _untouched(ob, gb, B, Lq, Lk, hk)


def test_seq_attention_hd_rejects_other_head_dims(abi_dev):
    from dig_amd import _lib as L
    dev = abi_dev
    B, H, hk, q, k, v, dout, lens = _seq_case(dev, 32, 5, 5, True, 3)
    with pytest.raises(L.DigHipError, match="unsupported"):
        _seq_run(L, "_hd", 32, B, H, 5, 5, 0.2, True, q, k, v, dout, lens, None)


# ------------------------------------------------------------------------------------------------ 2. decode kernels
@pytest.mark.parametrize("dk", [24, 48, 64])
def test_decode_attention_kernels_hd_vs_torch(abi_dev, dk):
    """dig_decode_self_attn (T = 8, t in {0, 3, 7}) and dig_decode_cross_attn (n_mem in {1, 7, 32, 33, 256, 257}: fewer keys than the 32 key
    slots, a second pass of the 256-thread loops; slots_per_mem in {1, 2}, with and without `weights`) at head dim 24 / 48 / 64; tolerances of test_decode.py::test_decode_attention_kernels_vs_torch.  Rows behind the outputs stay untouched."""
    from dig_amd import _lib as L
    dev = abi_dev
    torch.manual_seed(dk)
    B, T, H = 6, 8, 3
    hk, scale = H * dk, dk ** -0.5
    qkv = torch.randn(B, T, 3 * hk, device=dev).to(torch.bfloat16)
    for t in (0, 3, 7):
        ob = torch.full((B + 1, hk), POISON, device=dev).bfloat16()
        L.call("dig_decode_self_attn", L.ptr(qkv), L.ptr(ob), B, T, H, dk, t, cf(scale), L.stream())
        q = qkv[:, t, :hk].float().view(B, H, 1, dk)
        k = qkv[:, :t + 1, hk:2 * hk].float().view(B, t + 1, H, dk).permute(0, 2, 1, 3)
        v = qkv[:, :t + 1, 2 * hk:].float().view(B, t + 1, H, dk).permute(0, 2, 1, 3)
        ref = ((q @ k.transpose(-1, -2) * scale).softmax(-1) @ v).reshape(B, hk)
        assert (ob[:B].float() - ref).abs().max().item() < 2e-2 and bool((ob[B:].float() == POISON).all())
    for Nm in (1, 7, 32, 33, 256, 257):
        for spm in (1, 2):
            q = torch.randn(B, hk, device=dev).to(torch.bfloat16)
            kv = torch.randn(B // spm, Nm, 2 * hk, device=dev).to(torch.bfloat16)
            qf = q.float().view(B, H, 1, dk)
            kvb = kv.repeat_interleave(spm, 0)
            kf = kvb[:, :, :hk].float().view(B, Nm, H, dk).permute(0, 2, 1, 3)
            vf = kvb[:, :, hk:].float().view(B, Nm, H, dk).permute(0, 2, 1, 3)
            wr = (qf @ kf.transpose(-1, -2) * scale).softmax(-1)
            outs = []
            for with_w in (True, False):
                ob = torch.full((B + 1, hk), POISON, device=dev).bfloat16()
                w = torch.full((B + 1, H, Nm), POISON, device=dev)
                L.call("dig_decode_cross_attn", L.ptr(q), L.ptr(kv), L.ptr(ob), L.ptr(w) if with_w else None, B, Nm, H, dk, cf(scale), spm, L.stream())
                assert (ob[:B].float() - (wr @ vf).reshape(B, hk)).abs().max().item() < 2e-2 and bool((ob[B:].float() == POISON).all())
                if with_w:
                    assert (w[:B] - wr[:, :, 0]).abs().max().item() < 1e-4 and bool((w[B:] == POISON).all())
                outs.append(ob)
            assert torch.equal(outs[0], outs[1])


def test_decode_attention_kernels_reject_head_dim_32(abi_dev):
    from dig_amd import _lib as L
    dev = abi_dev
    B, T, H, dk, Nm = 2, 4, 2, 32, 16
    hk = H * dk
    qkv = torch.randn(B, T, 3 * hk, device=dev).to(torch.bfloat16)
    q = torch.randn(B, hk, device=dev).to(torch.bfloat16)
    kv = torch.randn(B, Nm, 2 * hk, device=dev).to(torch.bfloat16)
    out = torch.full((B, hk), POISON, device=dev).bfloat16()
    w = torch.full((B, H, Nm), POISON, device=dev)
    with pytest.raises(L.DigHipError, match="unsupported"):
        L.call("dig_decode_self_attn", L.ptr(qkv), L.ptr(out), B, T, H, dk, 1, cf(0.2), L.stream())
    with pytest.raises(L.DigHipError, match="unsupported"):
        L.call("dig_decode_cross_attn", L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(w), B, Nm, H, dk, cf(0.2), 1, L.stream())
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((out.float() == POISON).all()) and bool((w == POISON).all())


# ------------------------------------------------------------------------------------------------ fixture
_G = {}


def _gold():
    if not _G:
        _G["g"] = np.load(os.path.join(GOLD, "corres_decoder_tiny.npz"))
    return _G["g"]


def _fixture(tag):
    """(values of the fixture under `tag`, decoder config, encoder config, seeded parameters (classifier as seeded), the same with the evaluation's
    classifier scale, images, targets, lens); computed once per tag and not modified by the tests."""
    if tag not in _G:
        g = _gold()
        v = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}
        nl, d, nh, dk, di, T, ed = (int(x) for x in v["config"])
        c = D.DecoderConfig(n_layers=nl, d_model=d, n_head=nh, d_k=dk, d_inner=di, max_seq_len=T, enc_dim=ed)
        ecfg = O.DiGConfig(**O.TINY)
        P = {**D.det_encoder_state(ecfg, int(v["seed_enc"])), **D.det_decoder_state(c, int(v["seed_dec"]))}
        Pe = dict(P)
        Pe["decoder.classifier.weight"] = P["decoder.classifier.weight"] * float(v["cls_scale"])
        images = O.synthetic_batch(int(v["B"]), ecfg, int(v["batch_seed"]))[0]
        _G[tag] = (v, c, ecfg, P, Pe, images, torch.from_numpy(v["targets"]), torch.from_numpy(v["lens"]))
    return _G[tag]


TAGS = ["h8k24", "h4k48"]


def _memory(P, ecfg, c, images):
    e = D.encoder_features(P, ecfg, images)
    return torch.nn.functional.layer_norm(e @ P["linear_norm.0.weight"].t() + P["linear_norm.0.bias"], (c.d_model,), P["linear_norm.1.weight"],
                                          P["linear_norm.1.bias"], 1e-5)


# ------------------------------------------------------------------------------------------------ 3. oracles vs fixture (CPU)
@pytest.mark.parametrize("tag", TAGS)
def test_oracles_match_reference_fixture(tag):
    v, c, ecfg, P, Pe, images, targets, lens = _fixture(tag)
    assert (c.n_head, c.d_k) in ((8, 24), (4, 48)) and c.n_head * c.d_k == c.d_model == 192
    loss, grads, logits = F.loss_and_grads(P, ecfg, c, images, targets, lens)
    assert abs(loss - float(v["loss"])) < 1e-5 * float(v["loss"])
    np.testing.assert_allclose(logits.numpy(), v["logits"], atol=3e-5)
    for i, n in enumerate(v["grad_names"].tolist()):
        gi = grads[n]
        assert abs(gi.double().norm().item() - v["grad_norms"][i]) <= 3e-4 * v["grad_norms"][i] + 1e-7, n
        np.testing.assert_allclose(_samples(gi), v["grad_samples"][i], rtol=2e-3, atol=1e-5 * (np.abs(v["grad_samples"][i]).max() + 1e-3))
    probs, maps, toks = D.recognize(Pe, ecfg, c, images)
    assert np.array_equal(toks.numpy(), v["greedy_tokens"])
    np.testing.assert_allclose(probs.numpy(), v["greedy_probs"], atol=1e-5)
    np.testing.assert_allclose(maps.double().norm(dim=-1).numpy(), v["greedy_map_norms"], rtol=1e-4)
    np.testing.assert_allclose(np.stack([_samples(m) for m in maps.reshape(-1, maps.shape[-1])]), v["greedy_map_samples"], atol=1e-5)
    top2 = probs.topk(2, -1).values
    g = _gold()
    assert np.array_equal(((top2[..., 0] - top2[..., 1]) > float(g["margin"])).numpy(), v["greedy_clear"])
    ids = D.beam_search(Pe, c, _memory(Pe, ecfg, c, images), int(g["beam_width"]), int(g["eos"]))
    assert np.array_equal(ids.numpy(), v["beam_ids"])
    # the cap on what the tie rule may exclude
    assert int((~v["greedy_clear"]).sum()) * 8 <= v["greedy_clear"].size and int((~v["beam_clear"]).sum()) * 8 <= v["beam_clear"].size


# ------------------------------------------------------------------------------------------------ 4. model vs fixture (GPU)
def _device_model(c, ecfg, P, train=True):
    from dig_amd.finetune import RecModelTrain
    m = RecModelTrain(embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads, n_layers=c.n_layers, d_model=c.d_model, n_head=c.n_head,
                      d_k=c.d_k, d_inner=c.d_inner, nb_classes=c.num_classes, max_len=c.max_seq_len, decoder_dropout=0.0)
    m.load_state_dict(P)
    m.to("cuda:0")
    return m.train(train)


def _grad_check(grads, ref_g, bf_g, names, norms):
    """The gradient bounds of test_finetune.py::test_device_finetune_step_vs_reference_fixture: per tensor, direction and size no further from the fp32
    oracle than twice the oracle under CPU bf16 autocast, plus 5e-3 / 3e-2."""
    cos = torch.nn.functional.cosine_similarity
    tot = float(np.sqrt((norms ** 2).sum()))
    bad = []
    for i, n in enumerate(names):
        if norms[i] < 1e-3 * tot:
            continue
        r = ref_g[n].reshape(1, -1)
        c_hip, c_bf = cos(grads[n].reshape(1, -1), r).item(), cos(bf_g[n].float().reshape(1, -1), r).item()
        q_hip, q_bf = grads[n].norm().item() / norms[i], bf_g[n].float().norm().item() / norms[i]
        if (1 - c_hip) > 2 * (1 - c_bf) + 5e-3 or abs(q_hip - 1) > 2 * abs(q_bf - 1) + 3e-2:
            bad.append((n, c_hip, c_bf, q_hip, q_bf))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_device_training_step_vs_reference_fixture(tag):
    from dig_amd.finetune import SeqCrossEntropyLoss
    v, c, ecfg, P, _, images, targets, lens = _fixture(tag)
    m = _device_model(c, ecfg, P)
    logits = m((images.to("cuda:0"), targets, lens))[0]
    loss = SeqCrossEntropyLoss()(logits, targets, lens)
    loss.backward()
    ref_logits = torch.from_numpy(v["logits"])
    errs = (abs(loss.item() - float(v["loss"])) / float(v["loss"]), ((logits.detach().cpu() - ref_logits).norm() / ref_logits.norm()).item())
    print(f"{tag}: loss off by {errs[0]:.3e}, logits by {errs[1]:.3e} (relative)")
    assert errs[0] < 2e-2 and errs[1] < 2e-2
    _, ref_g, _ = F.loss_and_grads(P, ecfg, c, images, targets, lens)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        _, bf_g, _ = F.loss_and_grads(P, ecfg, c, images, targets, lens)
    grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters()}
    names, norms = v["grad_names"].tolist(), v["grad_norms"]
    assert not _grad_check(grads, ref_g, bf_g, names, norms)         # (ref_g carries the fixture's sampled gradients: test_oracles_match_reference_fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_device_greedy_and_beam_decoding_vs_reference_fixture(tag):
    g = _gold()
    v, c, ecfg, _, Pe, images, _, _ = _fixture(tag)
    m = _device_model(c, ecfg, Pe, train=False)
    dev = torch.device("cuda:0")
    m._prepare(dev)
    ref_p, ref_t = torch.from_numpy(v["greedy_probs"]), torch.from_numpy(v["greedy_tokens"])
    with torch.no_grad():
        mem = m.memory(m.encoder_features(images.to(dev)))
        probs, maps, toks = m.greedy_decode(mem, m.n_mem, force_tokens=ref_t.to(dev))
        ids = m.beam_search(mem, m.n_mem, int(g["beam_width"]), eos=int(g["eos"]))
    err = (probs.cpu() - ref_p).abs().max().item()
    print(f"{tag}: teacher-forced probabilities: max abs error {err:.3e}")
    assert err < 3e-2
    clear, bclear = torch.from_numpy(v["greedy_clear"]), torch.from_numpy(v["beam_clear"])
    assert int((~clear).sum()) * 8 <= clear.numel() and int((~bclear).sum()) * 8 <= bclear.numel()
    assert bool(toks.cpu().eq(ref_t)[clear].all())
    assert torch.equal(ids.cpu()[bclear], torch.from_numpy(v["beam_ids"])[bclear])
    maps = maps.cpu()
    assert maps.shape == (int(v["B"]), c.max_seq_len, 256) and (maps.sum(-1) - 1).abs().max().item() < 1e-3
    got = np.stack([_samples(r) for r in maps.reshape(-1, 256)])
    assert np.abs(got - v["greedy_map_samples"]).max() <= 3e-2 * np.abs(v["greedy_map_samples"]).max() + 1e-3


# ------------------------------------------------------------------------------------------------ 5. surface
def _args(name, encoder=None, **kw):
    g = _gold()
    return types.SimpleNamespace(model=encoder or str(g["encoder/" + name]), decoder_name=name, nb_classes=97, max_len=25, **kw)


@pytest.mark.parametrize("name", list(CORRES))
def test_corres_decoders_construct_with_the_reference_state_dict(name):
    from dig_amd.recognizer import RecModel, DECODERS
    g = _gold()
    d, nh, dk, di = CORRES[name]
    assert DECODERS[name] == dict(n_layers=6, d_model=d, n_head=nh, d_k=dk, d_inner=di)
    m = RecModel(_args(name))
    assert (m.d, m.nh, m.dk, m.d_inner, m.n_layers) == (d, nh, dk, di, 6)
    ref = {k: tuple(int(x) for x in s if x) for k, s in zip(g["keys/" + name].tolist(), g["shapes/" + name])}     # (shapes are zero-padded to 4 dims)
    ref = {k: s for k, s in ref.items() if not k.endswith("position_table") and not k.startswith("patch_embed.")}
    sd = m.state_dict()
    assert sorted(sd) == sorted(ref)
    assert {k: tuple(t.shape) for k, t in sd.items()} == ref
    gen = torch.Generator().manual_seed(1)
    new = {k: torch.randn(t.shape, generator=gen) for k, t in sd.items()}
    m.load_state_dict(new)
    back = m.state_dict()
    assert all(torch.equal(back[k], new[k]) for k in new)
    m2 = RecModel(_args(name))
    m2.load_state_dict(back)
    assert all(torch.equal(t, new[k]) for k, t in m2.state_dict().items())


def test_unbuilt_decoder_configurations_say_so():
    from dig_amd.recognizer import RecModel
    with pytest.raises(NotImplementedError, match="cls_query_attn_maps"):
        RecModel(_args("decoupled_tf_decoder", encoder="simmim_vit_small_patch4_32x128"))
    with pytest.raises(NotImplementedError, match="head dimension 24"):
        RecModel(_args("corres_tiny_tf_decoder", text_cond_vis=True))
    with pytest.raises(NotImplementedError, match="head dimension 48"):
        RecModel(_args("corres_small_tf_decoder", text_cond_vis=True))
    m = RecModel(_args("corres_base_tf_decoder", text_cond_vis=True))
    assert m.text_cond_vis and "decoder.layer_stack.5.enc_attn.gamma_decode.weight" in m.param_shapes()
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        RecModel(embed_dim=128, depth=2, num_heads=2, n_layers=1, d_model=128, n_head=4, d_k=32, d_inner=64)


# ------------------------------------------------------------------------------------------------ 6. one full-size step (GPU)
@pytest.mark.gpu
def test_full_size_corres_tiny_step_and_graph_decode():
    """corres_tiny_tf_decoder on simmim_vit_tiny_patch4_32x128, B = 4, every drop rate 0: finite loss, logits within the bound of the tiny
    training-step test of finetune_oracle on the same weights, one optimizer step changes every decoder tensor, and the greedy decode of the
    batch through the HIP-graph replay equals the eager decode bit for bit."""
    from dig_amd.finetune import RecModelTrain, SeqCrossEntropyLoss, create_optimizer
    torch.manual_seed(3)
    args = _args("corres_tiny_tf_decoder", drop=0.0, attn_drop_rate=0.0, drop_path=0.0)
    m = RecModelTrain(args, decoder_dropout=0.0).to("cuda:0").train()
    B, T = 4, 25
    ecfg = O.DiGConfig(embed_dim=192, depth=12, heads=3)
    c = D.DecoderConfig(n_layers=6, d_model=192, n_head=8, d_k=24, d_inner=768, enc_dim=192)
    images = O.synthetic_batch(B, ecfg, 9)[0]
    rng = np.random.RandomState(4)
    lens = torch.tensor([1, 25, 7, 13])
    targets = torch.from_numpy(rng.randint(0, 94, size=(B, T)))
    for b in range(B):
        targets[b, int(lens[b]) - 1] = 94
        targets[b, int(lens[b]):] = 95
    P = {k: t.clone() for k, t in m.state_dict().items()}
    opt = create_optimizer(types.SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None), m)
    opt.zero_grad()
    logits = m((images.to("cuda:0"), targets, lens))[0]
    loss = SeqCrossEntropyLoss()(logits, targets, lens)
    loss.backward()
    assert bool(torch.isfinite(loss))
    want = F.train_logits(P, ecfg, c, images, targets, lens)
    err = ((logits.detach().cpu() - want).norm() / want.norm()).item()
    print(f"full-size logits off by {err:.3e} (relative)")
    assert err < 2e-2
    opt.step()
    after = m.state_dict()
    same = [k for k in P if (k.startswith("decoder.") or k.startswith("linear_norm.")) and torch.equal(P[k], after[k])]
    assert not same, same
    m.eval()
    dev_images = images.to("cuda:0")
    m.use_hip_graph = False
    p0, _, _, a0 = m((dev_images, None, None))
    m.use_hip_graph = True
    for _ in range(2):                                                      # capture, then replay
        p1, _, _, a1 = m((dev_images, None, None))
        assert torch.equal(p0, p1) and torch.equal(a0, a1)
    assert p0.shape == (B, T, 97) and a0.shape == (B, T, 256) and bool(torch.isfinite(p0).all())
