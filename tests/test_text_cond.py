"""Text-conditional decoder cross-attention (`--text_cond_vis`): the fp32 specification (tests/textcond_model.py) against the fixture written
from the unmodified reference (tests/golden/text_cond_tiny.npz, tools/gen_text_cond_golden.py), the two entry points dig_tcv_attn_fwd / _bwd
against the specification on both builds of the ABI, and the model (training step, greedy / beam evaluation, checkpoints) on the device."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import decode_oracle as D
import dig_oracle as O
import finetune_oracle as FO
import textcond_model as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def _cpu_library():
    """cpu_abi/libdig_cpu.so is rebuilt by its own Makefile's dependencies (the test helper's rule does not list every source)."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "cpu_abi")], check=True, capture_output=True)


# ---------------------------------------------------------------------------------------------- operator level
# (S, Lq, N, heads, d, slots_per_mem): TINY; the largest supported; a key tail (37 = 4 * 9 + 1 keys, 6 heads); one query against shared memories
BWD_SHAPES = [(3, 5, 32, 2, 128, 1), (2, 25, 256, 8, 512, 1), (2, 7, 37, 6, 384, 1)]
FWD_SHAPES = BWD_SHAPES + [(6, 1, 256, 6, 384, 3)]
DROP_KEY = (0x1234ABCD, 0x0BADF00D)


def _drop_spec(p):
    from dig_amd import dropout as DR
    s = DR.DropSpec()
    s.k0, s.k1 = DROP_KEY
    s.thr, s.scale = DR.threshold(p), 1.0 / (1.0 - p)
    return s


@functools.lru_cache(maxsize=None)
def _case(shape, p):
    """Inputs (bf16 values) and the fp32 specification's outputs and gradients of one shape, computed once on the CPU."""
    S, Lq, N, H, d, spm = shape
    g = torch.Generator().manual_seed(S * 1000 + N)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = dict(film=rn(S, Lq, 2 * d).bfloat16(), u=(rn(S, Lq, H, d) * (1.5 / np.sqrt(2 * d))).bfloat16(), vk=rn(S // spm, N, d).bfloat16(),
             mem=rn(S // spm, N, d).bfloat16(), lg=1 + 0.1 * rn(d), lb=0.05 * rn(d), dc=rn(S, Lq, H, d).bfloat16())
    keep = None
    if p:
        from dig_amd import dropout as DR
        keep = TC.keep_factor(DROP_KEY[0], DROP_KEY[1], DR.threshold(p), 1.0 / (1.0 - p), S, H, Lq, N)
    leaves = {k: x[k].float().requires_grad_(True) for k in ("film", "u", "vk", "mem", "lg", "lb")}
    c, lse, wmean = TC.core(leaves["film"], leaves["u"], leaves["vk"], leaves["mem"], leaves["lg"], leaves["lb"], 1e-5, spm, keep)
    c.backward(x["dc"].float())
    ref = dict(c=c.detach(), lse=lse.detach(), wmean=wmean.detach(), **{"d" + k: v.grad for k, v in leaves.items()})
    return x, ref


def _run(dev, shape, p, x, backward=True):
    from dig_amd import ops
    S, Lq, N, H, d, spm = shape
    R, M = S * Lq, S // spm
    t = {k: v.to(dev).contiguous() for k, v in x.items()}
    film, u, vk, mem, dc = t["film"].view(R, 2 * d), t["u"].view(R, H * d), t["vk"].view(M * N, d), t["mem"].view(M * N, d), t["dc"].view(R, H * d)
    drop = _drop_spec(p) if p else None
    wmean = torch.empty(R, N, device=dev)
    c, lse = ops.tcv_attn_fwd(film, u, vk, mem, t["lg"], t["lb"], S, Lq, N, H, spm, drop, wmean)
    out = dict(c=c.view(S, Lq, H, d), lse=lse.view(S, Lq, H), wmean=wmean.view(S, Lq, N))
    if backward:
        dlg, dlb = torch.ones(d, device=dev), torch.full((d,), -2.0, device=dev)          # accumulated into
        du, dfilm, dvk, dmem = ops.tcv_attn_bwd(film, u, vk, mem, t["lg"], t["lb"], c, lse, dc, dlg, dlb, S, Lq, N, H, drop)
        out.update(du=du.view(S, Lq, H, d), dfilm=dfilm.view(S, Lq, 2 * d), dvk=dvk.view(M, N, d), dmem=dmem.view(M, N, d), dlg=dlg - 1.0, dlb=dlb + 2.0)
    return {k: v.float().cpu() for k, v in out.items()}


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _cos_ratio(a, b):
    return 1.0 - torch.nn.functional.cosine_similarity(a.reshape(1, -1), b.reshape(1, -1)).item(), abs(a.norm().item() / b.norm().item() - 1.0)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tcv_attention_entry_points_vs_spec(abi_dev, shape, p):
    """dig_tcv_attn_fwd / _bwd against the fp32 specification, with dropout off and under the same keyed masks.  Gate: at most twice the bf16
    yardstick's error (the specification's result rounded to bf16 where the entry points store bf16) plus a floor: 2^-8 on the relative
    Frobenius error of c and wmean (two bf16 roundings), 5e-3 on 1 - cos and 3e-2 on the norm ratio of every gradient (the fine-tune step's
    floors), 1e-3 absolute on lse."""
    x, ref = _case(shape, p)
    backward = shape[5] == 1
    got = _run(abi_dev, shape, p, x, backward)
    bf = lambda v: v.bfloat16().float()
    for k in ("c", "wmean"):
        err, yard = _rel(got[k], ref[k]), (_rel(bf(ref[k]), ref[k]) if k == "c" else 0.0)
        print(f"{k}: rel {err:.3e} yardstick {yard:.3e}")
        assert err <= 2 * yard + 2.0 ** -8, (k, err, yard)
    lse_err = (got["lse"] - ref["lse"]).abs().max().item()
    print(f"lse: abs {lse_err:.3e}")
    assert lse_err <= 1e-3
    if not backward:
        return
    for k in ("du", "dfilm", "dvk", "dmem", "dlg", "dlb"):
        r = ref[k]
        yard = _cos_ratio(bf(r), r) if k not in ("dlg", "dlb") else (0.0, 0.0)
        c1, q1 = _cos_ratio(got[k], r)
        print(f"{k}: 1-cos {c1:.3e} (yardstick {yard[0]:.3e}) norm ratio off by {q1:.3e} (yardstick {yard[1]:.3e})")
        assert c1 <= 2 * yard[0] + 5e-3 and q1 <= 2 * yard[1] + 3e-2, (k, c1, q1, yard)


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tcv_attention_is_deterministic_and_batch_independent(abi_dev, shape):
    """Two runs are bit-identical, and the batch equals its sequences run one at a time, bit for bit, in c / lse / wmean / du / dfilm."""
    x, _ = _case(shape, 0.0)
    a, b = _run(abi_dev, shape, 0.1, x), _run(abi_dev, shape, 0.1, x)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    full = _run(abi_dev, shape, 0.0, x)
    S = shape[0]
    for s in range(S):
        one = _run(abi_dev, (1,) + shape[1:], 0.0, {k: (v[s:s + 1] if v.dim() > 1 else v) for k, v in x.items()})
        for k in ("c", "lse", "wmean", "du", "dfilm"):
            assert torch.equal(one[k][0], full[k][s]), (k, s)


def _libs():
    from dig_amd import build
    import cpu_abi_util
    return [ctypes.CDLL(build.build(verbose=False)), ctypes.CDLL(cpu_abi_util.build())]


def test_tcv_bad_arguments_are_rejected_on_the_host():
    """Null pointers, unsupported shapes and misaligned rows return the ABI's codes before any launch (no GPU needed), on both builds."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    ok, odd, null = ctypes.c_void_p(base), ctypes.c_void_p(base + 2), ctypes.c_void_p(0)
    eps = ctypes.c_float(1e-5)
    for lib in _libs():
        fwd, bwd = lib.dig_tcv_attn_fwd, lib.dig_tcv_attn_bwd
        fwd.restype = bwd.restype = ctypes.c_int

        def f(film=ok, u=ok, c=ok, S=1, Lq=1, N=4, heads=2, d=128, spm=1):
            return fwd(film, u, ok, ok, ok, ok, eps, c, ok, null, S, Lq, N, heads, d, spm, null, null)

        def b(dc=ok, du=ok, ws=ok, N=4, heads=2, d=128, spm=1, S=1):
            return bwd(ok, ok, ok, ok, ok, ok, eps, ok, ok, dc, du, ok, ok, ok, ok, ok, ws, S, 1, N, heads, d, spm, null, null)

        assert f(film=null) == -1 and f(c=null) == -1 and f(S=0) == -1 and f(Lq=0) == -1 and f(N=0) == -1 and f(spm=0) == -1
        assert f(S=3, spm=2) == -1                                      # slots must divide the sequences
        assert f(d=256, heads=4) == -4 and f(heads=3) == -4 and f(N=257) == -4 and f(Lq=33) == -4
        assert f(u=odd) == -2 and f(c=odd) == -2
        assert b(dc=null) == -1 and b(ws=null) == -1 and b(N=0) == -1
        assert b(d=512, heads=6) == -4 and b(spm=2, S=2) == -4          # the backward owns one memory per sequence
        assert b(du=odd) == -2


def test_tcv_kernels_use_no_scratch():
    from dig_amd import build
    build.build(verbose=False)
    rows = [r for r in build.kernel_resources() if r["name"].startswith("tcv_")]
    assert {r["name"].split("(")[0] for r in rows} >= {f"tcv_{k}_kernel<{c}>" for k in ("fwd", "bwd_q", "bwd_k") for c in (2, 6, 8)} | {"tcv_fold_kernel"}
    assert [r for r in rows if r["scratch"]] == []


# ---------------------------------------------------------------------------------------------- specification and fixture
def _sample_index(numel, k=8):
    if numel <= k:
        return np.arange(numel)
    return (np.arange(k, dtype=np.int64) * 2654435761 + 12345) % numel


def _samples(t):
    return np.resize(t.reshape(-1)[_sample_index(t.numel())].numpy(), 8)


@functools.lru_cache(maxsize=None)
def _fixture():
    g = np.load(os.path.join(GOLD, "text_cond_tiny.npz"))
    c, ecfg = D.DecoderConfig(**D.TINY), O.DiGConfig(**O.TINY)
    P = {**D.det_encoder_state(ecfg, int(g["seed_enc"])), **D.det_decoder_state(c, int(g["seed_dec"])), **TC.det_text_cond_state(c, int(g["seed_tcv"]))}
    P["decoder.classifier.weight"] = P["decoder.classifier.weight"] * float(g["cls_scale"])
    images = O.synthetic_batch(int(g["B"]), ecfg, int(g["batch_seed"]))[0]
    return g, c, ecfg, P, images, torch.from_numpy(g["targets"]), torch.from_numpy(g["lens"])


def _check_grads(grads, names, norms, samples):
    for i, n in enumerate(names):
        gi = grads[n].detach()
        assert abs(gi.double().norm().item() - norms[i]) <= 3e-4 * norms[i] + 1e-7, n
        np.testing.assert_allclose(_samples(gi), samples[i], rtol=2e-3, atol=1e-5 * (np.abs(samples[i]).max() + 1e-3), err_msg=n)


@pytest.mark.parametrize("attn", [TC.attn_folded, TC.attn_literal], ids=["folded", "literal"])
def test_spec_training_step_matches_reference_fixture(attn):
    g, c, ecfg, P, images, targets, lens = _fixture()
    loss, grads, logits = TC.loss_and_grads(P, ecfg, c, images, targets, lens, attn=attn)
    assert abs(loss - float(g["loss"])) < 1e-5 * float(g["loss"])
    np.testing.assert_allclose(logits.numpy(), g["logits"], atol=3e-5)
    names = g["grad_names"].tolist()
    assert len(names) == len(P) - 1 and "encoder.mask_token" not in names
    _check_grads(grads, names, g["grad_norms"], g["grad_samples"])


def test_spec_decoding_matches_reference_fixture():
    """Greedy decoding and beam search (plain and with forced classifier outputs) of the specification against the reference's results."""
    g, c, ecfg, P, images, _, _ = _fixture()
    mem = TC.memory_of(P, ecfg, c, images)
    probs, maps, toks = TC.greedy_decode(P, c, mem)
    np.testing.assert_allclose(probs.numpy(), g["greedy_probs"], atol=2e-5)
    assert np.array_equal(toks.numpy(), g["greedy_tokens"])
    np.testing.assert_allclose(maps.double().norm(dim=-1).numpy(), g["greedy_map_norms"], rtol=1e-4)
    np.testing.assert_allclose(np.stack([_samples(m) for m in maps.reshape(-1, maps.shape[-1])]), g["greedy_map_samples"], atol=2e-6)
    top2 = probs.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > float(g["margin"])
    assert np.array_equal(clear.numpy(), g["greedy_clear"]) and int(g["n_clear"]) * 2 >= clear.numel()
    bw, eos = int(g["beam_width"]), int(g["eos"])
    ids, _, syms = TC.beam_search(P, c, mem, bw, eos)
    assert np.array_equal(ids.numpy(), g["beam_ids_plain"]) and np.array_equal(syms.numpy(), g["beam_syms_plain"])
    forced = O.det_tensor("beam_force", (c.max_seq_len, int(g["B"]) * bw, c.num_classes), int(g["seed_tcv"]), float(g["beam_force_scale"]))
    assert np.array_equal(TC.beam_search(P, c, mem, bw, eos, force_logits=forced)[0].numpy(), g["beam_ids_forced"])


@pytest.mark.parametrize("attn", [TC.attn_folded, TC.attn_literal], ids=["folded", "literal"])
def test_spec_attention_module_matches_reference_fixture(attn):
    g, c, _, P, _, _, _ = _fixture()
    pre, seed = "decoder.layer_stack.0.enc_attn.", int(g["seed_tcv"])
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items() if k.startswith(pre)}
    q = O.det_tensor("tcv_q", (1, 3, c.d_model), seed, 1.0).requires_grad_(True)
    m = O.det_tensor("tcv_mem", (1, 5, c.d_model), seed, 1.0).requires_grad_(True)
    out, amap = attn(Q, pre, c, q, m)
    (out * O.det_tensor("tcv_dout", (1, 3, c.d_model), seed, 1.0)).sum().backward()
    np.testing.assert_allclose(out.detach().numpy(), g["mod_out"], atol=2e-5)
    np.testing.assert_allclose(amap.detach().numpy(), g["mod_map"], atol=2e-6)
    grads = {**{k: v.grad for k, v in Q.items()}, "q_in": q.grad, "mem_in": m.grad}
    _check_grads(grads, g["mod_grad_names"].tolist(), g["mod_grad_norms"], g["mod_grad_samples"])


def test_spec_folded_equals_literal():
    """The fold is exact: in double precision the two forms agree to round-off in output, map and every gradient, at a shape with a key tail, and
    under dropout masks."""
    c = D.DecoderConfig(**{**D.TINY, "n_head": 3, "d_model": 192})
    pre = "decoder.layer_stack.1.enc_attn."
    base = {**D.det_decoder_state(c, 7), **TC.det_text_cond_state(c, 8)}
    q0, m0 = O.det_tensor("q", (2, 5, 192), 9, 1.0).double(), O.det_tensor("m", (2, 37, 192), 9, 1.0).double()
    keep = TC.keep_factor(3, 4, 1 << 30, 4.0 / 3.0, 2, 3, 5, 37).double()
    res = []
    for attn in (TC.attn_folded, TC.attn_literal):
        Q = {k: v.double().requires_grad_(True) for k, v in base.items() if k.startswith(pre)}
        q, m = q0.clone().requires_grad_(True), m0.clone().requires_grad_(True)
        out, amap = attn(Q, pre, c, q, m, keep)
        out.square().sum().backward()
        res.append([out.detach(), amap.detach(), q.grad, m.grad] + [Q[k].grad for k in sorted(Q)])
    for a, b in zip(*res):
        assert (a - b).abs().max().item() <= 1e-11 * (1.0 + b.abs().max().item())


def _tiny_kw(c, ecfg):
    return dict(embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads, n_layers=c.n_layers, d_model=c.d_model, n_head=c.n_head, d_k=c.d_k,
                d_inner=c.d_inner, nb_classes=c.num_classes, max_len=c.max_seq_len)


def test_model_keys_arena_and_optimizer_groups():
    """The flag adds the reference's eight tensors per layer behind enc_attn.fc.weight, in the reference's state_dict order; a reference state
    dict loads strictly; without the flag the keys do not exist; the new tensors follow the decay / layer-id rule of the other decoder tensors."""
    import types
    from dig_amd.recognizer import RecModel
    from dig_amd.finetune import RecModelTrain, LayerDecayValueAssigner, create_optimizer
    g, c, ecfg, P, _, _, _ = _fixture()
    m = RecModel(text_cond_vis=True, **_tiny_kw(c, ecfg))
    # the reference's names; its registration order within the 1-D / bias tensors and within the matrices (what decides the optimizer's
    # parameter indices: the two kinds never share a group), the new tensors behind enc_attn.fc.weight in its order
    keys, mine = g["state_keys"].tolist(), m.param_shapes()
    one_d = lambda k: len(mine[k]) == 1 or k.endswith(".bias")
    assert set(mine) == set(keys)
    assert [k for k in mine if one_d(k)] == [k for k in keys if one_d(k)] and [k for k in mine if not one_d(k)] == [k for k in keys if not one_d(k)]
    assert [k for k in mine if ".enc_attn." in k] == [k for k in keys if ".enc_attn." in k]
    m.load_state_dict(P, strict=True)
    sd = m.state_dict()
    assert all(torch.equal(sd[k], P[k]) for k in P)
    plain = RecModel(**_tiny_kw(c, ecfg))
    new = [k for k in m.param_shapes() if k not in plain.param_shapes()]
    assert new == list(TC.text_cond_shapes(c)) and list(plain.param_shapes()) == [k for k in m.param_shapes() if k not in new]
    with pytest.raises(KeyError):
        plain.load_state_dict(P, strict=True)
    with pytest.raises(KeyError):
        m.load_state_dict({k: v for k, v in P.items() if k not in new}, strict=True)
    for flag in (dict(insert_sem=True), dict(insert_sem=True, text_cond_vis=True)):
        with pytest.raises(NotImplementedError, match="insert_sem"):
            RecModel(types.SimpleNamespace(model="simmim_vit_small_patch4_32x128", decoder_name="tf_decoder", nb_classes=97, max_len=25, **flag))
    a = types.SimpleNamespace(model="simmim_vit_tiny_patch4_32x128", decoder_name="small_tf_decoder", nb_classes=97, max_len=25, text_cond_vis=True)
    assert RecModel(a).text_cond_vis and len(RecModel(a).param_shapes()) == len(RecModel(types.SimpleNamespace(**{**vars(a), "text_cond_vis": False})).param_shapes()) + 16
    t = RecModelTrain(text_cond_vis=True, **_tiny_kw(c, ecfg))
    assert set(t.state_dict()) == set(P)
    pre = "decoder.layer_stack.0.enc_attn."
    assert torch.equal(t.state_dict()[pre + "vis_norm.weight"], torch.ones(c.d_model)) and not t.state_dict()[pre + "vis_cond_norm.bias"].any()
    assert t.state_dict()[pre + "gamma_decode.weight"].abs().max().item() <= 1.0 / np.sqrt(c.d_model)
    nl = t.get_num_layers()
    asg = LayerDecayValueAssigner([0.75 ** (nl + 1 - i) for i in range(nl + 2)])
    opt = create_optimizer(types.SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None), t, get_num_layer=asg.get_layer_id,
                           get_layer_scale=asg.get_scale)
    group = {n: grp for grp in opt.param_groups for n in grp["names"]}
    for n in new:
        decay = n.endswith("gamma_decode.weight") or n.endswith("vis_proj.weight")
        assert group[n]["weight_decay"] == (0.05 if decay else 0.0) and group[n]["lr_scale"] == 1.0, n
    # the checkpoint layout: the reference's optimizer walks ITS registration order (optim_factory.get_parameter_groups): same indices
    want = {}
    for n in keys:
        lid = asg.get_layer_id(n[len("encoder."):] if n.startswith("encoder") else n)
        want.setdefault("layer_%d_%s" % (lid, "no_decay" if one_d(n) else "decay"), []).append(n)
    assert opt._ordered_names() == [n for names in want.values() for n in names]


# ---------------------------------------------------------------------------------------------- the model on the device
def _device_model(c, ecfg, P, decoder_dropout=0.0, **kw):
    from dig_amd.finetune import RecModelTrain
    m = RecModelTrain(text_cond_vis=True, decoder_dropout=decoder_dropout, **_tiny_kw(c, ecfg), **kw)
    m.load_state_dict(P)
    m.to("cuda:0")
    return m.train()


def _grad_gate(m, ref_g, bf_g):
    """Per tensor: 1 - cos and the norm ratio against the fp32 specification, at most twice the specification's own error under CPU bf16 autocast
    plus the fine-tune step's floors (5e-3, 3e-2); tensors below 1e-3 of the total gradient norm are skipped, as there."""
    grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters()}
    cos = torch.nn.functional.cosine_similarity
    names = [n for n in ref_g if n != "encoder.mask_token"]
    assert set(grads) == set(names)
    tot = float(np.sqrt(sum(ref_g[n].double().norm().item() ** 2 for n in names)))
    bad = []
    for n in names:
        r, nr = ref_g[n].reshape(1, -1), ref_g[n].norm().item()
        if nr < 1e-3 * tot:
            continue
        c_hip, c_bf = cos(grads[n].reshape(1, -1), r).item(), cos(bf_g[n].float().reshape(1, -1), r).item()
        q_hip, q_bf = grads[n].norm().item() / nr, bf_g[n].float().norm().item() / nr
        print(f"{n}: 1-cos {1 - c_hip:.2e} (bf16 {1 - c_bf:.2e}) norm ratio {q_hip:.4f} (bf16 {q_bf:.4f})")
        if (1 - c_hip) > 2 * (1 - c_bf) + 5e-3 or abs(q_hip - 1) > 2 * abs(q_bf - 1) + 3e-2:
            bad.append((n, c_hip, c_bf, q_hip, q_bf))
    assert not bad, bad


def _train_step_vs_spec(m, P, ecfg, c, images, targets, lens, dr=None, use_1d_attdec=False, ref=None):
    from dig_amd.finetune import SeqCrossEntropyLoss
    for p in m.parameters():
        p.grad.zero_()
    logits = m((images.to("cuda:0"), targets, lens))[0]
    loss = SeqCrossEntropyLoss()(logits, targets, lens)
    loss.backward()
    ref_loss, ref_g, ref_logits = TC.loss_and_grads(P, ecfg, c, images, targets, lens, dr, use_1d_attdec)
    if ref is not None:                                     # the reference's own numbers where the fixture holds them
        ref_loss, ref_logits = ref
    print(f"loss {loss.item():.5f} against {ref_loss:.5f}")
    assert abs(loss.item() - ref_loss) < 2e-2 * ref_loss
    assert ((logits.detach().cpu() - ref_logits).norm() / ref_logits.norm()).item() < 2e-2
    with torch.autocast("cpu", dtype=torch.bfloat16):
        _, bf_g, _ = TC.loss_and_grads(P, ecfg, c, images, targets, lens, dr, use_1d_attdec)
    _grad_gate(m, ref_g, bf_g)


@pytest.mark.gpu
def test_device_training_step_vs_reference_fixture():
    g, c, ecfg, P, images, targets, lens = _fixture()
    m = _device_model(c, ecfg, P)
    _train_step_vs_spec(m, P, ecfg, c, images, targets, lens, ref=(float(g["loss"]), torch.from_numpy(g["logits"])))


@pytest.mark.gpu
def test_device_training_step_1d_memory_vs_spec():
    """--use_1d_attdec: 32 memory rows per sample."""
    _, c, ecfg, P, images, targets, lens = _fixture()
    m = _device_model(c, ecfg, P, use_1d_attdec=True)
    assert m.n_mem == 32
    _train_step_vs_spec(m, P, ecfg, c, images, targets, lens, use_1d_attdec=True)


@pytest.mark.gpu
def test_device_training_step_with_decoder_dropout_vs_spec():
    """Decoder dropout 0.1 (the weights' mask inside dig_tcv_attn_fwd / _bwd, proj_drop behind fc) against the specification under the same keyed masks."""
    _, c, ecfg, P, images, targets, lens = _fixture()
    m = _device_model(c, ecfg, P, decoder_dropout=0.1, drop_seed=23)
    dr = FO.DropOracle(23, 0, depth=ecfg.depth, decoder_dropout=0.1)
    _train_step_vs_spec(m, P, ecfg, c, images, targets, lens, dr=dr)
    assert m.drop_step == 1
    plain = TC.forward_train(P, ecfg, c, images, targets, lens)
    dropped = TC.forward_train(P, ecfg, c, images, targets, lens, dr)
    assert ((plain - dropped).norm() / plain.norm()).item() > 0.05          # the masks matter


@pytest.mark.gpu
def test_device_greedy_and_beam_evaluation_vs_reference_fixture():
    """Greedy: teacher-forced probabilities within 3e-2 (row N4's tolerance) of the reference's, tokens equal wherever the reference's top-2 margin
    exceeds 6e-2, the last layer's head-mean weights as attention maps, the HIP-graph replay equal to the plain loop.  Beam search: the classifier
    outputs of every step with the reference's symbols fed back, and the reference's result with the forced classifier outputs."""
    g, c, ecfg, P, images, _, _ = _fixture()
    m = _device_model(c, ecfg, P).eval()
    dev = torch.device("cuda:0")
    m._prepare(dev)
    ref_p, ref_t = torch.from_numpy(g["greedy_probs"]), torch.from_numpy(g["greedy_tokens"])
    with torch.no_grad():
        mem = m.memory(m.encoder_features(images.to(dev)))
        probs, maps, toks = m.greedy_decode(mem, m.n_mem, force_tokens=ref_t.to(dev))
    err = (probs.cpu() - ref_p).abs().max().item()
    print(f"teacher-forced probabilities: max abs error {err:.3e}")
    assert err < 3e-2
    clear = torch.from_numpy(g["greedy_clear"])
    assert int(clear.sum()) == int(g["n_clear"]) and bool(toks.cpu().eq(ref_t)[clear].all())
    maps = maps.cpu()
    assert maps.shape == (int(g["B"]), c.max_seq_len, 256) and (maps.sum(-1) - 1).abs().max().item() < 1e-3
    got = np.stack([_samples(r) for r in maps.reshape(-1, 256)])
    assert np.abs(got - g["greedy_map_samples"]).max() <= 3e-2 * np.abs(g["greedy_map_samples"]).max() + 1e-3
    m.use_hip_graph = False
    p0, _, _, a0 = m((images.to(dev), None, None))
    m.use_hip_graph = True
    for _ in range(2):                                      # capture, then replay
        p1, _, _, a1 = m((images.to(dev), None, None))
        assert torch.equal(p0, p1) and torch.equal(a0, a1)
    bw, eos, T = int(g["beam_width"]), int(g["eos"]), c.max_seq_len
    syms = torch.from_numpy(g["beam_syms_plain"])
    mem32 = TC.memory_of(P, ecfg, c, images)
    _, want, _ = TC.beam_search(P, c, mem32, bw, eos, force_syms=syms)       # (== the reference's step outputs: asserted when the fixture is written)
    with torch.no_grad():
        _, lg = m.beam_search(mem, m.n_mem, bw, eos=eos, return_logits=True, force_tokens=syms.to(dev))
        err = ((lg.cpu().softmax(-1) - want.softmax(-1)).abs().max().item(), (lg.cpu() - want).abs().max().item() / want.abs().max().item())
        print(f"beam step outputs: probabilities off by {err[0]:.3e}, logits by {err[1]:.3e} of their largest")
        assert err[0] < 3e-2 and err[1] < 3e-2
        forced = O.det_tensor("beam_force", (T, int(g["B"]) * bw, c.num_classes), int(g["seed_tcv"]), float(g["beam_force_scale"]))
        ids = m.beam_search(mem, m.n_mem, bw, eos=eos, force_logits=forced.to(dev))
    assert np.array_equal(ids.cpu().numpy(), g["beam_ids_forced"])


@pytest.mark.gpu
def test_device_checkpoint_round_trip_and_eval_after_update(tmp_path):
    """save_model / auto_load_model is bit-exact for the model with the new tensors and its optimizer state, and an evaluation that follows an
    optimizer step reads the updated weights (equal to a fresh RecModel loaded from the state dict; different from before the step)."""
    import types
    from dig_amd.recognizer import RecModel
    from dig_amd.finetune import SeqCrossEntropyLoss, LayerDecayValueAssigner, create_optimizer
    from dig_amd.utils import NativeScalerWithGradNormCount, save_model, auto_load_model
    _, c, ecfg, P, images, targets, lens = _fixture()
    dev = "cuda:0"

    def make():
        m = _device_model(c, ecfg, P, decoder_dropout=0.1, drop_seed=5)
        nl = m.get_num_layers()
        asg = LayerDecayValueAssigner([0.75 ** (nl + 1 - i) for i in range(nl + 2)])
        args = types.SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, output_dir=str(tmp_path), resume="",
                                     auto_resume=True, start_epoch=0)
        opt = create_optimizer(args, m, get_num_layer=asg.get_layer_id, get_layer_scale=asg.get_scale)
        for grp in opt.param_groups:
            grp["lr"] = args.lr * grp["lr_scale"]
        return m, opt, args

    def step(m, opt):
        m.train()
        opt.zero_grad()
        loss = SeqCrossEntropyLoss()(m((images.to(dev), targets, lens))[0], targets, lens)
        NativeScalerWithGradNormCount()(loss, opt, clip_grad=1.0, parameters=None)
        return loss.item()

    m, opt, args = make()
    m.eval()
    before = m((images.to(dev), None, None))[0].clone()
    step(m, opt)
    m.eval()
    after = m((images.to(dev), None, None))[0].clone()
    fresh = RecModel(text_cond_vis=True, **_tiny_kw(c, ecfg)).eval()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(after, fresh((images.to(dev), None, None))[0]) and (after - before).abs().max().item() > 1e-3
    save_model(args, 0, m, m, opt, NativeScalerWithGradNormCount())
    l2 = step(m, opt)
    want, want_opt = m.state_dict(), opt.state_dict()
    m2, opt2, args2 = make()
    for _, p in m2.named_parameters():
        p.add_(1.0)
    auto_load_model(args2, m2, m2, opt2, NativeScalerWithGradNormCount())
    assert args2.start_epoch == 1 and m2.drop_step == 1 and opt2._step == 1
    assert step(m2, opt2) == l2
    got, got_opt = m2.state_dict(), opt2.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert all(torch.equal(got_opt["state"][i][k], want_opt["state"][i][k]) for i in want_opt["state"] for k in ("exp_avg", "exp_avg_sq"))
