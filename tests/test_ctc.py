"""The CTC recognition head (`--decoder_type ctc`): csrc/ctc.hip against torch's fp64 `ctc_loss` and a plain decode loop, the host-side
checks of its three entry points on both builds, `CTCRecModelTrain` against the reference's `CTCRecModel` (tests/golden/ctc_tiny.npz, written
by tools/gen_ctc_golden.py) and the driver.  Operator tests run on both builds (`abi_dev`); the specification is tests/ctc_model.py."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import ctc_model as S
import decode_oracle as D
import dig_oracle as O
import finetune_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = 128


# ---------------------------------------------------------------------------------------------- 1. loss and gradient against fp64
def _batch(T, C, labels, ldt, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(labels)
    x = torch.full((B, T, LD), float("nan"))
    x[:, :, :C] = 3 * torch.randn(B, T, C, generator=g)
    target = torch.full((B, ldt), C - 2, dtype=torch.int64)                 # (cells past a row's labels are never read as labels)
    for b, l in enumerate(labels):
        target[b, :len(l)] = torch.tensor(l, dtype=torch.int64)
    return x, target, torch.tensor([len(l) for l in labels], dtype=torch.int64)


CASES = {
    "T32": (32, 98, [[], [7], [5, 5], list(range(24)), [11] * 20, [3, 3, 4, 4, 3] + [9] * 10, list(range(40, 72)), [2] * 16 + [3]], 40),
    "T1": (1, 6, [[], [4], [4, 4]], 3),
    "T2": (2, 6, [[4, 4], [4, 5], [4]], 2),
    "T64": (64, 98, [list(range(63)), [], [1, 1, 2, 2] * 8, [6] * 40, list(range(90, 30, -1))], 63),
}
_REF = {}


def _reference(name):
    """fp64 and fp32 torch CTC on the CPU for a case, computed once: (x, target, n, nll64, g64, e32_nll, e32_g); g = d nll_b / d logits."""
    if name not in _REF:
        T, C, labels, ldt = CASES[name]
        x, target, n = _batch(T, C, labels, ldt, seed=len(name) + T)
        out = {}
        for dt in (torch.float64, torch.float32):
            nll, grad = S.ctc_nll_and_grad(x[:, :, :C].to(dt), target, n, blank=C - 1)
            out[dt] = (nll, grad)
        nll64, g64 = out[torch.float64]
        assert torch.isfinite(nll64).all() and torch.isfinite(g64).all()
        e_nll = float((out[torch.float32][0].double() - nll64).abs().max())
        e_g = float((out[torch.float32][1].double() - g64).abs().max())
        _REF[name] = (x, target, n, nll64, g64, e_nll, e_g)
    return _REF[name]


@pytest.mark.parametrize("len_offset", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_ctc_loss_and_gradient_against_fp64(abi_dev, name, len_offset):
    """Device figures (MI355X): DESIGN.md section 1, row N1 CTC head."""
    from dig_amd.ctc_recognizer import ctc_loss, ctc_loss_bwd
    T, C, labels, ldt = CASES[name]
    x, target, n, nll64, g64, e_nll, e_g = _reference(name)
    B, blank = len(labels), C - 1
    xd, td, ld_ = x.to(abi_dev), target.to(abi_dev), (n + len_offset).to(abi_dev)
    nll, loss = ctc_loss(xd, C, td, ld_, blank, len_offset)
    nll, loss = nll.cpu().double(), loss.cpu().double()
    err = (nll - nll64).abs()
    bound = 4 * e_nll + 2.0 ** -20 * nll64.abs()
    print(f"{name} len_offset {len_offset}: nll err {float(err.max()):.3e} (e32 {e_nll:.3e}, |nll| max {float(nll64.abs().max()):.1f})")
    assert (err <= bound).all(), (err, bound)
    want_loss = nll64.sum() / B
    assert abs(float(loss[0] - want_loss)) <= 4 * e_nll + 2.0 ** -20 * abs(float(want_loss))
    infeasible = [b for b, l in enumerate(labels) if len(l) + sum(l[i] == l[i - 1] for i in range(1, len(l))) > T]
    assert all(float(nll[b]) == 0.0 for b in infeasible) and (name == "T2" or infeasible)
    # ---- gradient, seeded with gscalar = B: the rows are d nll_b / d logits, entries bounded by 1
    gs = torch.full((1,), float(B), device=abi_dev)
    g32 = ctc_loss_bwd(xd, C, td, ld_, blank, len_offset, gscalar=gs, ldd=LD, f32=True)
    gerr = (g32[:, :, :C].cpu().double() - g64).abs()
    print(f"{name} len_offset {len_offset}: grad err {float(gerr.max()):.3e} (e32 {e_g:.3e})")
    assert float(gerr.max()) <= 4 * e_g + 1e-6
    assert all(float(g32[b].abs().max()) == 0.0 for b in infeasible)
    assert float(g32[:, :, C:].abs().max()) == 0.0                          # pad columns: zeros
    g16 = ctc_loss_bwd(xd, C, td, ld_, blank, len_offset, gscalar=gs, ldd=LD)
    assert g16.dtype == torch.bfloat16 and torch.equal(g16.view(torch.int16), g32.to(torch.bfloat16).view(torch.int16))
    again = ctc_loss_bwd(xd, C, td, ld_, blank, len_offset, gscalar=gs, ldd=LD, f32=True)
    assert torch.equal(again, g32) and torch.equal(ctc_loss(xd, C, td, ld_, blank, len_offset)[0].cpu().double(), nll)
    twice = ctc_loss_bwd(xd, C, td, ld_, blank, len_offset, gscalar=2 * gs, ldd=LD, f32=True)
    assert torch.equal(twice, 2 * g32)
    narrow = ctc_loss_bwd(xd, C, td, ld_, blank, len_offset, gscalar=gs, f32=True)           # ldd = C
    assert torch.equal(narrow, g32[:, :, :C])


def test_ctc_invalid_labels_give_zero_loss_and_gradient(abi_dev):
    """A label in [C, ld) or equal to the blank (values that keep even an unguarded read inside the row's own padding); a negative label on
    the CPU build only.  The other rows are untouched by their neighbour's labels."""
    from dig_amd.ctc_recognizer import ctc_loss, ctc_loss_bwd
    T, C, labels, ldt = CASES["T32"]
    x, target, n, nll64, g64, e_nll, e_g = _reference("T32")
    blank = C - 1
    bad = {1: C + 5, 3: blank, 5: LD - 1}
    if abi_dev.type == "cpu":
        bad[7] = -3
    t2 = target.clone()
    for b, v in bad.items():
        t2[b, len(labels[b]) // 2] = v
    xd, td, ld_ = x.to(abi_dev), t2.to(abi_dev), (n + 1).to(abi_dev)
    nll, loss = ctc_loss(xd, C, td, ld_, blank, 1)
    gs = torch.full((1,), float(len(labels)), device=abi_dev)
    g = ctc_loss_bwd(xd, C, td, ld_, blank, 1, gscalar=gs, ldd=LD, f32=True).cpu().double()
    nll = nll.cpu().double()
    for b in range(len(labels)):
        if b in bad:
            assert float(nll[b]) == 0.0 and float(g[b].abs().max()) == 0.0, b
        else:
            assert abs(float(nll[b] - nll64[b])) <= 4 * e_nll + 2.0 ** -20 * abs(float(nll64[b])), b
            assert float((g[b, :, :C] - g64[b]).abs().max()) <= 4 * e_g + 1e-6, b
    assert abs(float(loss[0]) - float(nll.sum()) / len(labels)) <= 1e-5 * float(nll.sum())


# ---------------------------------------------------------------------------------------------- 2. greedy decode, exact
def _logits_with_argmax(frames, C, seed, ties=False):
    """fp32 [B, T, LD] with the wanted arg-max per frame and distinct values; ties: the maximum is repeated at a HIGHER id as well."""
    g = torch.Generator().manual_seed(seed)
    B, T = frames.shape
    x = torch.full((B, T, LD), float("nan"))
    vals = torch.rand(B, T, C, generator=g).sort(dim=-1).values * 4 - 6 + torch.arange(C) * 1e-3      # distinct, all below -1
    x[:, :, :C] = vals.gather(2, torch.rand(B, T, C, generator=g).argsort(-1))
    top = 1.0 + torch.rand(B, T, generator=g)
    x[:, :, :C].scatter_(2, frames.unsqueeze(-1), top.unsqueeze(-1))
    if ties:
        for b in range(B):
            for t in range(T):
                c = int(frames[b, t])
                if c + 1 < C and (b + t) % 3 == 0:
                    x[b, t, c + 1 + (b + t) % (C - c - 1)] = top[b, t]
    return x


@pytest.mark.parametrize("B", [1, 63, 65])
def test_ctc_greedy_decode_is_exact(abi_dev, golden_dir, B):
    from dig_amd import evaluation_metric as EM
    from dig_amd.ctc_recognizer import ctc_greedy_decode
    z = np.load(os.path.join(golden_dir, "ctc_tiny.npz"), allow_pickle=False)
    voc = [str(v) for v in z["voc"]]
    C, blank, eos, pad = len(voc) + 1, len(voc), voc.index("EOS"), voc.index("PADDING")
    hand = torch.from_numpy(z["hand_frames"]).long()                         # [6, 32]: runs, repeats, EOS inside, UNKNOWN, all blank, 32 distinct
    g = torch.Generator().manual_seed(B)
    rnd = torch.randint(0, C, (max(B - 6, 0), 32), generator=g)
    rnd[torch.rand(rnd.shape, generator=g) < 0.4] = blank
    rnd[:, 1::2] = torch.where(torch.rand(rnd[:, 1::2].shape, generator=g) < 0.5, rnd[:, 0::2], rnd[:, 1::2])   # runs
    frames = torch.cat([hand, rnd])[:B]
    x = _logits_with_argmax(frames, C, seed=3 + B, ties=True)
    ids, score, n = ctc_greedy_decode(x.to(abi_dev), C, blank, eos, pad)
    want_ids, want_score, want_n = S.greedy_decode(x[:, :, :C], blank, eos, pad)
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(n.cpu().long(), want_n)
    assert float((score.cpu() - want_score).abs().max()) <= 1e-6
    assert torch.equal((x[:, :, :C] == x[:, :, :C].max(-1, keepdim=True).values).float().argmax(-1), frames)   # (the lowest id of every tie is the wanted class)
    assert int((x[:, :, :C] == x[:, :, :C].max(-1, keepdim=True).values).sum()) > frames.numel()
    # ---- strings and accuracies: the fixture's for the hand-made rows, Accuracy on the decoded rows = CTCAccuracy on the frames
    ds = type("D", (), {"voc": voc})()
    targets = torch.from_numpy(z["hand_targets"]).long()
    k = min(B, 6)
    pred, targ = EM.ctc_get_str_list(frames[:k].to(abi_dev), targets[:k].to(abi_dev), ds)
    assert pred == [str(s) for s in z["hand_pred_strings"]][:k] and targ == [str(s) for s in z["hand_targ_strings"]][:k]
    if B >= 6:
        assert EM.CTCAccuracy(frames[:6].to(abi_dev), targets.to(abi_dev), ds) == float(z["hand_ctc_accuracy"])
        from dig_amd.ctc_recognizer import match_widths
        p, t = match_widths(ids[:6], targets.to(abi_dev), pad)
        assert EM.Accuracy(p, t, ds) == float(np.float32(z["hand_ctc_accuracy"]))      # (Accuracy is a float32 mean on the device)


# ---------------------------------------------------------------------------------------------- 3. host-side validation (no GPU)
def _raw(lib_path):
    from dig_amd import _lib as L
    lib = ctypes.CDLL(lib_path)
    for name in ("dig_ctc_loss", "dig_ctc_loss_bwd", "dig_ctc_greedy_decode"):
        f = getattr(lib, name)
        f.restype, f.argtypes = ctypes.c_int, L._prototypes()[name]
    return lib


@pytest.mark.parametrize("build", ["hip", "cpu_abi"])
def test_ctc_entry_points_validate_on_the_host(build):
    """Every error code of the three entry points, before any launch: both builds run these checks on a machine without a GPU.  A refused call
    writes nothing."""
    from cpu_abi_util import build as build_cpu
    from dig_amd import _lib as L
    lib = _raw(L.LIB_PATH if build == "hip" else build_cpu())
    ARG, UNS, OK = L.const("DIG_ERR_ARG"), L.const("DIG_ERR_UNSUPPORTED"), L.const("DIG_OK")
    poison = 0x5A
    bufs = {k: (ctypes.c_ubyte * 4096)(*([poison] * 4096)) for k in ("x", "t", "l", "g", "nll", "loss", "d", "ids", "score", "n")}
    p = {k: ctypes.cast(v, ctypes.c_void_p) for k, v in bufs.items()}

    def loss(**kw):
        a = dict(x=p["x"], ld=128, t=p["t"], ldt=25, l=p["l"], off=1, B=4, T=32, C=98, blank=97, nll=p["nll"], loss=p["loss"])
        a.update(kw)
        return lib.dig_ctc_loss(a["x"], a["ld"], a["t"], a["ldt"], a["l"], a["off"], a["B"], a["T"], a["C"], a["blank"], a["nll"], a["loss"], None)

    def bwd(**kw):
        a = dict(x=p["x"], ld=128, t=p["t"], ldt=25, l=p["l"], off=1, g=p["g"], B=4, T=32, C=98, blank=97, d=p["d"], ldd=128, f32=0)
        a.update(kw)
        return lib.dig_ctc_loss_bwd(a["x"], a["ld"], a["t"], a["ldt"], a["l"], a["off"], a["g"], a["B"], a["T"], a["C"], a["blank"], a["d"], a["ldd"],
                                    a["f32"], None)

    def dec(**kw):
        a = dict(x=p["x"], ld=128, B=4, T=32, C=98, blank=97, eos=94, pad=95, ids=p["ids"], score=p["score"], n=p["n"])
        a.update(kw)
        return lib.dig_ctc_greedy_decode(a["x"], a["ld"], a["B"], a["T"], a["C"], a["blank"], a["eos"], a["pad"], a["ids"], a["score"], a["n"], None)

    for fn, ptrs in ((loss, ("x", "t", "l", "nll", "loss")), (bwd, ("x", "t", "l", "d")), (dec, ("x", "ids", "score", "n"))):
        for k in ptrs:
            assert fn(**{k: None}) == ARG, (fn.__name__, k)
        for kw in ({"B": -1}, {"T": 0}, {"T": -3}, {"C": 0}, {"C": -1}, {"ld": 97}, {"ld": 0}):
            assert fn(**kw) == ARG, (fn.__name__, kw)
        for kw in ({"T": 65}, {"C": 257, "ld": 257, "ldd": 257}, {"C": 1, "blank": 0, "ld": 1, "ldd": 1}):
            assert fn(**kw) == UNS, (fn.__name__, kw)
        assert fn(B=0) == OK and fn(B=0, T=64, C=256, ld=256, ldd=256, blank=255) == OK
    for fn in (loss, bwd):
        for kw in ({"ldt": 0}, {"ldt": -1}, {"blank": 98}, {"blank": -1}):
            assert fn(**kw) == ARG, (fn.__name__, kw)
        assert fn(ldt=64) == UNS and fn(ldt=63, B=0) == OK
    assert bwd(ldd=97) == ARG and bwd(g=None, B=0) == OK                      # (gscalar is optional: null = 1)
    assert all(all(v == poison for v in b) for b in bufs.values())


# ---------------------------------------------------------------------------------------------- the specification against the fixture (CPU)
def _sample_index(numel, k=8):
    if numel <= k:
        return np.arange(numel)
    return (np.arange(k, dtype=np.int64) * 2654435761 + 12345) % numel


_FIX = {}


def _fixture(golden_dir):
    if not _FIX:
        z = np.load(os.path.join(golden_dir, "ctc_tiny.npz"), allow_pickle=False)
        ecfg = O.DiGConfig(**O.TINY)
        P = S.state(ecfg, int(z["nb_classes"]), int(z["seed_enc"]), int(z["seed_head"]))
        images = O.synthetic_batch(int(z["B"]), ecfg, int(z["batch_seed"]))[0]
        _FIX.update(z=z, ecfg=ecfg, P=P, images=images, targets=torch.from_numpy(z["targets"]), lens=torch.from_numpy(z["lens"]),
                    voc=[str(v) for v in z["voc"]])
    return _FIX


def _scaled(P, scale):
    Q = dict(P)
    Q["ctc_classifier.3.weight"], Q["ctc_classifier.3.bias"] = P["ctc_classifier.3.weight"] * scale, P["ctc_classifier.3.bias"] * scale
    return Q


def test_specification_equals_the_reference_fixture(golden_dir):
    """tests/ctc_model.py against what tools/gen_ctc_golden.py recorded of the unmodified reference: the state (names, shapes, norms, samples), the
    logits, the fp64 loss and gradients, the evaluation frames and strings, the hand-made rows."""
    f = _fixture(golden_dir)
    z, P, ecfg, images, targets, lens, voc = f["z"], f["P"], f["ecfg"], f["images"], f["targets"], f["lens"], f["voc"]
    blank = len(voc)
    assert list(P) == z["state_names"].tolist()
    for i, (k, v) in enumerate(P.items()):
        assert list(v.shape) == [d for d in z["state_shapes"][i] if d] and abs(v.double().norm().item() - z["state_norms"][i]) <= 1e-12 * z["state_norms"][i], k
        assert np.array_equal(np.resize(v.reshape(-1)[_sample_index(v.numel())].numpy(), 8), z["state_samples"][i]), k
    np.testing.assert_allclose(S.logits(P, ecfg, images).numpy(), z["logits"], atol=3e-5)
    P64 = {k: v.double() for k, v in P.items()}
    loss, grads, lg = S.loss_and_grads(P64, ecfg, images.double(), targets, lens, blank)
    assert abs(loss - float(z["loss"])) <= 1e-9 * float(z["loss"])
    np.testing.assert_allclose(S.ctc_nll(lg, targets, lens - 1, blank).numpy(), z["nll"], rtol=1e-9)
    for i, n in enumerate(z["grad_names"].tolist()):
        assert abs(grads[n].norm().item() - z["grad_norms"][i]) <= 1e-7 * z["grad_norms"][i] + 1e-300, n
        got = np.resize(grads[n].reshape(-1)[_sample_index(grads[n].numel())].numpy(), 8)
        np.testing.assert_allclose(got, z["grad_samples"][i], rtol=1e-6, atol=1e-9 * z["grad_norms"][i])
    ev = S.logits(_scaled(P, float(z["cls_scale"])), ecfg, images)
    np.testing.assert_allclose(ev.numpy(), z["eval_logits"], atol=3e-5 * float(z["cls_scale"]))
    clear = torch.from_numpy(z["eval_clear"])
    assert int((~clear).sum()) * 8 <= clear.numel()
    frames = torch.from_numpy(z["eval_frames"])
    assert torch.equal(ev.argmax(-1)[clear], frames[clear])
    assert S.frames_to_strings(frames, voc, blank) == [str(s) for s in z["eval_pred_strings"]]
    hand = torch.from_numpy(z["hand_frames"])
    assert S.frames_to_strings(hand, voc, blank) == [str(s) for s in z["hand_pred_strings"]]
    # the decode loop on one-hot logits gives the same strings through the vocabulary
    ids, _, n = S.greedy_decode(torch.nn.functional.one_hot(hand, blank + 1).float(), blank, voc.index("EOS"), voc.index("PADDING"))
    assert [D.str_list(ids[b:b + 1], voc)[0] for b in range(6)] == [str(s) for s in z["hand_pred_strings"]]


# ---------------------------------------------------------------------------------------------- 4. the model against the fixture (gpu)
def _device_model(f, P=None):
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    ecfg = f["ecfg"]
    m = CTCRecModelTrain(embed_dim=ecfg.embed_dim, depth=ecfg.depth, num_heads=ecfg.heads, nb_classes=int(f["z"]["nb_classes"]),
                         max_len=int(f["z"]["max_len"]))
    m.load_state_dict(f["P"] if P is None else P)
    m.to("cuda:0")
    return m


def test_ctc_model_state_dict_is_the_reference_s(golden_dir):
    """Keys, order and shapes: the tiny model of the fixture and the three full-size encoders (the aliases `patch_embed.*` that the reference's
    class registers beside `encoder.patch_embed.*` are the same tensors under a second name)."""
    import types
    from dig_amd.ctc_recognizer import CTCRecModelTrain
    f = _fixture(golden_dir)
    z = f["z"]
    models = {"tiny": CTCRecModelTrain(embed_dim=f["ecfg"].embed_dim, depth=f["ecfg"].depth, num_heads=f["ecfg"].heads, nb_classes=int(z["nb_classes"]),
                                       max_len=int(z["max_len"]))}
    for enc in ("simmim_vit_tiny_patch4_32x128", "simmim_vit_small_patch4_32x128", "simmim_vit_base_patch4_32x128"):
        models[enc] = CTCRecModelTrain(types.SimpleNamespace(model=enc, nb_classes=97, max_len=25, drop=0.0, attn_drop_rate=0.0, drop_path=0.0))
    for name, m in models.items():
        keys, shapes = z["keys/" + name].tolist(), z["shapes/" + name]
        want = [(k, tuple(int(d) for d in s if d)) for k, s in zip(keys, shapes) if not k.startswith("patch_embed.")]
        assert len(want) < len(keys)
        sd = m.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == want, name
        assert m.no_weight_decay() == {"encoder.pos_embed", "encoder.cls_token"} and m.get_num_layers() == m.depth
        assert m.blank == m.nb_classes and m.is_ctc
        head = {k: v for k, v in sd.items() if k.startswith("ctc_classifier.")}
        assert list(head) == ["ctc_classifier.%d.%s" % (i, p) for i in (0, 1, 3) for p in ("weight", "bias")]
        assert float(head["ctc_classifier.1.weight"].min()) == 1.0 and float(head["ctc_classifier.1.bias"].abs().max()) == 0.0   # PyTorch defaults
        for i in (0, 3):
            bound = 1.0 / math.sqrt(head[f"ctc_classifier.{i}.weight"].shape[1])
            assert 0.9 * bound < float(head[f"ctc_classifier.{i}.weight"].abs().max()) <= bound
            assert 0.0 < float(head[f"ctc_classifier.{i}.bias"].abs().max()) <= bound


@pytest.mark.gpu
def test_ctc_model_step_vs_reference_fixture(golden_dir):
    """Forward, SeqCTCLoss, the hand-written backward and the layer-decay AdamW step of CTCRecModelTrain against the fixture (bf16 kernels: the
    specification under CPU bf16 autocast is the noise yardstick of the gradients), and the decoded frames of the evaluation forward."""
    import types
    from dig_amd.ctc_recognizer import SeqCTCLoss
    from dig_amd.finetune import LayerDecayValueAssigner, create_optimizer
    f = _fixture(golden_dir)
    z, P, ecfg, images, targets, lens, voc = f["z"], f["P"], f["ecfg"], f["images"], f["targets"], f["lens"], f["voc"]
    blank = len(voc)
    m = _device_model(f).train()
    nl, ld, lr, wd = m.get_num_layers(), 0.75, 1e-3, 0.05
    assigner = LayerDecayValueAssigner([ld ** (nl + 1 - i) for i in range(nl + 2)])
    args = types.SimpleNamespace(opt="adamw", lr=lr, weight_decay=wd, opt_eps=1e-8, opt_betas=None)
    opt = create_optimizer(args, m, get_num_layer=assigner.get_layer_id, get_layer_scale=assigner.get_scale, skip_list=m.no_weight_decay())
    for grp in opt.param_groups:
        grp["lr"] = lr * grp["lr_scale"]
    opt.zero_grad()
    out = m((images.to("cuda:0"), targets, lens))
    logits = out[0]
    assert out[1:] == (None, None, None) and tuple(logits.shape) == (4, 32, blank + 1) and logits.dtype == torch.float32
    loss = SeqCTCLoss(blank)(logits, targets, lens)
    loss.backward()
    ref_logits = torch.from_numpy(z["logits"])
    rel = ((logits.detach().cpu() - ref_logits).norm() / ref_logits.norm()).item()
    print(f"logits rel {rel:.3e}, loss {loss.item():.5f} (fixture {float(z['loss']):.5f})")
    assert rel < 2e-2
    assert abs(loss.item() - float(z["loss"])) < 2e-2 * float(z["loss"])
    _, ref_g, _ = S.loss_and_grads(P, ecfg, images, targets, lens, blank)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        _, bf_g, _ = S.loss_and_grads(P, ecfg, images, targets, lens, blank)
    grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters()}
    cos = torch.nn.functional.cosine_similarity
    names, norms = z["grad_names"].tolist(), z["grad_norms"]
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
    assert not bad, bad
    # AdamW with layer decay on the reference's own gradients -> the parameters after the step
    Pn = {k: v.clone() for k, v in P.items()}
    FO.adamw_step(Pn, ref_g, {}, 1, lr, FO.param_groups(Pn, nl, ld, wd))
    for n, p in m.named_parameters():
        p.grad.copy_(ref_g[n].to("cuda:0"))
    opt.step()
    sd = m.state_dict()
    for n in names:
        assert abs(sd[n].double().norm().item() - Pn[n].double().norm().item()) <= 2e-5 * Pn[n].double().norm().item() + 1e-6, n
        assert (sd[n] - Pn[n]).abs().max().item() <= 1e-5 * Pn[n].abs().max().item() + 1e-7, n
    assert torch.equal(sd["encoder.mask_token"], P["encoder.mask_token"])
    # ---- evaluation: the no-dropout walk, the head scaled as the fixture's evaluation was
    e = _device_model(f, _scaled(P, float(z["cls_scale"]))).eval()
    ev, a, b, c = e((images.to("cuda:0"), None, None))
    assert (a, b, c) == (None, None, None) and not ev.requires_grad and tuple(ev.shape) == (4, 32, blank + 1)
    ref_ev = torch.from_numpy(z["eval_logits"])
    assert ((ev.cpu() - ref_ev).norm() / ref_ev.norm()).item() < 2e-2
    clear, frames = torch.from_numpy(z["eval_clear"]), torch.from_numpy(z["eval_frames"])
    assert torch.equal(ev.argmax(-1).cpu()[clear], frames[clear])
    ids, score, n = e.decode(ev)
    want_ids, want_score, want_n = S.greedy_decode(ev.cpu(), blank, e.eos, e.padding)
    assert tuple(ids.shape) == (4, 33) and torch.equal(ids.cpu(), want_ids) and torch.equal(n.cpu().long(), want_n)
    assert float((score.cpu() - want_score).abs().max()) <= 1e-6
    if bool(clear.all(1).any()):                                               # a sample without an unclear frame decodes to the reference's string
        from dig_amd import evaluation_metric as EM
        text, tl = EM.tokens_to_text(ids, voc)
        for b_ in torch.nonzero(clear.all(1)).reshape(-1).tolist():
            assert "".join(chr(v) for v in text[b_, :int(tl[b_])].tolist()) == str(z["eval_pred_strings"][b_])


@pytest.mark.gpu
def test_ctc_model_through_the_engine_loops(golden_dir):
    """train_one_epoch (4 micro-batches, update_freq 2) and evaluate with a CTC model: the loop's training loss against the specification running
    the same two optimizer steps, the class accuracy from the decoded rows, and evaluate's meters against the specification's evaluation."""
    import types
    from dig_amd.ctc_recognizer import SeqCTCLoss
    from dig_amd.engine_for_finetuning import evaluate, train_one_epoch
    from dig_amd.finetune import LayerDecayValueAssigner, create_optimizer
    from dig_amd.utils import NativeScalerWithGradNormCount
    f = _fixture(golden_dir)
    P, ecfg, voc = f["P"], f["ecfg"], f["voc"]
    blank, max_len = len(voc), int(f["z"]["max_len"])
    m = _device_model(f).train()
    nl, ld, lr, wd = m.get_num_layers(), 0.75, 1e-3, 0.05
    assigner = LayerDecayValueAssigner([ld ** (nl + 1 - i) for i in range(nl + 2)])
    args = types.SimpleNamespace(opt="adamw", lr=lr, weight_decay=wd, opt_eps=1e-8, opt_betas=None, eval_freq=1000, eval_edit_distance=True, beam_width=0)
    opt = create_optimizer(args, m, get_num_layer=assigner.get_layer_id, get_layer_scale=assigner.get_scale, skip_list=m.no_weight_decay())
    rng = np.random.RandomState(5)
    batches = []
    for i in range(4):
        B = 5
        lens = torch.from_numpy(rng.randint(1, max_len + 1, size=B))
        tg = torch.from_numpy(rng.randint(0, voc.index("EOS"), size=(B, max_len)))
        for b in range(B):
            tg[b, int(lens[b]) - 1] = voc.index("EOS")
            tg[b, int(lens[b]):] = voc.index("PADDING")
        batches.append((O.synthetic_batch(B, ecfg, 900 + i)[0], tg, lens))
    loader = type("Ldr", (list,), {})(batches)
    loader.dataset = types.SimpleNamespace(idx_to_class={i: ch for i, ch in enumerate(voc)})
    stats = train_one_epoch(m, SeqCTCLoss(blank), loader, opt, torch.device("cuda:0"), 0, NativeScalerWithGradNormCount(), None, None, None,
                            None, start_steps=0, lr_schedule_values=np.array([lr, 0.5 * lr]), wd_schedule_values=np.array([wd, wd]),
                            num_training_steps_per_epoch=2, update_freq=2, args=args)
    Pn = {k: v.clone() for k, v in P.items()}
    state, losses = {}, []
    groups = FO.param_groups(Pn, nl, ld, wd)
    for s in range(2):
        acc_g = None
        for mb in batches[2 * s:2 * s + 2]:
            l, gr, _ = S.loss_and_grads(Pn, ecfg, *mb, blank)
            losses.append(l)
            acc_g = gr if acc_g is None else {k: acc_g[k] + gr[k] for k in gr}
        FO.adamw_step(Pn, {k: v / 2 for k, v in acc_g.items()}, state, s + 1, [lr, 0.5 * lr][s], groups)
    print("loop loss", stats["loss"], "specification", losses)
    assert abs(stats["loss"] - np.mean(losses)) < 3e-2 * np.mean(losses), (stats["loss"], losses)
    assert 0.0 <= stats["class_acc"] <= 1.0 and opt._step == 2
    test = evaluate(loader, m, torch.device("cuda:0"), args=args)
    assert set(test) == {"loss", "acc", "recognition_fmeasure", "edit_distance"} and all(math.isfinite(v) for v in test.values())
    with torch.no_grad():
        want = [S.loss(S.logits(Pn, ecfg, mb[0]), mb[1], mb[2], blank).item() for mb in batches]
    assert abs(test["loss"] - np.mean(want)) < 3e-2 * np.mean(want), (test["loss"], want)
    assert 0.0 <= test["acc"] <= 1.0 and test["edit_distance"] >= 0.0


# ---------------------------------------------------------------------------------------------- 5. the driver
from test_finetune_driver import COMMON, _driver, _load  # noqa: E402

CTC = COMMON.replace("--smoothing 0.", "--smoothing 0.1") + " --decoder_type ctc"


def test_driver_refuses_what_the_ctc_head_has_not():
    drv = _driver()
    for flags, words in (("--beam_width 5", "decodes greedily"), ("--text_cond_vis", "belongs to the transformer decoder"),
                         ("--use_1d_attdec", "always classifies the 32 column means")):
        with pytest.raises(SystemExit, match=words):
            drv.get_args((CTC + " " + flags).split())
    with pytest.raises(SystemExit, match="tf_decoder, attention or ctc"):
        drv.get_args((COMMON + " --decoder_type rnn").split())
    args = drv.get_args(CTC.split())
    assert args.decoder_type == "ctc" and args.smoothing == 0.1
    for flags in ("--beam_width 5", "--text_cond_vis", "--use_1d_attdec"):        # ... and the other heads still take them
        assert drv.get_args((COMMON + " " + flags).split()).decoder_type == "tf_decoder"


@pytest.fixture(scope="module")
def ctc_run(tmp_path_factory):
    """Two epochs straight through (shared, read-only)."""
    import contextlib
    import io
    drv = _driver()
    out = str(tmp_path_factory.mktemp("ctc_straight"))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = drv.main(drv.get_args((CTC + " --save_ckpt --output_dir " + out).split()))
    return out, res, buf.getvalue()


@pytest.mark.gpu
def test_ctc_driver_trains_resumes_and_evaluates(ctc_run, tmp_path, monkeypatch):
    """--decoder_type ctc end to end: the criterion is SeqCTCLoss whatever --smoothing says (said once), an interrupted run resumes to the same
    checkpoint bit for bit, and --eval reproduces the logged metrics."""
    import dig_amd.engine_for_finetuning as E
    out_a, res, printed = ctc_run
    assert printed.count("is ignored with --decoder_type ctc") == 1 and "criterion = SeqCTCLoss(" in printed and "Model = CTCRecModelTrain" in printed
    assert math.isfinite(res["train_stats"]["loss"]) and math.isfinite(res["test_stats"]["loss"]) and res["test_stats"]["loss"] > 0
    ck = _load(os.path.join(out_a, "checkpoint-1.pth"))
    assert [k for k in ck["model"] if not k.startswith("encoder.")] == ["ctc_classifier.%d.%s" % (i, p) for i in (0, 1, 3) for p in ("weight", "bias")]
    assert tuple(ck["model"]["ctc_classifier.3.weight"].shape) == (98, 512)
    drv = _driver()
    argv = (CTC + " --save_ckpt --auto_resume --output_dir " + str(tmp_path)).split()
    real = E.train_one_epoch

    class Interrupted(Exception):
        pass

    def one_epoch_only(model, criterion, data_loader, optimizer, device, epoch, *a, **k):
        if epoch == 1:
            raise Interrupted
        return real(model, criterion, data_loader, optimizer, device, epoch, *a, **k)
    monkeypatch.setattr(E, "train_one_epoch", one_epoch_only)
    with pytest.raises(Interrupted):
        drv.main(drv.get_args(argv))
    monkeypatch.setattr(E, "train_one_epoch", real)
    args = drv.get_args(argv)
    drv.main(args)
    assert args.start_epoch == 1
    a, b = ck, _load(str(tmp_path / "checkpoint-1.pth"))
    assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"]), [k for k in a["model"] if not torch.equal(a["model"][k], b["model"][k])][:5]
    sa, sb = a["optimizer"]["state"], b["optimizer"]["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    assert all(torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"]) for i in sa)
    last = [json.loads(l) for l in open(os.path.join(out_a, "log.txt"))][-1]
    lines = [json.loads(l) for l in (tmp_path / "log.txt").read_text().splitlines()]
    assert {k: v for k, v in lines[-1].items() if k.startswith("test_")} == {k: v for k, v in last.items() if k.startswith("test_")}
    got = drv.main(drv.get_args((CTC + " --eval --resume " + os.path.join(out_a, "checkpoint-1.pth")).split()))
    assert set(got["test_stats"]) == {"loss", "acc", "recognition_fmeasure", "edit_distance"}
    for k in ("acc", "loss", "recognition_fmeasure", "edit_distance"):
        assert got["test_stats"][k] == last["test_" + k] == res["test_stats"][k], k
