"""ABINet augmentation of fine-tuning (dig_amd/augment.py AbiAugment, dig_amd/csrc/abiaug.hip): the sampler's tables and distributions, the
warped canvas sizes against the reference's formulas, every stage against the numpy model (tests/abiaug_model.py), the tail against Pillow
(tests/golden/abi_aug_tail.npz, tools/gen_abi_aug_golden.py), the identity table, argument checks, FinetuneBatchTransform's branches and a
short fine-tune run.  Operator tests run through the HIP library on the MI355X and the plain-C++ build in the GPU-less container (`abi_dev`).

Exactness: the resamplers are integer arithmetic on float32 source coordinates, the blur a float32 sum, the noise double arithmetic, all
without contraction in both builds -- bit-exact on `cpu_abi`.  On `hip` the warp and the rescale are held to the key view's allowance
(|diff| <= 1 on <= 0.1 % of the bytes): a float32 coordinate that lands on a rounding boundary of the 1/32 grid after a divide; none is
expected, as keyview.hip's resamplers show."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import abiaug_model as M
import input_oracle as IO
from dig_amd import _lib as L
from dig_amd.augment import (ABI_PARAMS_DTYPE, ABI_RUN_DTYPE, AbiAugment, KeyViewAugment, PackedCrops, abi_params_from_numpy,
                             abi_params_to_numpy, draw_abi_run, pack_crops)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "abi_aug_tail.npz")


def _sizes_packed(hs, ws, dev):
    h = torch.tensor(hs, dtype=torch.int32, device=dev)
    w = torch.tensor(ws, dtype=torch.int32, device=dev)
    return PackedCrops(torch.zeros(1, dtype=torch.uint8, device=dev), None, h, w, len(hs), int(max(hs)), int(max(ws)))


def _run(geom_type=0, noise_var=5, mb_size=3, mb_angle=30.0, factor=2, order=(0, 1, 2)):
    r = np.zeros((), ABI_RUN_DTYPE)
    r["geom_type"], r["noise_var"], r["mb_size"], r["mb_angle"], r["rescale_factor"], r["det_order"] = (geom_type, noise_var, mb_size,
                                                                                                        mb_angle, factor, order)
    return r


def _sample(dev, hs, ws, run, seed=7, step=0):
    aug = AbiAugment(seed, dev)
    aug.run = run
    params, info = aug.sample(_sizes_packed(hs, ws, dev), step=step)
    return abi_params_to_numpy(params), info.cpu().numpy()


def _crops(rng, n, hmax=14, wmax=40):
    return [rng.randint(0, 256, size=(rng.randint(2, hmax), rng.randint(2, wmax), 3)).astype(np.uint8) for _ in range(n)]


def _stages(dev, crops, tables, run):
    """warp + deteriorate through the library with the given tables -> (final images, tail output)."""
    aug = AbiAugment(0, dev)
    aug.run = run
    packed = pack_crops(crops, dev)
    tables = tables.copy()
    total = M.layout(tables, run)
    params = abi_params_from_numpy(tables, dev)
    mh, mw = int(max(tables["wh"].max(), packed.max_h)), int(max(tables["ww"].max(), packed.max_w))
    work = torch.zeros(max(total, 0), dtype=torch.uint8, device=dev)
    aug.warp(packed, params, work, mh, mw)
    aug.deteriorate(packed, params, work, mh, mw)
    out = aug.tail(packed, params, work, mh, mw).cpu().numpy()
    w = work.cpu().numpy()
    finals = []
    for P, c in zip(tables, crops):
        if P["final_buf"] == 0:
            finals.append(c)
        else:
            rb = M.round256(3 * int(P["wh"]) * int(P["ww"]))
            o = int(P["ws_off"]) + (rb if P["final_buf"] == 2 else 0)
            finals.append(w[o:o + 3 * int(P["wh"]) * int(P["ww"])].reshape(int(P["wh"]), int(P["ww"]), 3))
    return finals, out, tables


def _gate(t, run, geom):
    """Set the geometry gates of tables t to `geom` (0 / 1 per image), with the warped size that goes with the gate."""
    t["geom"] = geom
    for P in t:
        P["wh"], P["ww"] = M.canvas(P, int(P["h"]), int(P["w"]), int(run["geom_type"])) if P["geom"] else (P["h"], P["w"])


def _check(got, want, exact, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if exact:
        assert d.max(initial=0) == 0, (what, int((d > 0).sum()), d.size)
    else:
        assert d.max(initial=0) <= 1 and (d > 0).mean() <= 1e-3, (what, int((d > 0).sum()), d.size)


# ---------------------------------------------------------------------------------------------------------------------------------- sampler
def test_run_parameters():
    runs = [draw_abi_run(s) for s in range(3000)]
    g = np.array([int(r["geom_type"]) for r in runs])
    for t in range(3):
        assert abs((g == t).mean() - (0.33, 0.33, 0.34)[t]) < 0.04
    assert all(1 <= r["noise_var"] <= 19 and 1 <= r["mb_size"] <= 5 and -90 <= r["mb_angle"] <= 90 and 0 <= r["rescale_factor"] <= 4
               and sorted(r["det_order"]) == [0, 1, 2] for r in runs)
    assert set(int(r["rescale_factor"]) for r in runs) == {0, 1, 2, 3, 4}
    assert draw_abi_run(5) == draw_abi_run(5) and AbiAugment(5, "cpu").run == draw_abi_run(5)


def test_sampler_distributions(abi_dev):
    n = 20000
    rng = np.random.RandomState(1)
    hs, ws = list(rng.randint(1, 80, n)), list(rng.randint(1, 300, n))
    t, info = _sample(abi_dev, hs, ws, _run(geom_type=1))
    for f, p in (("geom", 0.5), ("det", 0.25), ("jit", 0.25)):
        sd = np.sqrt(p * (1 - p) / n)
        assert abs(t[f].mean() - p) < 4.5 * sd, f
    for f in ("angle", "shear"):
        a = t[f] if f == "angle" else t[f][:, 0]
        assert abs(a.mean()) < 0.5 and abs(a.std() - 15.0) < 0.4 and np.abs(a).max() <= 45, f     # sym(45): std 2 m / 6 = 15
    assert abs(t["shear"][:, 1].std() - 5.0) < 0.15 and np.abs(t["shear"][:, 1]).max() <= 15
    s = t["scale"]
    assert s.min() >= 0.5 and s.max() <= 2 and abs(s.mean() - 1.25) < 0.02 and abs(s.std() - 1.5 / np.sqrt(12)) < 0.01
    fr = t["persp_ow"][:, 0] / np.maximum(np.array(ws) * 0.25, 1e-9)                            # int(Beta(1,4) W / 4): mean ~ 0.2 - trunc
    assert (t["persp_ow"] >= 0).all() and (t["persp_ow"] <= np.array(ws)[:, None] // 4).all() and 0.12 < fr[np.array(ws) > 200].mean() < 0.2
    for f in ("geom_interp", "rs_interp"):
        v = t[f].reshape(-1)
        assert np.allclose(np.bincount(v, minlength=4) / v.size, 0.25, atol=0.015), f
    assert all(sorted(r) == [0, 1, 2, 3] for r in t["jit_order"])
    jf = t["jit_factor"]
    assert (np.abs(jf[:, :3] - 1) <= 0.5).all() and (np.abs(jf[:, 3]) <= 0.1).all()
    # layout: offsets are the prefix sum of the per-image bytes, info the totals
    run = _run(geom_type=1)
    tt = t.copy()
    assert M.layout(tt, run) == info[0] and np.array_equal(tt["ws_off"], t["ws_off"]) and np.array_equal(tt["final_buf"], t["final_buf"])
    assert info[1] == t["wh"].max() and info[2] == t["ww"].max()


@pytest.mark.gpu
def test_sampler_builds_identical():
    """HIP and the plain-C++ build draw bit-identical tables (every field, the derived geometry included)."""
    from cpu_abi_util import cpu_abi_backend
    rng = np.random.RandomState(2)
    hs, ws = list(rng.randint(1, 120, 3000)), list(rng.randint(1, 500, 3000))
    for gt in range(3):
        run = _run(geom_type=gt, mb_size=1 + gt * 2, mb_angle=-70.0 + 50 * gt)
        a, ia = _sample(torch.device("cuda:0"), hs, ws, run, seed=99, step=5)
        with cpu_abi_backend() as d:
            b, ib = _sample(d, hs, ws, run, seed=99, step=5)
        assert a.tobytes() == b.tobytes() and np.array_equal(ia, ib), gt


@pytest.mark.parametrize("geom_type", [0, 1, 2])
def test_canvas_sizes(abi_dev, geom_type):
    rng = np.random.RandomState(10 + geom_type)
    hs, ws = list(rng.randint(1, 100, 400)), list(rng.randint(1, 400, 400))
    t, _ = _sample(abi_dev, hs, ws, _run(geom_type=geom_type), seed=geom_type)
    on = t["geom"] == 1
    assert on.sum() > 150
    for P, h, w in zip(t[on], np.array(hs)[on], np.array(ws)[on]):
        assert (int(P["wh"]), int(P["ww"])) == M.canvas(P, int(h), int(w), geom_type), (geom_type, h, w, P["angle"], P["scale"], P["shear"])
    assert (t["wh"][~on] == np.array(hs)[~on]).all() and (t["ww"][~on] == np.array(ws)[~on]).all()


# ---------------------------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("geom_type", [0, 1, 2])
def test_warp_against_model(abi_dev, geom_type):
    rng = np.random.RandomState(20 + geom_type)
    crops = _crops(rng, 8)
    run = _run(geom_type=geom_type)
    t, _ = _sample(abi_dev, [c.shape[0] for c in crops], [c.shape[1] for c in crops], run, seed=3)
    exact = abi_dev.type == "cpu"
    for interp in range(4):
        tt = t.copy()
        tt["det"], tt["jit"], tt["geom_interp"] = 0, 0, interp
        _gate(tt, run, 1)
        finals, out, tt = _stages(abi_dev, crops, tt, run)
        for i, (c, P) in enumerate(zip(crops, tt)):
            _check(finals[i], M.warp(c, P), exact, ("warp", geom_type, interp, i))
            _check(out[i], M.tail(finals[i], P), True, ("tail after warp", geom_type, interp, i))


@pytest.mark.parametrize("order", [(0, 1, 2), (1, 2, 0), (2, 0, 1)])
def test_deterioration_against_model(abi_dev, order):
    rng = np.random.RandomState(sum(order) * 7 + order[0])
    exact = abi_dev.type == "cpu"
    cases = [(d, f, (a, b)) for d, f, (a, b) in zip([1, 2, 3, 4, 5], [0, 1, 2, 3, 4], [(0, 1), (1, 2), (2, 3), (3, 0), (3, 3)])]
    cases += [(2, f, (a, b)) for f in (1, 4) for a, b in ((0, 0), (1, 1), (2, 2))]
    for d, factor, (ia, ib) in cases:
        crops = _crops(rng, 3, 10, 24)
        run = _run(geom_type=int(rng.randint(3)), noise_var=int(rng.randint(1, 20)), mb_size=d, mb_angle=float(rng.uniform(-90, 90)),
                   factor=factor, order=order)
        t, _ = _sample(abi_dev, [c.shape[0] for c in crops], [c.shape[1] for c in crops], run, seed=d * 10 + factor)
        t["det"], t["jit"], t["rs_interp"] = 1, 0, (ia, ib)
        _gate(t, run, [0, 1, 0])
        finals, out, t = _stages(abi_dev, crops, t, run)
        for i, (c, P) in enumerate(zip(crops, t)):
            x = M.warp(c, P) if P["geom"] else c
            want = M.deteriorate(x, P, run, i)
            _check(finals[i], want, exact or factor == 0, ("det", order, d, factor, ia, ib, i))


def test_tail_golden(abi_dev):
    """The model's tail and the device tail (jitter at the image's resolution, Pillow bicubic resize) against Pillow."""
    g = np.load(GOLD)
    n = int(g["n_cases"][0])
    crops = [g[f"crop_{i}"] for i in range(n)]
    t = np.zeros(n, ABI_PARAMS_DTYPE)
    for i, c in enumerate(crops):
        t[i]["h"], t[i]["w"], t[i]["wh"], t[i]["ww"] = c.shape[0], c.shape[1], c.shape[0], c.shape[1]
        t[i]["jit"], t[i]["jit_order"], t[i]["jit_factor"] = 1, g[f"order_{i}"], g[f"factors_{i}"]
        t[i]["hue_shift"] = int(float(t[i]["jit_factor"][3]) * 255.0) % 256
    _, out, t = _stages(abi_dev, crops, t, _run())
    for i in range(n):
        want = g[f"out_{i}"]
        assert np.array_equal(M.tail_u8(crops[i], t[i]), want), i
        assert np.array_equal(out[i], IO.to_tensor_normalize(want)), i


def test_all_gates_off_is_resize_normalize(abi_dev):
    from dig_amd.datasets import resize_normalize
    rng = np.random.RandomState(5)
    crops = _crops(rng, 6, 70, 300)
    t, _ = _sample(abi_dev, [c.shape[0] for c in crops], [c.shape[1] for c in crops], _run())
    t["det"], t["jit"] = 0, 0
    _gate(t, _run(), 0)
    _, out, _ = _stages(abi_dev, crops, t, _run())
    assert np.array_equal(out, resize_normalize(crops, device=abi_dev).cpu().numpy())


def test_full_pipeline_against_model(abi_dev):
    """Sampled tables end to end (all gates as drawn), AbiAugment.__call__ against the model image by image."""
    rng = np.random.RandomState(6)
    crops = _crops(rng, 24, 12, 36)
    aug = AbiAugment(11, abi_dev)
    aug.run = _run(geom_type=2, factor=1, order=(2, 1, 0))
    params, _ = aug.sample(pack_crops(crops, abi_dev))
    t = abi_params_to_numpy(params)
    out = aug(crops).cpu().numpy()
    assert aug.step == 1 and t["geom"].any() and t["det"].any() and t["jit"].any()
    tol = 1.5 / 255 / 0.5 if abi_dev.type != "cpu" else 0
    for i, (c, P) in enumerate(zip(crops, t)):
        assert np.abs(out[i] - M.augment(c, P, aug.run, i)).max() <= tol + 1e-6, i


# ---------------------------------------------------------------------------------------------------------------------------------- ABI
def test_bad_arguments(abi_dev):
    null = None
    crops = _crops(np.random.RandomState(8), 2)
    pk = pack_crops(crops, abi_dev)
    aug = AbiAugment(0, abi_dev)
    params, info = aug.sample(pk)
    run = np.ascontiguousarray(np.asarray(aug.run, ABI_RUN_DTYPE).reshape(1))
    rp = ctypes.c_void_p(run.ctypes.data)
    work = torch.zeros(1 << 20, dtype=torch.uint8, device=abi_dev)
    out = torch.empty((2, 3, 32, 128), device=abi_dev)
    lib = L.lib()
    S = L.stream()
    a = (L.ptr(pk.data), L.ptr(pk.offsets), L.ptr(pk.heights), L.ptr(pk.widths))

    def rc(name, *args):
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = L._prototypes()[name]
        return f(*args)
    assert rc("dig_abiaug_sample", L.ptr(params), L.ptr(info), a[2], a[3], 0, rp, 0, 0, S) == -1
    assert rc("dig_abiaug_sample", L.ptr(params), null, a[2], a[3], 2, rp, 0, 0, S) == -1
    assert rc("dig_abiaug_sample", L.ptr(params), L.ptr(info), a[2], a[3], 2, null, 0, 0, S) == -1
    for bad in (dict(geom_type=3), dict(mb_size=0), dict(mb_size=6), dict(factor=5), dict(noise_var=-1)):
        r = np.ascontiguousarray(_run(**bad).reshape(1))
        assert rc("dig_abiaug_sample", L.ptr(params), L.ptr(info), a[2], a[3], 2, ctypes.c_void_p(r.ctypes.data), 0, 0, S) == -1, bad
    f = lib.dig_abiaug_workspace_bytes
    f.restype, f.argtypes = ctypes.c_longlong, L._prototypes()["dig_abiaug_workspace_bytes"]
    assert f(1, 0, 0, 10, rp) == -1 and f(1, 1, 10, 10, null) == -1 and f(0, 0, 10, 10, rp) == 0
    assert f(1, 0, 10, 10, rp) == 512 and f(0, 1, 10, 10, rp) == 1024 + (M.RS_BYTES if aug.run["rescale_factor"] > 0 else 0)
    for name in ("dig_abiaug_warp_u8", "dig_abiaug_deteriorate_u8"):
        assert rc(name, *a, 2, L.ptr(params), rp, L.ptr(work), work.numel(), 0, 8, S) == -1
        assert rc(name, *a, 2, L.ptr(params), rp, null, work.numel(), 8, 8, S) == -1
        assert rc(name, null, *a[1:], 2, L.ptr(params), rp, L.ptr(work), work.numel(), 8, 8, S) == -1
        assert rc(name, *a, 2, L.ptr(params), rp, L.ptr(work), -1, 8, 8, S) == -1
        assert rc(name, *a, 2, null, rp, L.ptr(work), work.numel(), 8, 8, S) == -1
    tl = lambda *x: rc("dig_abiaug_tail", *a, 2, L.ptr(params), rp, L.ptr(work), work.numel(), *x, S)  # noqa: E731
    assert tl(null, 32, 128, ctypes.c_float(.5), ctypes.c_float(.5), 64, 64) == -1
    assert tl(L.ptr(out), 0, 128, ctypes.c_float(.5), ctypes.c_float(.5), 64, 64) == -1
    assert tl(L.ptr(out), 32, 128, ctypes.c_float(.5), ctypes.c_float(0), 64, 64) == -1
    assert tl(L.ptr(out), 32, 128, ctypes.c_float(.5), ctypes.c_float(.5), 1 << 20, 1 << 20) == -4


def test_short_workspace_skips_the_image(abi_dev):
    """A table whose region lies past work_bytes is not written (the image is skipped, nothing outside the workspace is touched)."""
    crops = [np.full((6, 10, 3), 77, np.uint8), np.full((6, 10, 3), 99, np.uint8)]
    run = _run(factor=0)
    t, _ = _sample(abi_dev, [6, 6], [10, 10], run)
    t["det"], t["jit"] = 0, 0
    _gate(t, run, 1)
    M.layout(t, run)
    need = int(t["ws_off"][1]) + M.image_bytes(1, 0, int(t["wh"][1]), int(t["ww"][1]), 0)
    pk = pack_crops(crops, abi_dev)
    aug = AbiAugment(0, abi_dev)
    aug.run = run
    work = torch.full((need + 64,), 5, dtype=torch.uint8, device=abi_dev)
    aug.warp(pk, abi_params_from_numpy(t, abi_dev), work[:need - 1], int(t["wh"].max()), int(t["ww"].max()))
    w = work.cpu().numpy()
    assert (w[int(t["ws_off"][1]):] == 5).all() and (w[:3 * int(t["wh"][0]) * int(t["ww"][0])] == 77).all()


# ---------------------------------------------------------------------------------------------------------------------------------- transform
def test_finetune_transform_selection(abi_dev):
    from dig_amd.datasets import FinetuneBatchTransform, resize_normalize
    crops = _crops(np.random.RandomState(9), 5, 40, 200)
    base = dict(input_h=32, input_w=128)
    cases = [(dict(num_view=2, use_abi_aug=True), False, "resize"), (dict(num_view=1, use_abi_aug=True), True, "resize"),
             (dict(num_view=2, use_abi_aug=True), True, "abi"), (dict(num_view=2, use_abi_aug=False), True, "keyview")]
    for extra, train, kind in cases:
        tf = FinetuneBatchTransform(types.SimpleNamespace(**base, **extra), train, seed=4, device=abi_dev)
        assert tf.kind == kind
        got = [tf(crops).cpu().numpy() for _ in range(2)]
        if kind == "resize":
            ref = [resize_normalize(crops, device=abi_dev).cpu().numpy()] * 2
        else:
            o = AbiAugment(4, abi_dev) if kind == "abi" else KeyViewAugment(4, abi_dev)
            ref = [o(crops).cpu().numpy() for _ in range(2)]
        for g_, r_ in zip(got, ref):
            assert np.array_equal(g_, r_), kind
        if kind != "resize":
            assert not np.array_equal(got[0], got[1])        # the step counter advances


@pytest.mark.gpu
def test_finetune_steps_with_abi_aug():
    """Two train_one_epoch steps of a tiny RecModelTrain fed by FinetuneBatchTransform(num_view=2, use_abi_aug=True): finite losses, and
    the views differ from resize_normalize exactly on the images whose gates fired."""
    import test_finetune as TF
    from dig_amd.datasets import FinetuneBatchTransform, resize_normalize
    from dig_amd.engine_for_finetuning import train_one_epoch
    from dig_amd.finetune import LayerDecayValueAssigner, SeqCrossEntropyLoss, create_optimizer
    from dig_amd.utils import NativeScalerWithGradNormCount
    _, c, ecfg, P, _, _, _ = TF._fixture()
    m = TF._device_model(c, ecfg, P)
    nl, lr, wd = m.get_num_layers(), 1e-3, 0.05
    assigner = LayerDecayValueAssigner([0.75 ** (nl + 1 - i) for i in range(nl + 2)])
    args = types.SimpleNamespace(opt="adamw", lr=lr, weight_decay=wd, opt_eps=1e-8, opt_betas=None, eval_freq=1000, input_h=32, input_w=128,
                                 num_view=2, use_abi_aug=True)
    opt = create_optimizer(args, m, get_num_layer=assigner.get_layer_id, get_layer_scale=assigner.get_scale)
    tf = FinetuneBatchTransform(args, True, seed=3, device="cuda:0")
    rng = np.random.RandomState(4)
    batches, fired = [], 0
    for s in range(2):
        B = 16
        crops = _crops(rng, B, 64, 300)
        pk = pack_crops(crops, "cuda:0")
        params, _ = tf.aug.sample(pk)
        t = abi_params_to_numpy(params)
        x = tf(pk)
        plain = resize_normalize(pk)
        differs = (x - plain).abs().flatten(1).amax(1).cpu().numpy() > 0
        gates = (t["geom"] | t["det"] | t["jit"]).astype(bool)
        assert not differs[~gates].any() and differs[gates].mean() > 0.9
        fired += int(gates.sum())
        lens = torch.from_numpy(rng.randint(1, c.max_seq_len + 1, size=B))
        tg = torch.from_numpy(rng.randint(0, 94, size=(B, c.max_seq_len)))
        for b in range(B):
            tg[b, int(lens[b]) - 1] = 94
            tg[b, int(lens[b]):] = 95
        batches.append((x, tg, lens))
    assert fired > 8
    loader = type("Ldr", (list,), {})(batches)
    loader.dataset = types.SimpleNamespace(idx_to_class={i: ch for i, ch in enumerate(TF.D.vocabulary())})
    stats = train_one_epoch(m, SeqCrossEntropyLoss(), loader, opt, torch.device("cuda:0"), 0, NativeScalerWithGradNormCount(), None, None, None,
                            None, start_steps=0, lr_schedule_values=np.array([lr, lr]), wd_schedule_values=np.array([wd, wd]),
                            num_training_steps_per_epoch=2, update_freq=1, args=args)
    assert np.isfinite(stats["loss"])
