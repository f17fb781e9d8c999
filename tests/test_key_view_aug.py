"""Key-view augmentation of MoCo pre-training (dig_amd/augment.py, dig_amd/csrc/keyview.hip): the sampler's structure and distributions, each
stage-A op and sampled op sequences against the numpy model (tests/keyview_model.py), stage B against Pillow (tests/golden/key_view_tail.npz,
tools/gen_key_view_golden.py), the identity table against the plain input transform, and the batch transform / driver surfaces.
Operator tests run through the HIP library on the MI355X and through the plain-C++ build in the GPU-less container (`abi_dev`)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import input_oracle as IO
import keyview_model as M
from dig_amd.augment import PARAMS_DTYPE, KeyViewAugment, PackedCrops, pack_crops, params_from_numpy, params_to_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "key_view_tail.npz")

# Ops whose per-pixel work is a LUT / blend / short stencil: bit-exact on every build, no allowance.  The blur and the resamplers
# (1, 2, 3, 5, 6, 7) are bit-exact on the plain-C++ build; on the device they are allowed |diff| <= 1 on <= 0.1 % of the pixels, for a
# source coordinate (a float32 divide in the homography / crop scale, the barycentric weights) or a long weighted sum landing within an
# ulp of a rounding boundary of floor(t + 0.5) -- keyview.hip is compiled without contraction, so none is expected.
EXACT_OPS = {0, 4, 8, 9}


def _sizes_packed(hs, ws, dev):
    """A PackedCrops carrying only the sizes (what the sampler reads)."""
    h = torch.tensor(hs, dtype=torch.int32, device=dev)
    w = torch.tensor(ws, dtype=torch.int32, device=dev)
    return PackedCrops(torch.zeros(1, dtype=torch.uint8, device=dev), None, h, w, len(hs), int(max(hs)), int(max(ws)))


def _sample(dev, hs, ws, seed, step):
    return params_to_numpy(KeyViewAugment(seed, dev).sample(_sizes_packed(hs, ws, dev), step=step))


def _stage_a(dev, crops, tables):
    packed = pack_crops(crops, dev)
    work = KeyViewAugment.stage_a(packed, params_from_numpy(tables, dev)).cpu().numpy()
    offs = packed.offsets.cpu().numpy()
    return [work[o:o + c.size].reshape(c.shape) for o, c in zip(offs, crops)]


def _check(got, want, ops, exact, what):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if exact or set(ops) <= EXACT_OPS:
        assert d.max(initial=0) == 0, (what, ops, int((d > 0).sum()), d.size)
    else:
        assert d.max(initial=0) <= 1 and (d > 0).mean() <= 1e-3, (what, ops, int((d > 0).sum()), d.size)


def _ragged(rng, n, hmax=120, wmax=400):
    return [rng.randint(0, 256, size=(rng.randint(1, hmax), rng.randint(1, wmax), 3)).astype(np.uint8) for _ in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------- sampler
def test_sampler_structure(abi_dev):
    rng = np.random.RandomState(1)
    hs, ws = list(rng.randint(1, 200, 512)), list(rng.randint(1, 700, 512))
    hs[:3], ws[:3] = [1, 1, 200], [1, 300, 1]
    t = _sample(abi_dev, hs, ws, 0x5EED, 3)
    assert ((t["n_ops"] >= 2) & (t["n_ops"] <= 5)).all()
    for r in t:
        ops = r["ops"][:r["n_ops"]]
        assert len(set(ops)) == len(ops) and ((ops >= 0) & (ops <= 9)).all() and (r["ops"][r["n_ops"]:] == -1).all()
        assert sorted(r["jit_order"]) == [0, 1, 2, 3]
    for name, lo, hi in (("contrast_alpha", .5, 1), ("blur_sigma", .5, 1.5), ("crop_tb", 0, .3), ("crop_lr", 0, .1), ("sharpen_alpha", 0, .5),
                         ("sharpen_lightness", 0, .5), ("rotate_deg", -10, 10), ("pa_scale", .03, .04), ("persp_sigma", .05, .1),
                         ("solar_tau", 32, 128), ("gray_alpha", 0, 1)):
        assert (t[name] >= np.float32(lo)).all() and (t[name] <= np.float32(hi)).all(), name
    jf = t["jit_factor"]
    assert (np.abs(jf[:, :2] - 1) <= np.float32(.4)).all() and (np.abs(jf[:, 2] - 1) <= np.float32(.2)).all() and (np.abs(jf[:, 3]) <= .1).all()
    for f in ("jitter", "gray", "solar_above"):
        assert set(np.unique(t[f])) <= {0, 1}
    assert (t["persp_d"] >= 0).all() and (t["pad"] == 0).all()
    # derived coefficients = the model's derivation from the raw draws (integers exactly; floats to rounding)
    for r, h, w in zip(t, hs, ws):
        ref = M.derive(r.copy(), h, w)
        for f in ("blur_radius", "crop_y", "crop_x", "hue_shift"):
            assert np.array_equal(r[f], ref[f]), (f, h, w)
        for f in ("blur_taps", "sharpen_k", "rot", "homog"):
            np.testing.assert_allclose(r[f], ref[f], rtol=1e-5, atol=1e-4 * max(h, w), err_msg=f)
    # counter-based: reproducible from (seed, step); another step or seed gives another table
    assert t.tobytes() == _sample(abi_dev, hs, ws, 0x5EED, 3).tobytes()
    for other in (_sample(abi_dev, hs, ws, 0x5EED, 4), _sample(abi_dev, hs, ws, 0x5EEE, 3)):
        assert (other["n_ops"] != t["n_ops"]).any() and (other["contrast_alpha"] != t["contrast_alpha"]).mean() > .99


@pytest.mark.gpu
def test_sampler_hip_and_cpu_tables_agree():
    from cpu_abi_util import cpu_abi_backend
    rng = np.random.RandomState(2)
    hs, ws = list(rng.randint(1, 200, 4096)), list(rng.randint(1, 700, 4096))
    hip = _sample(torch.device("cuda:0"), hs, ws, 77, 11)
    with cpu_abi_backend() as d:
        cpu = _sample(d, hs, ws, 77, 11)
    # the sampler's transcendentals are series of basic operations (keyview.inc), not libm: the tables agree bit for bit, floats included
    for name in PARAMS_DTYPE.names:
        a, b = hip[name], cpu[name]
        if a.dtype.kind == "i":
            assert np.array_equal(a, b), name
        else:
            ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
            assert ulp.max() == 0, (name, int(ulp.max()), int((ulp > 0).sum()))


def test_sampler_distributions(abi_dev):
    N = 65536
    rng = np.random.RandomState(3)
    hs, ws = list(rng.randint(1, 200, N)), list(rng.randint(1, 700, N))
    t = _sample(abi_dev, hs, ws, 12345, 0)

    def near(x, p, n, what):
        assert abs(x - p) <= 5 * np.sqrt(p * (1 - p) / n), (what, x, p)
    for k in range(2, 6):
        near((t["n_ops"] == k).mean(), .25, N, f"n={k}")
    ops = t["ops"]
    for o in range(10):
        near((ops == o).any(1).mean(), .35, N, f"op {o} included")
    for pos in range(5):
        rows = ops[t["n_ops"] > pos, pos]
        for o in range(10):
            near((rows == o).mean(), .1, len(rows), f"op {o} at position {pos}")
    near(t["jitter"].mean(), .8, N, "jitter")
    near(t["gray"].mean(), .2, N, "grayscale")
    near(t["solar_above"].mean(), .5, N, "solarize above")
    code = (t["jit_order"] * np.array([64, 16, 4, 1])).sum(1)
    for c in np.unique(code):
        near((code == c).mean(), 1 / 24, N, "jitter permutation")
    assert len(np.unique(code)) == 24
    for name, col, lo, hi in (("contrast_alpha", None, .5, 1), ("blur_sigma", None, .5, 1.5), ("crop_tb", 0, 0, .3), ("crop_tb", 1, 0, .3),
                              ("crop_lr", 0, 0, .1), ("sharpen_alpha", None, 0, .5), ("sharpen_lightness", None, 0, .5),
                              ("rotate_deg", None, -10, 10), ("pa_scale", None, .03, .04), ("persp_sigma", None, .05, .1),
                              ("solar_tau", None, 32, 128), ("gray_alpha", None, 0, 1), ("jit_factor", 0, .6, 1.4), ("jit_factor", 1, .6, 1.4),
                              ("jit_factor", 2, .8, 1.2), ("jit_factor", 3, -.1, .1)):
        x = t[name].astype(np.float64) if col is None else t[name][:, col].astype(np.float64)
        assert abs(x.mean() - (lo + hi) / 2) <= 5 * (hi - lo) / np.sqrt(12 * N), name
    # the normals behind the displacements: N(0, 1) after dividing out s * H / s * W; |N(0, 1)| behind the perspective corners
    z = np.concatenate([(t["pa_dy"] / (t["pa_scale"][:, None] * np.array(hs)[:, None])).ravel(),
                        (t["pa_dx"] / (t["pa_scale"][:, None] * np.array(ws)[:, None])).ravel()])
    assert abs(z.mean()) <= 5 / np.sqrt(z.size) and abs(z.var() - 1) <= 5 * np.sqrt(2 / z.size)
    a = (t["persp_d"] / t["persp_sigma"][:, None]).ravel()
    assert abs(a.mean() - np.sqrt(2 / np.pi)) <= 5 * np.sqrt((1 - 2 / np.pi) / a.size)


# ---------------------------------------------------------------------------------------------------------------------------------- stage A
def _op_table(rng, k, h, w):
    raw = {0: dict(contrast_alpha=rng.uniform(.5, 1)), 1: dict(blur_sigma=rng.uniform(.5, 1.5)),
           2: dict(crop_tb=rng.uniform(0, .3, 2)), 3: dict(crop_lr=rng.uniform(0, .1, 2)),
           4: dict(sharpen_alpha=rng.uniform(0, .5), sharpen_lightness=rng.uniform(0, .5)), 5: dict(rotate_deg=rng.uniform(-10, 10)),
           6: dict(pa_dy=rng.randn(16) * .035 * h, pa_dx=rng.randn(16) * .035 * w),
           7: dict(persp_d=np.abs(rng.randn(8)) * rng.uniform(.05, .1)),
           8: dict(solar_tau=rng.uniform(32, 128), solar_above=rng.randint(2)), 9: dict(gray_alpha=rng.uniform(0, 1))}[k]
    return M.table(h, w, ops=[k], **raw)


@pytest.mark.parametrize("k", range(10))
def test_stage_a_each_op_matches_the_model(abi_dev, k):
    rng = np.random.RandomState(100 + k)
    crops = [rng.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in ((1, 1), (1, 37), (23, 1), (2, 2), (200, 700), (32, 128))]
    crops += _ragged(rng, 10)
    tables = np.array([_op_table(rng, k, *c.shape[:2]) for c in crops], dtype=PARAMS_DTYPE)
    if k in (2, 3):                                              # the extremes of the crop ranges
        tables[0]["crop_tb"] = tables[0]["crop_lr"] = [.3, .3]
        tables[4] = M.table(200, 700, ops=[k], crop_tb=[.3, .3], crop_lr=[.1, .1])
    got = _stage_a(abi_dev, crops, tables)
    for i, (c, t, g) in enumerate(zip(crops, tables, got)):
        _check(g, M.stage_a(c, t), [k], abi_dev.type == "cpu", f"crop {i} {c.shape}")


def test_stage_a_sampled_sequences_match_the_model(abi_dev):
    rng = np.random.RandomState(5)
    crops = _ragged(rng, 256, 100, 320)
    packed = pack_crops(crops, abi_dev)
    tables = params_to_numpy(KeyViewAugment(99, abi_dev).sample(packed))
    got = _stage_a(abi_dev, crops, tables)
    for i, (c, t, g) in enumerate(zip(crops, tables, got)):
        _check(g, M.stage_a(c, t), list(t["ops"][:t["n_ops"]]), abi_dev.type == "cpu", f"crop {i} {c.shape}")


# ---------------------------------------------------------------------------------------------------------------------------------- stage B
def _golden_tables():
    z = np.load(GOLD)
    crops = M.golden_crops()
    n = int(z["n_cases"][0])
    tables = np.array([M.table(*crops[i].shape[:2], jitter=z[f"flags_{i}"][0], gray=z[f"flags_{i}"][1], jit_order=z[f"order_{i}"],
                               jit_factor=z[f"factors_{i}"]) for i in range(n)], dtype=PARAMS_DTYPE)
    return z, crops[:n], tables


def test_model_stage_b_equals_the_pillow_fixture():
    z, crops, tables = _golden_tables()
    for i, (c, t) in enumerate(zip(crops, tables)):
        assert np.array_equal(M.stage_b_u8(c, t), z[f"out_{i}"]), i


def test_stage_b_equals_the_pillow_fixture(abi_dev):
    z, crops, tables = _golden_tables()
    out = KeyViewAugment(0, abi_dev).apply(pack_crops(crops, abi_dev), params_from_numpy(tables, abi_dev)).cpu().numpy()
    for i in range(len(crops)):
        assert np.array_equal(out[i], IO.to_tensor_normalize(z[f"out_{i}"])), (i, z[f"order_{i}"], z[f"flags_{i}"])


def test_hsv_conversions_equal_pillow_on_every_colour():
    Image = pytest.importorskip("PIL.Image")
    c = np.arange(1 << 24, dtype=np.uint32)
    px = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    hsv = np.asarray(Image.fromarray(px, "RGB").convert("HSV"))
    h, s, v = M.rgb2hsv(px[..., 0], px[..., 1], px[..., 2])
    assert np.array_equal(np.stack([h, s, v], -1), hsv)
    rgb = np.asarray(Image.frombytes("HSV", (4096, 4096), px.tobytes()).convert("RGB"))     # every (h, s, v) triple back to RGB
    assert np.array_equal(np.stack(M.hsv2rgb(px[..., 0], px[..., 1], px[..., 2]), -1), rgb)


def test_identity_table_equals_the_plain_transform(abi_dev):
    from dig_amd.datasets import resize_normalize
    rng = np.random.RandomState(8)
    crops = _ragged(rng, 24, 180, 700) + [np.full((1, 1, 3), 9, np.uint8)]
    tables = np.array([M.identity_table() for _ in crops], dtype=PARAMS_DTYPE)
    packed = pack_crops(crops, abi_dev)
    out = KeyViewAugment(0, abi_dev).apply(packed, params_from_numpy(tables, abi_dev))
    assert torch.equal(out.cpu(), resize_normalize(crops, device=abi_dev).cpu())


def test_sampled_key_views_match_the_model(abi_dev):
    rng = np.random.RandomState(9)
    crops = _ragged(rng, 48, 80, 300)
    aug = KeyViewAugment(2024, abi_dev)
    packed = pack_crops(crops, abi_dev)
    tables = params_to_numpy(aug.sample(packed))
    out = aug(packed).cpu().numpy()
    assert aug.step == 1
    for i, (c, t) in enumerate(zip(crops, tables)):
        ops = list(t["ops"][:t["n_ops"]])
        want = M.key_view(c, t)
        if abi_dev.type == "cpu" or set(ops) <= EXACT_OPS:
            assert np.array_equal(out[i], want), (i, ops)
        else:                                                   # a stage-A pixel one level off moves the resized pixels by a few levels
            assert (out[i] != want).mean() <= 0.02, (i, ops)


def test_entry_points_reject_bad_arguments(abi_dev):
    from dig_amd import _lib
    aug = KeyViewAugment(0, abi_dev)
    packed = pack_crops([np.zeros((4, 5, 3), np.uint8)], abi_dev)
    with pytest.raises(_lib.DigHipError, match="bad argument"):
        _lib.call("dig_keyview_sample", None, _lib.ptr(packed.heights), _lib.ptr(packed.widths), 1, 0, 0, _lib.stream())
    params = aug.sample(packed)
    with pytest.raises(_lib.DigHipError, match="bad argument"):                   # workspace smaller than a crop
        _lib.call("dig_keyview_stage_a_u8", _lib.ptr(packed.data), _lib.ptr(packed.offsets), _lib.ptr(packed.heights), _lib.ptr(packed.widths), 1,
                  _lib.ptr(params), _lib.ptr(torch.empty(512, dtype=torch.uint8, device=abi_dev)), 512, 400, 400, _lib.stream())
    with pytest.raises(_lib.DigHipError, match="unsupported"):                    # coefficient tables beyond the LDS
        _lib.call("dig_keyview_stage_b", _lib.ptr(packed.data), _lib.ptr(packed.offsets), _lib.ptr(packed.heights), _lib.ptr(packed.widths), 1,
                  _lib.ptr(params), _lib.ptr(torch.empty(3 * 32 * 128, device=abi_dev)), 32, 128, 0.5, 0.5, 4, 100000, _lib.stream())


# ---------------------------------------------------------------------------------------------------------------------------------- surfaces
def _transform_args():
    import types
    return types.SimpleNamespace(input_h=32, input_w=128, window_size=(8, 32), mask_ratio=0.7, num_view=2)


@pytest.mark.gpu
def test_gpu_batch_transform_builds_the_key_view():
    from dig_amd.datasets import GpuBatchTransform
    rng = np.random.RandomState(10)
    crops = _ragged(rng, 16, 60, 300)
    tf = GpuBatchTransform(_transform_args(), seed=4, device="cuda:0", key_view_aug="seqclr")
    images, aug, masks = tf(crops)
    assert images.shape == aug.shape == (16, 3, 32, 128) and aug.dtype == torch.float32 and masks.shape == (16, 2, 256)
    assert float(aug.min()) >= -1 and float(aug.max()) <= 1
    plain_images, plain_aug, _ = GpuBatchTransform(_transform_args(), seed=4, device="cuda:0")(crops, crops)
    assert torch.equal(images, plain_images) and not torch.equal(aug, plain_aug)
    # reproducible from (seed, step): a fresh transform replays step 0; step 1 differs
    again = GpuBatchTransform(_transform_args(), seed=4, device="cuda:0", key_view_aug="seqclr")
    assert torch.equal(again(crops)[1], aug)
    assert not torch.equal(again(crops)[1], aug)
    # the key view is the model's at (seed, step 0)
    tables = params_to_numpy(KeyViewAugment(4, "cuda:0").sample(pack_crops(crops, "cuda:0")))
    exact = [i for i, t in enumerate(tables) if set(t["ops"][:t["n_ops"]]) <= EXACT_OPS]
    for i in exact:
        assert np.array_equal(aug[i].cpu().numpy(), M.key_view(crops[i], tables[i])), i
    # explicit aug_crops: today's output
    i2, a2, _ = tf(crops, crops[::-1])
    assert np.array_equal(a2[0].cpu().numpy(), IO.transform(crops[-1]))


def _driver():
    spec = importlib.util.spec_from_file_location("dig_driver_kv", os.path.join(ROOT, "run_mae_pretraining_moco.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_driver_key_view_aug_flag():
    drv = _driver()
    assert drv.get_args([]).key_view_aug == "none"
    assert drv.get_args(["--key_view_aug", "seqclr", "--num_view", "2"]).key_view_aug == "seqclr"
    with pytest.raises(SystemExit):
        drv.get_args(["--key_view_aug", "seqclr", "--aug_module", "pkg.fn"])
    with pytest.raises(SystemExit):
        drv.get_args(["--key_view_aug", "imgaug"])


def test_batch_transform_rejects_unknown_key_view_aug():
    from dig_amd.datasets import GpuBatchTransform
    with pytest.raises(ValueError):
        GpuBatchTransform(_transform_args(), device="cpu", key_view_aug="abinet")


@pytest.mark.gpu
def test_driver_trains_with_the_device_key_view(tmp_path):
    import json
    import subprocess
    import sys
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(11)
    data = tmp_path / "data"
    data.mkdir()
    for i in range(8):
        Image.fromarray(rng.randint(0, 256, size=(rng.randint(20, 64), rng.randint(60, 300), 3)).astype(np.uint8)).save(data / f"{i}.png")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "run_mae_pretraining_moco.py"), "--image_alone_path", str(data), "--num_view", "2",
           "--key_view_aug", "seqclr", "--batch_size", "4", "--epochs", "1", "--output_dir", str(out), "--num_workers", "2",
           "--mask_ratio", "0.7", "--moco_dim", "256", "--moco_mlp_dim", "4096", "--moco_m", "0.99", "--moco_m_cos", "--moco_t", "0.2",
           "--num_windows", "4", "--warmup_epochs", "0", "--contrast_warmup_steps", "0", "--contrast_start_epoch", "0", "--loss_weight_contrast", "0.1",
           "--only_mim_on_ori_img", "--model", "pretrain_simmim_moco_ori_vit_small_patch4_32x128", "--patchnet_name", "no_patchtrans",
           "--encoder_type", "vit", "--save_ckpt_freq", "100"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    logs = [json.loads(line) for line in open(out / "log.txt")]
    assert logs and all(np.isfinite(v) for k, v in logs[-1].items() if k.startswith("train_loss"))
