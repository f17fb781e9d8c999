"""Key-view augmentation of MoCo pre-training on the device: the reference's `AloneImageLmdb` second view (dataset/dataset_image.py:39-50,
88-120,145-149) -- imgaug SomeOf((2, 5), 10 seqCLR ops) at the crop's resolution, Resize((32, 128), BICUBIC),
RandomApply([ColorJitter(0.4, 0.4, 0.2, 0.1)], p=0.8), RandomGrayscale(p=0.2), ToTensor, Normalize(0.5, 0.5).

The crops come in the packed upload the first view is resized from (`pack_crops`), so the key view costs no second upload:

    aug = KeyViewAugment(seed, device)
    key = aug(packed)                        # fp32 [n, 3, 32, 128]; draws its tables at (seed, step), then step += 1

Each image's parameters live in one 512-byte table (include/dig_aug_types.h, mirrored by `PARAMS_DTYPE`); the semantics of every field are
in dig_amd/csrc/keyview.inc.  `sample` / `stage_a` / `stage_b` expose the three entry points, so a caller (the tests) can pass tables of
its own."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L

# field order and sizes of struct dig_kv_params (include/dig_aug_types.h)
PARAMS_DTYPE = np.dtype([
    ("n_ops", "<i4"), ("ops", "<i4", 5),
    ("contrast_alpha", "<f4"), ("blur_sigma", "<f4"), ("crop_tb", "<f4", 2), ("crop_lr", "<f4", 2), ("sharpen_alpha", "<f4"),
    ("sharpen_lightness", "<f4"), ("rotate_deg", "<f4"), ("pa_scale", "<f4"), ("pa_dy", "<f4", 16), ("pa_dx", "<f4", 16),
    ("persp_sigma", "<f4"), ("persp_d", "<f4", 8), ("solar_tau", "<f4"), ("solar_above", "<i4"), ("gray_alpha", "<f4"),
    ("blur_radius", "<i4"), ("blur_taps", "<f4", 11), ("sharpen_k", "<f4", 9), ("crop_y", "<i4", 2), ("crop_x", "<i4", 2),
    ("rot", "<f4", 6), ("homog", "<f4", 9),
    ("jitter", "<i4"), ("jit_order", "<i4", 4), ("jit_factor", "<f4", 4), ("hue_shift", "<i4"), ("gray", "<i4"), ("pad", "<i4", 17)])
PARAMS_WORDS = L.const("DIG_KV_WORDS")
assert PARAMS_DTYPE.itemsize == 4 * PARAMS_WORDS

OP_NAMES = ("LinearContrast", "GaussianBlur", "CropRows", "CropCols", "Sharpen", "Rotate", "PiecewiseAffine", "PerspectiveTransform",
            "Solarize", "Grayscale")

# crops packed for the device: data uint8 [sum H*W*3], offsets int64 [n], heights / widths int32 [n] (all on `device`)
PackedCrops = namedtuple("PackedCrops", "data offsets heights widths n max_h max_w")


def pack_crops(crops, device="cuda"):
    """List of HxWx3 uint8 numpy arrays -> PackedCrops on `device`: one pinned staging buffer, one upload of the bytes and one of the
    metadata."""
    n = len(crops)
    hs = np.array([c.shape[0] for c in crops], dtype=np.int32)
    ws = np.array([c.shape[1] for c in crops], dtype=np.int32)
    sizes = hs.astype(np.int64) * ws.astype(np.int64) * 3
    offs = np.zeros(n, dtype=np.int64)
    np.cumsum(sizes[:-1], out=offs[1:])
    dev = torch.device(device)
    pin = (lambda t: t.pin_memory()) if dev.type == "cuda" else (lambda t: t)       # (pinned staging only where there is a device to copy to)
    packed = pin(torch.empty(int(sizes.sum()), dtype=torch.uint8))
    flat = packed.numpy()
    for c, o, s in zip(crops, offs, sizes):
        if c.dtype != np.uint8 or c.ndim != 3 or c.shape[2] != 3:
            raise ValueError("crops must be HxWx3 uint8 (the RGB image PIL decodes)")
        flat[o:o + s] = np.ascontiguousarray(c).reshape(-1)
    d_packed = packed.to(dev, non_blocking=True)
    d_meta = pin(torch.from_numpy(np.concatenate([offs, hs.astype(np.int64), ws.astype(np.int64)]))).to(dev, non_blocking=True)
    d_off, d_h, d_w = d_meta[:n], d_meta[n:2 * n].to(torch.int32), d_meta[2 * n:].to(torch.int32)
    return PackedCrops(d_packed, d_off, d_h, d_w, n, int(hs.max()), int(ws.max()))


def params_to_numpy(params):
    """Device / host table tensor (int32 [n, 128]) -> numpy structured array of PARAMS_DTYPE."""
    return params.cpu().numpy().view(PARAMS_DTYPE).reshape(-1)


def params_from_numpy(table, device):
    """numpy structured array of PARAMS_DTYPE -> int32 [n, 128] tensor on `device` (a caller-built table)."""
    a = np.ascontiguousarray(np.asarray(table, dtype=PARAMS_DTYPE))
    return torch.from_numpy(a.view(np.int32).reshape(-1, PARAMS_WORDS).copy()).to(device)


class KeyViewAugment:
    """The key view of a packed batch of crops, on the device.  `__call__` draws the tables for (seed, step) -- Philox4x32-10, a stream
    of its own next to the mask generator's -- runs both stages and advances its step counter, as RandomMaskingGenerator does."""

    def __init__(self, seed=0, device="cuda", out_h=32, out_w=128, mean=0.5, std=0.5):
        self.seed, self.step, self.device = int(seed), 0, torch.device(device)
        self.out_h, self.out_w, self.mean, self.std = out_h, out_w, mean, std

    def sample(self, packed, step=None):
        """int32 [n, 128] tables of every crop at (seed, step) (default: the current step; the counter is not advanced)."""
        params = torch.empty((packed.n, PARAMS_WORDS), device=packed.data.device, dtype=torch.int32)
        L.call("dig_keyview_sample", L.ptr(params), L.ptr(packed.heights), L.ptr(packed.widths), packed.n, ctypes.c_ulonglong(self.seed),
               ctypes.c_uint((self.step if step is None else step) & 0xFFFFFFFF), L.stream())
        return params

    @staticmethod
    def stage_a(packed, params):
        """Workspace (uint8, two halves) after stage A; image i's result is at [offsets[i], offsets[i] + H W 3) of the first half."""
        nbytes = packed.data.numel()
        ws = _workspace_bytes(nbytes, packed.n)
        work = torch.empty(ws, device=packed.data.device, dtype=torch.uint8)
        L.call("dig_keyview_stage_a_u8", L.ptr(packed.data), L.ptr(packed.offsets), L.ptr(packed.heights), L.ptr(packed.widths), packed.n,
               L.ptr(params), L.ptr(work), ws, packed.max_h, packed.max_w, L.stream())
        return work

    def stage_b(self, packed, params, work):
        out = torch.empty((packed.n, 3, self.out_h, self.out_w), device=packed.data.device, dtype=torch.float32)
        L.call("dig_keyview_stage_b", L.ptr(work), L.ptr(packed.offsets), L.ptr(packed.heights), L.ptr(packed.widths), packed.n, L.ptr(params),
               L.ptr(out), self.out_h, self.out_w, ctypes.c_float(self.mean), ctypes.c_float(self.std), packed.max_h, packed.max_w, L.stream())
        return out

    def apply(self, packed, params):
        """Both stages with the given tables: fp32 [n, 3, out_h, out_w]."""
        return self.stage_b(packed, params, self.stage_a(packed, params))

    def __call__(self, packed):
        if not isinstance(packed, PackedCrops):
            packed = pack_crops(packed, self.device)
        out = self.apply(packed, self.sample(packed))
        self.step += 1
        return out


def _workspace_bytes(packed_bytes, n_img):
    ws = L.query("dig_keyview_workspace_bytes", packed_bytes, n_img)
    if ws <= 0:
        L.check(int(ws), "dig_keyview_workspace_bytes")
    return ws


# ------------------------------------------------------------------------------------------------------------------------------------------
# ABINet augmentation of fine-tuning (--num_view 2 --use_abi_aug): transforms.py:188-504 / dataset/dataset_lmdb.py:36-47 of the reference.

# field order and sizes of struct dig_abi_params / dig_abi_run (include/dig_aug_types.h)
ABI_PARAMS_DTYPE = np.dtype([
    ("geom", "<i4"), ("det", "<i4"), ("jit", "<i4"), ("geom_interp", "<i4"), ("angle", "<f4"), ("scale", "<f4"), ("shear", "<f4", 2),
    ("persp_ow", "<i4", 4), ("persp_oh", "<i4", 4), ("h", "<i4"), ("w", "<i4"), ("wh", "<i4"), ("ww", "<i4"), ("minv", "<f4", 9),
    ("rs_interp", "<i4", 2), ("mb_k", "<f4", 25), ("jit_order", "<i4", 4), ("jit_factor", "<f4", 4), ("hue_shift", "<i4"),
    ("noise_key", "<u4", 2), ("noise_step", "<u4"), ("final_buf", "<i4"), ("pad0", "<i4"), ("ws_off", "<i8"), ("pad", "<i4", 24)])
ABI_PARAMS_WORDS = L.const("DIG_ABI_WORDS")
assert ABI_PARAMS_DTYPE.itemsize == 4 * ABI_PARAMS_WORDS
ABI_RUN_DTYPE = np.dtype([("geom_type", "<i4"), ("noise_var", "<i4"), ("mb_size", "<i4"), ("mb_angle", "<f4"), ("rescale_factor", "<i4"),
                          ("det_order", "<i4", 3)])
assert ABI_RUN_DTYPE.itemsize == 32

GEOM_NAMES = ("rotation", "affine", "perspective")
DET_NAMES = ("noise", "motion_blur", "rescale")


def draw_abi_run(seed):
    """The run parameters the reference's constructors draw once per dataset object (CVGeometry, CVGaussianNoise, CVMotionBlur,
    CVRescale, CVDeterioration's shuffle), from numpy's RandomState(seed): a record of ABI_RUN_DTYPE."""
    rs = np.random.RandomState(seed & 0xFFFFFFFF)
    r = np.zeros((), dtype=ABI_RUN_DTYPE)
    t = rs.random_sample()
    r["geom_type"] = 0 if t < 0.33 else (1 if t < 0.66 else 2)
    r["noise_var"] = max(int(rs.beta(1, 4) * 20), 1)
    r["mb_size"] = max(int(rs.beta(1, 4) * 6), 1)
    r["mb_angle"] = rs.uniform(-90, 90)
    r["rescale_factor"] = round(rs.uniform(0, 4))
    r["det_order"] = rs.permutation(3)
    return r


def abi_params_to_numpy(params):
    """Device / host table tensor (int32 [n, 96]) -> numpy structured array of ABI_PARAMS_DTYPE."""
    return params.cpu().numpy().view(ABI_PARAMS_DTYPE).reshape(-1)


def abi_params_from_numpy(table, device):
    """numpy structured array of ABI_PARAMS_DTYPE -> int32 [n, 96] tensor on `device` (a caller-built table)."""
    a = np.ascontiguousarray(np.asarray(table, dtype=ABI_PARAMS_DTYPE))
    return torch.from_numpy(a.view(np.int32).reshape(-1, ABI_PARAMS_WORDS).copy()).to(device)


class AbiAugment:
    """The fine-tune training view of a packed batch of crops, on the device: CVGeometry (p 0.5), CVDeterioration (p 0.25), CVColorJitter
    (p 0.25), Resize((out_h, out_w), BICUBIC), ToTensor, Normalize -- the reference's `--num_view 2 --use_abi_aug` transform.

    `run` holds what the reference fixes per dataset object (geometry type, noise variance, motion-blur size and angle, rescale factor,
    deterioration order), drawn from `seed` at construction; a caller may set it.  `__call__` draws the per-image tables for
    (seed, step) -- Philox4x32-10 -- runs the stages and advances its step counter.

    The warped images live in a workspace sized by the sampler (`info[0]`, one 32-byte readback per batch): with the affine scale up to 2
    and the rotation / shear canvases a warped image can hold several times the crop's pixels, and a bound from (n, max_h, max_w) alone
    would reserve that for every image."""

    def __init__(self, seed=0, device="cuda", out_h=32, out_w=128, mean=0.5, std=0.5):
        self.seed, self.step, self.device = int(seed), 0, torch.device(device)
        self.out_h, self.out_w, self.mean, self.std = out_h, out_w, mean, std
        self.run = draw_abi_run(self.seed)

    def _run_ptr(self):
        self._run_buf = np.ascontiguousarray(np.asarray(self.run, dtype=ABI_RUN_DTYPE).reshape(1))
        return ctypes.c_void_p(self._run_buf.ctypes.data)

    def sample(self, packed, step=None):
        """(int32 [n, 96] tables at (seed, step), int64 [4] info on the device: workspace bytes, max warped height / width, images with a
        workspace).  The counter is not advanced."""
        params = torch.empty((packed.n, ABI_PARAMS_WORDS), device=packed.data.device, dtype=torch.int32)
        info = torch.empty(4, device=packed.data.device, dtype=torch.int64)
        L.call("dig_abiaug_sample", L.ptr(params), L.ptr(info), L.ptr(packed.heights), L.ptr(packed.widths), packed.n, self._run_ptr(),
               ctypes.c_ulonglong(self.seed), ctypes.c_uint((self.step if step is None else step) & 0xFFFFFFFF), L.stream())
        return params, info

    def _common(self, packed, params, work):
        return (L.ptr(packed.data), L.ptr(packed.offsets), L.ptr(packed.heights), L.ptr(packed.widths), packed.n, L.ptr(params),
                self._run_ptr(), L.ptr(work) if work.numel() else None, work.numel())

    def workspace(self, info):
        """(uint8 workspace, max warped height, max warped width) for a sampler's info (one readback)."""
        total, mh, mw, _ = (int(v) for v in info.cpu())
        return torch.empty(total, device=info.device, dtype=torch.uint8), mh, mw

    def warp(self, packed, params, work, max_wh, max_ww):
        L.call("dig_abiaug_warp_u8", *self._common(packed, params, work), max(max_wh, packed.max_h), max(max_ww, packed.max_w), L.stream())

    def deteriorate(self, packed, params, work, max_wh, max_ww):
        L.call("dig_abiaug_deteriorate_u8", *self._common(packed, params, work), max(max_wh, packed.max_h), max(max_ww, packed.max_w),
               L.stream())

    def tail(self, packed, params, work, max_wh, max_ww):
        out = torch.empty((packed.n, 3, self.out_h, self.out_w), device=packed.data.device, dtype=torch.float32)
        L.call("dig_abiaug_tail", *self._common(packed, params, work), L.ptr(out), self.out_h, self.out_w, ctypes.c_float(self.mean),
               ctypes.c_float(self.std), max(max_wh, packed.max_h), max(max_ww, packed.max_w), L.stream())
        return out

    def apply(self, packed, params, info=None):
        """All stages with the given tables: fp32 [n, 3, out_h, out_w].  `info` as `sample` returns it; None: derived from the tables."""
        if info is None:
            t = abi_params_to_numpy(params)
            total = int(max((t["ws_off"] + [workspace_bytes(g, d, h, w, self.run) for g, d, h, w in zip(t["geom"], t["det"], t["wh"], t["ww"])]).max(), 0))
            info = torch.tensor([total, int(t["wh"].max()), int(t["ww"].max()), 0], dtype=torch.int64)
        work, mh, mw = self.workspace(info)
        work = work.to(packed.data.device)
        self.warp(packed, params, work, mh, mw)
        self.deteriorate(packed, params, work, mh, mw)
        return self.tail(packed, params, work, mh, mw)

    def __call__(self, packed):
        if not isinstance(packed, PackedCrops):
            packed = pack_crops(packed, self.device)
        params, info = self.sample(packed)
        out = self.apply(packed, params, info)
        self.step += 1
        return out


def workspace_bytes(geom, det, wh, ww, run):
    """Workspace bytes of one image (dig_abiaug_workspace_bytes)."""
    buf = np.ascontiguousarray(np.asarray(run, dtype=ABI_RUN_DTYPE).reshape(1))
    b = L.query("dig_abiaug_workspace_bytes", int(geom), int(det), int(wh), int(ww), ctypes.c_void_p(buf.ctypes.data))
    if b < 0:
        L.check(int(b), "dig_abiaug_workspace_bytes")
    return b
