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
PARAMS_WORDS = 128
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
    f = L.lib().dig_keyview_workspace_bytes
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_longlong, ctypes.c_int]
    ws = f(packed_bytes, n_img)
    if ws <= 0:
        L.check(int(ws), "dig_keyview_workspace_bytes")
    return ws
