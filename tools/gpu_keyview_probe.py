"""Device time of the key-view augmentation (dig_amd/augment.py) on 128 crops of the two size classes of tools/gpu_input_probe.py: the
sampler, stage A (5 launches), stage B, and the three together, each timed with events over 50 calls after warm-up (buffers already on
the device), next to the plain resize of the first view for scale.  One JSON line per class; `--out FILE` writes them there as well.

    python tools/gpu_keyview_probe.py [--out keyview_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dig_amd import _lib as L  # noqa: E402
from dig_amd.augment import KeyViewAugment, _workspace_bytes, pack_crops  # noqa: E402
from dig_amd.datasets import resize_normalize  # noqa: E402


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3                      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_keyview_probe: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    lines = []
    for name, hh, ww in (("32x100..64x320", (32, 64), (100, 320)), ("100x300..200x700", (100, 200), (300, 700))):
        crops = [rng.randint(0, 256, size=(rng.randint(*hh), rng.randint(*ww), 3)).astype(np.uint8) for _ in range(args.n)]
        pk = pack_crops(crops, dev)
        aug = KeyViewAugment(1, dev)
        params = aug.sample(pk)
        ws = _workspace_bytes(pk.data.numel(), pk.n)
        work = torch.empty(ws, device=dev, dtype=torch.uint8)
        out = torch.empty((pk.n, 3, 32, 128), device=dev)

        def sample():
            L.call("dig_keyview_sample", L.ptr(params), L.ptr(pk.heights), L.ptr(pk.widths), pk.n, ctypes.c_ulonglong(1), ctypes.c_uint(0),
                   L.stream())

        def stage_a():
            L.call("dig_keyview_stage_a_u8", L.ptr(pk.data), L.ptr(pk.offsets), L.ptr(pk.heights), L.ptr(pk.widths), pk.n, L.ptr(params),
                   L.ptr(work), ws, pk.max_h, pk.max_w, L.stream())

        def stage_b():
            L.call("dig_keyview_stage_b", L.ptr(work), L.ptr(pk.offsets), L.ptr(pk.heights), L.ptr(pk.widths), pk.n, L.ptr(params), L.ptr(out),
                   32, 128, ctypes.c_float(0.5), ctypes.c_float(0.5), pk.max_h, pk.max_w, L.stream())

        def all3():
            sample()
            stage_a()
            stage_b()
        rec = {"class": name, "crops": pk.n, "mb_uint8": round(pk.data.numel() / 1e6, 2),
               "sample_us": round(timed(sample), 1), "stage_a_us": round(timed(stage_a), 1), "stage_b_us": round(timed(stage_b), 1),
               "total_us": round(timed(all3), 1), "first_view_resize_us": round(timed(lambda: resize_normalize(pk)), 1),
               "ops_per_image_mean": float(params[:, 0].float().mean())}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
