"""Device time of the ABINet augmentation (dig_amd/augment.py AbiAugment) on 256 crops of two size classes: the sampler, the warp, the
deterioration launches, the tail, and sampler + all stages together (the readback of the workspace size included), each timed with events
over 30 calls after warm-up, next to the plain resize of the same crops.  One JSON line per class (and per geometry type of the run);
`--out FILE` writes them there as well.

    python tools/gpu_abiaug_probe.py [--out abiaug_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dig_amd.augment import AbiAugment, abi_params_to_numpy, pack_crops  # noqa: E402
from dig_amd.datasets import resize_normalize  # noqa: E402


def timed(fn, reps=30, warm=3):
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
    ap.add_argument("--n", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_abiaug_probe: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    lines = []
    for name, hh, ww in (("32x100..64x320", (32, 64), (100, 320)), ("100x300..200x700", (100, 200), (300, 700))):
        crops = [rng.randint(0, 256, size=(rng.randint(*hh), rng.randint(*ww), 3)).astype(np.uint8) for _ in range(args.n)]
        pk = pack_crops(crops, dev)
        for gt in range(3):
            aug = AbiAugment(1, dev)
            aug.run["geom_type"], aug.run["rescale_factor"] = gt, 2
            params, info = aug.sample(pk)
            work, mh, mw = aug.workspace(info)
            t = abi_params_to_numpy(params)
            rec = {"class": name, "crops": pk.n, "run": {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in
                                                       zip(aug.run.dtype.names, aug.run.tolist())},
                   "workspace_mb": round(work.numel() / 1e6, 2), "max_warped": [mh, mw],
                   "gates": [int(t["geom"].sum()), int(t["det"].sum()), int(t["jit"].sum())],
                   "sample_us": round(timed(lambda: aug.sample(pk)), 1),
                   "warp_us": round(timed(lambda: aug.warp(pk, params, work, mh, mw)), 1),
                   "deteriorate_us": round(timed(lambda: aug.deteriorate(pk, params, work, mh, mw)), 1),
                   "tail_us": round(timed(lambda: aug.tail(pk, params, work, mh, mw)), 1),
                   "total_us": round(timed(lambda: aug.apply(pk, *aug.sample(pk))), 1),
                   "plain_resize_us": round(timed(lambda: resize_normalize(pk)), 1)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
