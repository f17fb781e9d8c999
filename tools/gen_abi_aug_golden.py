"""Write tests/golden/abi_aug_tail.npz: the tail of the ABINet augmentation as Pillow computes it, called the way torchvision's PIL path
calls it -- ColorJitter(0.5, 0.5, 0.5, 0.1) at the image's own resolution (adjust_* = ImageEnhance.*.enhance / the HSV round trip of
F_pil.adjust_hue), then transforms.Resize((32, 128), BICUBIC).  The crops stand in for warped images (sizes from the canvases the
geometry gives: taller, wider and smaller than the crops); the fixture holds them and the uint8 results, so the tests need no Pillow.

    python tools/gen_abi_aug_golden.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
from gen_key_view_golden import adjust_hue  # noqa: E402


def tail(crop, order, factors):
    img = Image.fromarray(crop, "RGB")
    f = [float(np.float32(x)) for x in factors]                    # the table holds float32 factors
    for k in order:
        if k == 0:
            img = ImageEnhance.Brightness(img).enhance(f[0])
        elif k == 1:
            img = ImageEnhance.Contrast(img).enhance(f[1])
        elif k == 2:
            img = ImageEnhance.Color(img).enhance(f[2])
        elif k == 3:
            img = adjust_hue(img, f[3])
    return np.asarray(img.resize((128, 32), Image.BICUBIC), dtype=np.uint8)


def main():
    rng = np.random.RandomState(20261016)
    sizes = [(32, 128), (45, 170), (80, 150), (16, 60), (70, 200), (33, 129), (9, 40), (64, 64), (50, 260), (32, 128)]
    cases = [([0], [0.55, 1, 1, 0]), ([1], [1, 1.45, 1, 0]), ([2], [1, 1, 0.52, 0]), ([3], [1, 1, 1, -0.093]), ([1], [1, 0.51, 1, 0])]
    out = {"n_cases": np.array([len(sizes)])}
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        base = np.stack([np.sin(6.3 * (xx * rng.rand() + yy * rng.rand()) + rng.rand() * 6) for _ in range(3)], -1) * 110 + 128
        crop = np.clip(base + rng.randn(h, w, 3) * 18, 0, 255).astype(np.uint8)
        if i < len(cases):
            order, factors = cases[i]
        else:
            order = list(rng.permutation(4))
            factors = [0.5 + rng.rand(), 0.5 + rng.rand(), 0.5 + rng.rand(), -0.1 + 0.2 * rng.rand()]
        out[f"crop_{i}"] = crop
        out[f"out_{i}"] = tail(crop, order, factors)
        out[f"order_{i}"] = np.array(list(order) + [-1] * (4 - len(order)), np.int32)
        out[f"factors_{i}"] = np.array(factors, np.float32)
    path = os.path.join(ROOT, "tests", "golden", "abi_aug_tail.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
