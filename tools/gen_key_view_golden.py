"""Write tests/golden/key_view_tail.npz: stage B of the key-view augmentation as Pillow computes it, called the way torchvision's PIL path
calls it (transforms.Resize((32, 128), BICUBIC), ColorJitter's adjust_* = ImageEnhance.*.enhance / the HSV round trip of F_pil.adjust_hue,
RandomGrayscale = convert("L") replicated).  The crops and the cases come from tests/keyview_model.py (golden_crops / golden_cases, fixed
seeds); the fixture holds the uint8 results, so the tests need no Pillow.

    python tools/gen_key_view_golden.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import keyview_model as M  # noqa: E402


def adjust_hue(img, hue):
    # torchvision F_pil.adjust_hue: H channel += uint8(hue * 255) with wrap-around (the truncated value mod 256), back to RGB
    h, s, v = img.convert("HSV").split()
    np_h = (np.array(h, dtype=np.int64) + int(float(np.float32(hue)) * 255.0) % 256) % 256
    return Image.merge("HSV", (Image.fromarray(np_h.astype(np.uint8), "L"), s, v)).convert("RGB")


def tail(crop, order, factors, gray):
    img = Image.fromarray(crop, "RGB").resize((128, 32), Image.BICUBIC)
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
    if gray:
        img = img.convert("L").convert("RGB")                      # (L replicated: what np.dstack([L] * 3) gives)
    return np.asarray(img, dtype=np.uint8)


def main():
    crops, cases = M.golden_crops(), M.golden_cases()
    out = {"n_cases": np.array([len(cases)])}
    for i, (crop, (jit, order, factors, gray)) in enumerate(zip(crops, cases)):
        out[f"out_{i}"] = tail(crop, order if jit else [], factors, gray)
        out[f"order_{i}"] = np.array(list(order) + [-1] * (4 - len(order)), np.int32)
        out[f"factors_{i}"] = np.array(factors, np.float32)
        out[f"flags_{i}"] = np.array([jit, gray], np.int32)
    path = os.path.join(ROOT, "tests", "golden", "key_view_tail.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
