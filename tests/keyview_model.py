"""Numpy statement of the key-view augmentation (dig_amd/csrc/keyview.inc): both stages, given a parameter table (dig_amd.augment.PARAMS_DTYPE).
This is the spec the device kernels are tested against.  Per-pixel arithmetic is float32 in the kernel's operation order (numpy float32
arithmetic is IEEE without contraction, as the kernels are compiled); Pillow's HSV conversions mix float and double as its C source does.

    table(H, W, n_ops=..., ops=[...], **raw)   a table with the derived coefficients computed from the raw parameters for an H x W crop
    stage_a(img, P) / op(img, k, P)            seqCLR ops at the crop's resolution (uint8 -> uint8)
    stage_b(img, P, out_h, out_w)              Pillow bicubic resize, ColorJitter ops, RandomGrayscale, ToTensor + Normalize -> fp32 [3, h, w]
"""
import math

import numpy as np

import input_oracle as IO
from dig_amd.augment import PARAMS_DTYPE

f32 = np.float32
MAX_TAPS = 11


# ----------------------------------------------------------------------------------------------------------------------------- tables
def identity_table():
    t = np.zeros((), dtype=PARAMS_DTYPE)
    t["ops"] = -1
    t["contrast_alpha"], t["blur_sigma"], t["pa_scale"], t["persp_sigma"], t["solar_tau"] = 1.0, 0.5, 0.03, 0.05, 128.0
    t["jit_order"] = [0, 1, 2, 3]
    t["jit_factor"] = [1.0, 1.0, 1.0, 0.0]
    return t


def derive(t, H, W):
    """Fill the derived coefficients of table `t` from its raw parameters for an H x W crop (keyview.inc sample_one, in double)."""
    sg = float(t["blur_sigma"])
    r = int(math.ceil(3.0 * sg))
    e = [math.exp(-float(d * d) / (2.0 * sg * sg)) for d in range(-r, r + 1)]
    s = sum(e)
    taps = np.zeros(MAX_TAPS, np.float32)
    taps[:2 * r + 1] = [v / s for v in e]
    t["blur_radius"], t["blur_taps"] = r, taps
    sa, sl = float(t["sharpen_alpha"]), float(t["sharpen_lightness"])
    k = np.full(9, -sa)
    k[4] = (1.0 - sa) + sa * (8.0 + sl)
    t["sharpen_k"] = k.astype(np.float32)

    def window(p0, p1, n):
        a, b = int(math.floor(float(p0) * n + 0.5)), int(math.floor(float(p1) * n + 0.5))
        if n - a - b < 1:
            b = n - 1 - a
            if b < 0:
                a, b = n - 1, 0
        return [a, n - a - b]
    t["crop_y"] = window(t["crop_tb"][0], t["crop_tb"][1], H)
    t["crop_x"] = window(t["crop_lr"][0], t["crop_lr"][1], W)
    th = float(t["rotate_deg"]) * 3.141592653589793 / 180.0
    c, s_ = math.cos(th), math.sin(th)
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    t["rot"] = np.array([c, s_, cx - c * cx - s_ * cy, -s_, c, cy + s_ * cx - c * cy], np.float32)
    d = [float(v) for v in t["persp_d"]]
    w1, h1 = float(W - 1), float(H - 1)
    x0, y0 = d[0] * W, d[1] * H
    x1, y1 = w1 - d[2] * W, d[3] * H
    x2, y2 = w1 - d[4] * W, h1 - d[5] * H
    x3, y3 = d[6] * W, h1 - d[7] * H
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    if W < 2 or H < 2 or abs(den) < 1e-9:
        t["homog"] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    else:
        g, h = (sx * dy2 - dx2 * sy) / den, (dx1 * sy - sx * dy1) / den
        t["homog"] = np.array([(x1 - x0 + g * x1) / w1, (x3 - x0 + h * x3) / h1, x0, (y1 - y0 + g * y1) / w1, (y3 - y0 + h * y3) / h1, y0,
                               g / w1, h / h1, 1.0], np.float32)
    t["hue_shift"] = int(float(t["jit_factor"][3]) * 255.0) % 256
    return t


def table(H, W, ops=(), **fields):
    """A hand-built table for an H x W crop: `ops` in order, raw fields as keywords (others at identity_table's values)."""
    t = identity_table()
    t["n_ops"] = len(ops)
    t["ops"] = list(ops) + [-1] * (5 - len(ops))
    for k, v in fields.items():
        t[k] = v
    return derive(t, H, W)


# ----------------------------------------------------------------------------------------------------------------------------- stage A
def round_u8(t):
    r = np.floor(t + f32(0.5))
    return np.clip(r, 0, 255).astype(np.uint8)


def refl101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def luma(r, g, b):
    return (19595 * r.astype(np.int64) + 38470 * g.astype(np.int64) + 7471 * b.astype(np.int64) + 0x8000) >> 16


def cubic_coeffs(x):
    A = f32(-0.75)
    one = f32(1)
    w0 = ((A * (x + one) - f32(5) * A) * (x + one) + f32(8) * A) * (x + one) - f32(4) * A
    w1 = ((A + f32(2)) * x - (A + f32(3))) * x * x + one
    w2 = ((A + f32(2)) * (one - x) - (A + f32(3))) * (one - x) * (one - x) + one
    w3 = one - w0 - w1 - w2
    return w0, w1, w2, w3


def bilinear(img, sx, sy, zero):
    H, W = img.shape[:2]
    sx = np.fmin(np.fmax(sx, f32(-2)), f32(W + 1))
    sy = np.fmin(np.fmax(sy, f32(-2)), f32(H + 1))
    xf, yf = np.floor(sx), np.floor(sy)
    fx, fy = sx - xf, sy - yf
    gx, gy = f32(1) - fx, f32(1) - fy
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    v = img.astype(np.float32)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        val = v[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(inside[..., None], val, f32(0)) if zero else val
    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    gx, fx, gy, fy = gx[..., None], fx[..., None], gy[..., None], fy[..., None]
    top = v00 * gx + v01 * fx
    bot = v10 * gx + v11 * fx
    return round_u8(top * gy + bot * fy)


def op(img, k, P):
    """Op k of the table on an H x W x 3 uint8 image."""
    H, W = img.shape[:2]
    v = img.astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx, fy = xx.astype(np.float32), yy.astype(np.float32)
    if k == 0:
        return round_u8(f32(127.5) + f32(P["contrast_alpha"]) * (v - f32(127.5)))
    if k == 1:
        r = int(np.clip(P["blur_radius"], 0, (MAX_TAPS - 1) // 2))
        taps = P["blur_taps"].astype(np.float32)
        acc = np.zeros_like(v)
        for j in range(-r, r + 1):
            rows = v[refl101(np.arange(H) + j, H)]
            h = np.zeros_like(v)
            for i in range(-r, r + 1):
                h = h + taps[r + i] * rows[:, refl101(np.arange(W) + i, W)]
            acc = acc + taps[r + j] * h
        return round_u8(acc)
    if k in (2, 3):
        rows = k == 2
        n = H if rows else W
        win = P["crop_y"] if rows else P["crop_x"]
        first = int(np.clip(win[0], 0, n - 1))
        ln = int(np.clip(win[1], 1, n - first))
        idx = np.arange(n).astype(np.float32)
        s = (idx + f32(0.5)) * (f32(ln) / f32(n)) - f32(0.5)
        sf = np.floor(s)
        w = cubic_coeffs(s - sf)
        i0 = sf.astype(np.int64) - 1
        acc = np.zeros_like(v)
        for q in range(4):
            i = first + np.clip(i0 + q, 0, ln - 1)
            if rows:
                acc = acc + w[q][:, None, None] * v[i]
            else:
                acc = acc + w[q][None, :, None] * v[:, i]
        return round_u8(acc)
    if k == 4:
        kk = P["sharpen_k"].astype(np.float32)
        acc = np.zeros_like(v)
        for dy in (-1, 0, 1):
            rows = v[refl101(np.arange(H) + dy, H)]
            for dx in (-1, 0, 1):
                acc = acc + kk[(dy + 1) * 3 + dx + 1] * rows[:, refl101(np.arange(W) + dx, W)]
        return round_u8(acc)
    if k == 5:
        m = P["rot"].astype(np.float32)
        return bilinear(img, (m[0] * fx + m[1] * fy) + m[2], (m[3] * fx + m[4] * fy) + m[5], True)
    if k == 6:
        u = (fx * f32(3)) / f32(W - 1) if W > 1 else np.zeros_like(fx)
        w = (fy * f32(3)) / f32(H - 1) if H > 1 else np.zeros_like(fy)
        ci = np.where(u < 2, u.astype(np.int64), 2)
        ri = np.where(w < 2, w.astype(np.int64), 2)
        u = u - ci.astype(np.float32)
        w = w - ri.astype(np.float32)
        k00 = ri * 4 + ci

        def disp(d):
            d = d.astype(np.float32)
            upper = (d[k00] + u * (d[k00 + 1] - d[k00])) + w * (d[k00 + 5] - d[k00 + 1])
            lower = (d[k00] + w * (d[k00 + 4] - d[k00])) + u * (d[k00 + 5] - d[k00 + 4])
            return np.where(u >= w, upper, lower)
        return bilinear(img, fx + disp(P["pa_dx"]), fy + disp(P["pa_dy"]), False)
    if k == 7:
        h = P["homog"].astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = (h[6] * fx + h[7] * fy) + h[8]
            sx = ((h[0] * fx + h[1] * fy) + h[2]) / den
            sy = ((h[3] * fx + h[4] * fy) + h[5]) / den
        return bilinear(img, sx, sy, True)
    if k == 8:
        tau = f32(P["solar_tau"])
        inv = (v >= tau) if P["solar_above"] else (v < tau)
        return np.where(inv, 255 - img.astype(np.int64), img).astype(np.uint8)
    if k == 9:
        a = f32(P["gray_alpha"])
        b = f32(1) - a
        g = luma(img[..., 0], img[..., 1], img[..., 2]).astype(np.float32)[..., None]
        return round_u8(b * v + a * g)
    return img.copy()


def stage_a(img, P):
    for k in P["ops"][:int(np.clip(P["n_ops"], 0, 5))]:
        img = op(img, int(k), P)
    return img


# ----------------------------------------------------------------------------------------------------------------------------- stage B
def blend(d, v, f):
    t = np.asarray(d).astype(np.float32) + f32(f) * (v.astype(np.int64) - d).astype(np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.int64)


def _round_half_away(x):
    fl = np.floor(x)
    return np.where(x - fl >= 0.5, fl + 1, fl)


def rgb2hsv(r, g, b):
    """Pillow's rgb2hsv_row on int arrays -> (h, s, v) int arrays."""
    r, g, b = (np.asarray(a, np.int64) for a in (r, g, b))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    same = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(np.float32)
        s = cr / maxc.astype(np.float32)
        rc = (maxc - r).astype(np.float32) / cr
        gc = (maxc - g).astype(np.float32) / cr
        bc = (maxc - b).astype(np.float32) / cr
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, ((2.0 + rc.astype(np.float64)) - bc.astype(np.float64)).astype(np.float32),
                              ((4.0 + gc.astype(np.float64)) - rc.astype(np.float64)).astype(np.float32)))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        uh = np.clip(np.trunc(h.astype(np.float64) * 255.0), 0, 255)
        us = np.clip(np.trunc(s.astype(np.float64) * 255.0), 0, 255)
    uh = np.where(same, 0, np.nan_to_num(uh)).astype(np.int64)
    us = np.where(same, 0, np.nan_to_num(us)).astype(np.int64)
    return uh, us, maxc


def hsv2rgb(h, s, v):
    """Pillow's hsv2rgb on int arrays -> (r, g, b) int arrays."""
    h, s, v = (np.asarray(a, np.int64) for a in (h, s, v))
    hd = h.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(hd).astype(np.int64)
    f = (hd - i.astype(np.float32).astype(np.float64)).astype(np.float32)
    fs = (s.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32)
    vd = v.astype(np.float32).astype(np.float64)
    p = np.clip(_round_half_away(vd * (1.0 - fs.astype(np.float64))), 0, 255).astype(np.int64)
    q = np.clip(_round_half_away(vd * (1.0 - (fs * f).astype(np.float64))), 0, 255).astype(np.int64)
    t = np.clip(_round_half_away(vd * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64)))), 0, 255).astype(np.int64)
    sel = i % 6
    r = np.choose(sel, [v, q, p, p, t, v])
    g = np.choose(sel, [t, v, v, q, p, p])
    b = np.choose(sel, [p, p, t, v, v, q])
    z = s == 0
    return np.where(z, v, r), np.where(z, v, g), np.where(z, v, b)


def jitter_op(img, k, P):
    """Jitter op k (0 brightness, 1 contrast, 2 saturation, 3 hue) on an int H x W x 3 image."""
    f = P["jit_factor"][k]
    if k == 0:
        return blend(0, img, f)
    if k == 1:
        m = int(float(luma(img[..., 0], img[..., 1], img[..., 2]).sum()) / (img.shape[0] * img.shape[1]) + 0.5)
        return blend(m, img, f)
    if k == 2:
        return blend(luma(img[..., 0], img[..., 1], img[..., 2])[..., None], img, f)
    h, s, v = rgb2hsv(img[..., 0], img[..., 1], img[..., 2])
    return np.stack(hsv2rgb((h + int(P["hue_shift"])) & 255, s, v), -1)


def stage_b_u8(img, P, out_h=32, out_w=128):
    x = IO.resize_bicubic_u8(img, out_h, out_w).astype(np.int64)
    if P["jitter"]:
        for k in P["jit_order"]:
            if 0 <= k <= 3:                             # (entries outside 0..3 are skipped: hand-built tables)
                x = jitter_op(x, int(k), P)
    if P["gray"]:
        x = np.repeat(luma(x[..., 0], x[..., 1], x[..., 2])[..., None], 3, -1)
    return x.astype(np.uint8)


def stage_b(img, P, out_h=32, out_w=128):
    return IO.to_tensor_normalize(stage_b_u8(img, P, out_h, out_w))


def key_view(img, P, out_h=32, out_w=128):
    return stage_b(stage_a(img, P), P, out_h, out_w)


# ----------------------------------------------------------------------------------------------------------------------------- golden
def golden_crops():
    """The crops of tests/golden/key_view_tail.npz (tools/gen_key_view_golden.py): smooth colour fields with noise, from a fixed seed."""
    rng = np.random.RandomState(20261015)
    sizes = [(32, 128), (32, 128), (20, 90), (57, 211), (32, 128), (9, 300), (64, 64), (32, 128), (45, 160), (32, 128), (28, 100), (70, 240)]
    crops = []
    for h, w in sizes:
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        base = np.stack([np.sin(6.3 * (xx * rng.rand() + yy * rng.rand()) + rng.rand() * 6) for _ in range(3)], -1) * 110 + 128
        crops.append(np.clip(base + rng.randn(h, w, 3) * 18, 0, 255).astype(np.uint8))
    return crops


def golden_cases():
    """[(jitter, order, factors, gray)] per golden crop: every jitter op alone (both directions), sampled orders, grayscale."""
    rng = np.random.RandomState(7)
    cases = [(1, [0], [0.6, 1, 1, 0]), (1, [0], [1.37, 1, 1, 0]), (1, [1], [1, 0.63, 1, 0]), (1, [1], [1, 1.38, 1, 0]),
             (1, [2], [1, 1, 0.81, 0]), (1, [2], [1, 1, 1.19, 0]), (1, [3], [1, 1, 1, -0.093]), (1, [3], [1, 1, 1, 0.071])]
    out = [(j, o, f, 0) for j, o, f in cases]
    for i in range(len(golden_crops()) - len(out)):
        f = [0.6 + 0.8 * rng.rand(), 0.6 + 0.8 * rng.rand(), 0.8 + 0.4 * rng.rand(), -0.1 + 0.2 * rng.rand()]
        out.append((1, list(rng.permutation(4)), f, int(i % 2)))
    return out
