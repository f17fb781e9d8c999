"""Numpy statement of the ABINet augmentation of fine-tuning (dig_amd/csrc/abiaug.inc), given a table (dig_amd.augment.ABI_PARAMS_DTYPE)
and a run (ABI_RUN_DTYPE).  The spec the device kernels are tested against: integer resamplers, float32 coordinates / blur sums in the
kernels' operation order (numpy float32 arithmetic is IEEE without contraction), the noise in double (Python floats).

    canvas(P, H, W, geom_type)          the warped size, restated from the reference's formulas with math / numpy trigonometry
    warp(img, P) / noise(img, P, i, var) / blur(img, P, d) / resize_cv(img, h, w, interp) / pyrdown(img) / rescale(img, P, factor)
    deteriorate(img, P, run, i)         the run's ops in its order
    tail(img, P, out_h, out_w)          ColorJitter at the image's resolution, Pillow bicubic resize, ToTensor + Normalize
    augment(img, P, run, i)             everything
    layout(tables, run)                 final_buf / ws_off of each table (what the sampler writes)
"""
import math

import numpy as np

import input_oracle as IO
import keyview_model as KM

f32 = np.float32
RS_H, RS_W = 128, 512
RS_BYTES = 3 * RS_H * RS_W + 3 * (RS_H // 2) * (RS_W // 2)


# ------------------------------------------------------------------------------------------------------------------------------- layout
def round256(b):
    return (b + 255) // 256 * 256


def image_bytes(geom, det, wh, ww, factor):
    if not geom and not det:
        return 0
    rb = round256(3 * wh * ww)
    return 2 * rb + (RS_BYTES if factor > 0 else 0) if det else rb


def det_ops(run):
    return [int(o) for o in run["det_order"] if not (o == 2 and run["rescale_factor"] <= 0)]


def layout(tables, run):
    off = 0
    for P in tables:
        n = len(det_ops(run))
        P["final_buf"] = (2 if n % 2 else 1) if P["det"] else (1 if P["geom"] else 0)
        P["ws_off"] = off
        off += image_bytes(P["geom"], P["det"], P["wh"], P["ww"], run["rescale_factor"])
    return off


# ------------------------------------------------------------------------------------------------------------------------------- canvas
def min_area_box(px, py):
    """Minimum-area rectangle of four points in order (rotating calipers over the four edges, the first minimal edge wins) -> truncated
    (min_x, min_y, max_x, max_y) of its corners."""
    best, bx, by = -1.0, [px[0]] * 4, [py[0]] * 4
    for e in range(4):
        ex, ey = px[(e + 1) % 4] - px[e], py[(e + 1) % 4] - py[e]
        ln = math.sqrt(ex * ex + ey * ey)
        if ln == 0.0:
            continue
        ux, uy = ex / ln, ey / ln
        vx, vy = -uy, ux
        su = [(px[k] - px[e]) * ux + (py[k] - py[e]) * uy for k in range(4)]
        sv = [(px[k] - px[e]) * vx + (py[k] - py[e]) * vy for k in range(4)]
        u0, u1, v0, v1 = min(0.0, *su), max(0.0, *su), min(0.0, *sv), max(0.0, *sv)
        area = (u1 - u0) * (v1 - v0)
        if best < 0 or area < best:
            best = area
            bx = [(px[e] + cu * ux) + cv * vx for cu, cv in ((u0, v0), (u1, v0), (u1, v1), (u0, v1))]
            by = [(py[e] + cu * uy) + cv * vy for cu, cv in ((u0, v0), (u1, v0), (u1, v1), (u0, v1))]
    xs, ys = [int(v) for v in bx], [int(v) for v in by]
    return min(xs), min(ys), max(xs), max(ys)


def canvas(P, H, W, geom_type):
    """(warped height, width) by the reference's formulas (transforms.py CVRandomRotation / CVRandomAffine / CVRandomPerspective)."""
    if geom_type == 0:
        a = math.radians(float(P["angle"]))
        abs_cos, abs_sin = abs(math.cos(a)), abs(math.sin(a))
        dw, dh = int(H * abs_sin + W * abs_cos), int(H * abs_cos + W * abs_sin)
    elif geom_type == 1:
        rot, sx, sy = math.radians(float(P["angle"])), math.radians(float(P["shear"][0])), math.radians(float(P["shear"][1]))
        cx, cy, scale = W / 2, H / 2, float(P["scale"])
        a = math.cos(rot - sy) / math.cos(sy)
        b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
        c = math.sin(rot - sy) / math.cos(sy)
        d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
        M = [x / scale for x in [d, -b, 0, -c, a, 0]]
        M[2] += M[0] * (-cx) + M[1] * (-cy)
        M[5] += M[3] * (-cx) + M[4] * (-cy)
        M[2] += cx
        M[5] += cy
        pts = [(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)]
        ex = [float(int(M[0] * x + M[1] * y + M[2])) for x, y in pts]
        ey = [float(int(M[3] * x + M[4] * y + M[5])) for x, y in pts]
        x0, y0, x1, y1 = min_area_box(ex, ey)
        dw, dh = x1 - x0, y1 - y0
    else:
        ow, oh = [int(v) for v in P["persp_ow"]], [int(v) for v in P["persp_oh"]]
        ex = [float(ow[0]), float(W - 1 - ow[1]), float(W - 1 - ow[2]), float(ow[3])]
        ey = [float(oh[0]), float(oh[1]), float(H - 1 - oh[2]), float(H - 1 - oh[3])]
        x0, y0, x1, y1 = min_area_box(ex, ey)
        x0, y0 = max(x0, 0), max(y0, 0)
        dw, dh = x1 - x0, y1 - y0
    return max(dh, 1), max(dw, 1)


# ------------------------------------------------------------------------------------------------------------------------------- resamplers
def _sat22(acc):
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def _round2048(w):
    return int(np.floor(f32(w) * f32(2048) + f32(0.5)))


def _warp_taps(s, n, interp):
    """Per-pixel (first index, [weights]) arrays of one warp axis."""
    s = np.fmin(np.fmax(s, f32(-4)), f32(n + 3))
    q = np.floor(s * f32(32) + f32(0.5)).astype(np.int64)
    if interp == 0:
        return (q + 16) >> 5, [np.full(q.shape, 2048, np.int64)]
    f = q & 31
    if interp == 2:
        c = KM.cubic_coeffs(f.astype(np.float32) * f32(1 / 32))
        return (q >> 5) - 1, [np.floor(ci * f32(2048) + f32(0.5)).astype(np.int64) for ci in c]
    return q >> 5, [(32 - f) * 64, f * 64]


def warp(img, P):
    H, W = img.shape[:2]
    wh, ww = int(P["wh"]), int(P["ww"])
    m = P["minv"].astype(np.float32)
    y, x = np.meshgrid(np.arange(wh, dtype=np.float32), np.arange(ww, dtype=np.float32), indexing="ij")
    den = (m[6] * x + m[7] * y) + m[8]
    sx, sy = ((m[0] * x + m[1] * y) + m[2]) / den, ((m[3] * x + m[4] * y) + m[5]) / den
    interp = 1 if P["geom_interp"] == 3 else int(np.clip(P["geom_interp"], 0, 2))
    x0, wx = _warp_taps(sx, W, interp)
    y0, wy = _warp_taps(sy, H, interp)
    v = img.astype(np.int64)
    acc = np.zeros((wh, ww, 3), np.int64)
    for j, wyj in enumerate(wy):
        for i, wxi in enumerate(wx):
            acc += (wyj * wxi)[..., None] * v[np.clip(y0 + j, 0, H - 1), np.clip(x0 + i, 0, W - 1)]
    return _sat22(acc)


def _resize_axis(interp, box, n, m):
    """Dense int64 [m, n] weight matrix of one axis of cv2.resize (abiaug.inc resize_taps)."""
    Wt = np.zeros((m, n), np.int64)
    scale = n / m
    for x in range(m):
        if interp == 0:
            Wt[x, min(max(int(math.floor(x * scale)), 0), n - 1)] += 2048
        elif interp == 3 and box:
            fsx1 = x * scale
            fsx2 = fsx1 + scale
            cell = min(scale, n - fsx1)
            sx1, sx2 = int(math.ceil(fsx1)), int(math.floor(fsx2))
            if sx1 - fsx1 > 1e-3:
                Wt[x, min(max(sx1 - 1, 0), n - 1)] += _round2048(f32((sx1 - fsx1) / cell))
            for s in range(sx1, min(sx2, n)):
                Wt[x, s] += _round2048(f32(1.0 / cell))
            if fsx2 - sx2 > 1e-3 and sx2 < n:
                Wt[x, sx2] += _round2048(f32(min(fsx2 - sx2, 1.0, cell) / cell))
        else:
            if interp == 3:
                sx = int(math.floor(x * scale))
                f = f32((x + 1) - (sx + 1) / scale)
                f = f32(0) if f <= 0 else f32(f - np.floor(f))
            else:
                s = f32((x + 0.5) * scale - 0.5)
                sx = int(np.floor(s))
                f = f32(s - f32(sx))
            if interp == 2:
                for k, c in enumerate(KM.cubic_coeffs(f)):
                    Wt[x, min(max(sx - 1 + k, 0), n - 1)] += _round2048(c)
                continue
            if sx < 0:
                f, sx = f32(0), 0
            if sx >= n - 1:
                f, sx = f32(0), n - 1
            Wt[x, sx] += _round2048(f32(1) - f)
            Wt[x, min(sx + 1, n - 1)] += _round2048(f)
    return Wt


def resize_cv(img, dh, dw, interp):
    sh, sw = img.shape[:2]
    interp = int(np.clip(interp, 0, 3))
    box = interp == 3 and sh >= dh and sw >= dw
    Wy, Wx = _resize_axis(interp, box, sh, dh), _resize_axis(interp, box, sw, dw)
    acc = np.einsum("yi,ijc->yjc", Wy, np.einsum("xj,ijc->ixc", Wx, img.astype(np.int64)))
    return _sat22(acc)


def pyrdown(img):
    sh, sw = img.shape[:2]
    k = np.array([1, 4, 6, 4, 1], np.int64)
    oh, ow = (sh + 1) // 2, (sw + 1) // 2
    v = img.astype(np.int64)
    ry = np.stack([KM.refl101(2 * np.arange(oh) + j - 2, sh) for j in range(5)])      # [5, oh]
    rx = np.stack([KM.refl101(2 * np.arange(ow) + i - 2, sw) for i in range(5)])
    acc = np.zeros((oh, ow, 3), np.int64)
    for j in range(5):
        for i in range(5):
            acc += k[j] * k[i] * v[ry[j][:, None], rx[i][None, :]]
    return ((acc + 128) >> 8).astype(np.uint8)


def rescale(img, P, factor):
    if factor <= 0:
        return img
    x = resize_cv(img, RS_H, RS_W, int(P["rs_interp"][0]))
    for _ in range(factor):
        x = pyrdown(x)
    return resize_cv(x, img.shape[0], img.shape[1], int(P["rs_interp"][1]))


def blur(img, P, d):
    H, W = img.shape[:2]
    a = d // 2
    k = P["mb_k"].astype(np.float32)
    v = img.astype(np.float32)
    acc = np.zeros((H, W, 3), np.float32)
    for j in range(d):
        ry = KM.refl101(np.arange(H) + j - a, H)
        for i in range(d):
            rx = KM.refl101(np.arange(W) + i - a, W)
            acc = acc + k[j * d + i] * v[ry[:, None], rx[None, :]]
    return KM.round_u8(acc)


# ------------------------------------------------------------------------------------------------------------------------------- noise
def _sincos_poly(x):
    x2 = x * x
    ps = pc = 0.0
    for n in range(12, 0, -1):
        ps = 1.0 - ps * x2 / float((2 * n) * (2 * n + 1))
        pc = 1.0 - pc * x2 / float((2 * n - 1) * (2 * n))
    return x * ps, pc


def _cos2pi(u):
    a = 4.0 * u
    q = int(math.floor(a))
    s, c = _sincos_poly((a - q) * 1.5707963267948966)
    return (c, -s, -c, s)[q]


def _log(x):
    m, e = math.frexp(x)
    z = (m - 1.0) / (m + 1.0)
    z2 = z * z
    p = 0.0
    for k in range(30, -1, -1):
        p = 1.0 / float(2 * k + 1) + z2 * p
    return float(e) * 0.6931471805599453 + 2.0 * z * p


def noise(img, P, i, var):
    flat = img.reshape(-1)
    out = np.empty_like(flat)
    key = (int(P["noise_key"][0]), int(P["noise_key"][1]))
    sd = math.sqrt(float(max(var, 0)))
    for e in range(flat.size):
        b1 = IO.philox4x32_10((i, int(P["noise_step"]), 2 * e, 0x41424E5A), key)[0]
        b2 = IO.philox4x32_10((i, int(P["noise_step"]), 2 * e + 1, 0x41424E5A), key)[0]
        u1 = float((b1 >> 8) + 1) * (1.0 / 16777216.0)
        u2 = float(f32(b2 >> 8) * f32(1.0 / 16777216.0))
        z = math.sqrt(-2.0 * _log(u1)) * _cos2pi(u2)
        t = min(max(float(flat[e]) + z * sd, 0.0), 255.0)
        out[e] = int(t)
    return out.reshape(img.shape)


# ------------------------------------------------------------------------------------------------------------------------------- stages
def deteriorate(img, P, run, i):
    for op in det_ops(run):
        if op == 0:
            img = noise(img, P, i, int(run["noise_var"]))
        elif op == 1:
            img = blur(img, P, int(run["mb_size"]))
        else:
            img = rescale(img, P, int(run["rescale_factor"]))
    return img


def tail_u8(img, P, out_h=32, out_w=128):
    x = img.astype(np.int64)
    if P["jit"]:
        for k in P["jit_order"]:
            if 0 <= k <= 3:
                x = KM.jitter_op(x, int(k), P)
    return IO.resize_bicubic_u8(x.astype(np.uint8), out_h, out_w)


def tail(img, P, out_h=32, out_w=128):
    return IO.to_tensor_normalize(tail_u8(img, P, out_h, out_w))


def augment(img, P, run, i, out_h=32, out_w=128):
    if P["geom"]:
        img = warp(img, P)
    if P["det"]:
        img = deteriorate(img, P, run, i)
    return tail(img, P, out_h, out_w)
