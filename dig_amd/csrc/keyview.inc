// Key-view augmentation of MoCo pre-training (dataset/dataset_image.py:39-50,88-120,145-149 of the reference): the per-image parameter
// sampler and the per-pixel definitions of both stages.  Host-and-device code included by keyview.hip and by the plain-C++ build of the
// same entry points, so both builds run one definition; tests/keyview_model.py restates it in numpy (the spec of the tests).
//
// Sampler (one image; counter-based, so any image / step can be drawn on its own).  Every draw is the first word x of Philox4x32-10 with
// key (seed lo, seed hi) and counter (image, step, draw index, TAG); TAG != 0 keeps the stream apart from the mask generator's (c3 = 0).
//   uniform u = (x >> 8) 2^-24 (float, exact);  U(lo, hi) = lo + (hi - lo) u in float;  an integer below n = (x n) >> 32;
//   normal: Box-Muller on u1 = ((x1 >> 8) + 1) 2^-24, u2 = u(x2): sqrt(-2 ln u1) cos(2 pi u2), evaluated in double (series of basic
//   operations, kv_log / kv_cos2pi, not libm: the two builds draw bit-identical tables), rounded to float;
//   n = 2 + below(4); the op order is the first n entries of a Fisher-Yates shuffle of 0..9; every op's raw parameters are drawn
//   whether the op runs or not (fixed draw indices, KV_D_* below); derived coefficients are computed in double and rounded to float.
//
// Stage A (seqCLR ops at the crop's resolution; uint8 in and out of every op).  Per-pixel work is float32 add / multiply / divide /
// floor with contraction off; "round" is floor(t + 0.5) clipped to [0, 255].  reflect-101 border: ... 2 1 | 0 1 2 ... n-1 | n-2 ...
//   0 LinearContrast  v' = round(127.5 + alpha (v - 127.5))
//   1 GaussianBlur    separable: for each tap row j (in order), h = sum_i t_i v(refl(y + j), refl(x + i)) (in order); acc += t_j h;
//                     one rounding at the end.  Radius ceil(3 sigma), taps exp(-d^2 / (2 sigma^2)) / sum.
//   2 Crop rows       rows [top, top + len) resized back to H with a cubic (a = -0.75, OpenCV's coefficient form), centre-aligned:
//                     s = (y + 0.5) (len / H) - 0.5, taps floor(s) - 1 .. + 2 clamped into the window; top / bottom = round(p H),
//                     at least one row kept.
//   3 Crop columns    the same on columns.
//   4 Sharpen         3 x 3 kernel (1 - alpha) delta + alpha E, E = -1 but 8 + L at the centre, taps row by row, reflect-101.
//   5 Rotate          source = affine(x, y) (about ((W-1)/2, (H-1)/2)); bilinear, 0 outside the image.
//   6 PiecewiseAffine output pixel in cell (ci, ri) of the regular 4 x 4 grid on linspace(0, W-1, 4) x linspace(0, H-1, 4), local
//                     (u, v) in [0, 1]^2, triangle u >= v: d = d00 + u (d01 - d00) + v (d11 - d01), else d = d00 + v (d10 - d00) +
//                     u (d11 - d10) (barycentric on the cell split along its main diagonal); source = (x, y) + d; bilinear, clamped.
//   7 Perspective     one homography from the H x W output onto the quadrilateral of the corners moved inward by |N| W, |N| H
//                     (Heckbert's square-to-quad, scaled); bilinear, 0 outside.  H < 2 or W < 2: identity.
//   8 Solarize        v' = 255 - v where v >= tau (above) or v < tau (below), one choice for all channels.
//   9 Grayscale       g = Pillow's L; v' = round((1 - alpha) v + alpha g).
// Bilinear: x0 = floor(sx), fx = sx - x0, ((v00 (1-fx) + v01 fx) (1-fy) + (v10 (1-fx) + v11 fx) fy), source first clamped to
// [-2, W + 1] x [-2, H + 1] (no change to the result; keeps the integer conversion defined).
//
// Stage B (Pillow as torchvision's PIL path calls it, bit-exact): Resize((32, 128), BICUBIC) (pillow_resize.h), then if `jitter` the four
// ColorJitter ops in `jit_order` -- each Image.blend(d, img, f) = clip(trunc(float(d) + f (img - d))): brightness d = 0, contrast
// d = int(mean(L) + 0.5) over the image, saturation d = L per pixel, hue: Pillow RGB -> HSV, H += hue_shift mod 256, HSV -> RGB -- then if
// `gray` L replicated to three channels, then ToTensor + Normalize.
#pragma once

#include <cmath>
#include <cstddef>

#include "pillow_resize.h"
#include "../../include/dig_aug_types.h"

namespace dig_kv {

constexpr unsigned TAG = 0x4B455956u;                     // c3 of every sampler counter
constexpr int N_LAUNCH = DIG_KV_MAX_OPS;                  // stage A: one launch per op position
enum {
  KV_D_N = 0, KV_D_PERM = 1 /* ..9 */, KV_D_JIT = 10, KV_D_JPERM = 11 /* ..13 */, KV_D_JF = 14 /* ..17 */, KV_D_GRAY = 18,
  KV_D_CONTRAST = 20, KV_D_SIGMA = 21, KV_D_CROP_TB = 22, KV_D_CROP_LR = 24, KV_D_SHARPEN = 26, KV_D_ROT = 28, KV_D_PA_S = 29,
  KV_D_PA_N = 30 /* 32 normals, two draws each: ..93 */, KV_D_PS_S = 94, KV_D_PS_N = 95 /* 8 normals: ..110 */, KV_D_SOLAR = 111,
  KV_D_GRAY_A = 113
};

// sin / cos / log / exp of the sampler from IEEE add, multiply, divide and exact scaling only (contraction off): the two builds' libm
// results may differ in the last bits (and a coefficient derived from a differing sine then differs by far more), these do not
DIG_HD inline void sincos_poly(double x, double* s, double* c) {         // |x| <= pi / 2: Taylor series to x^25 / x^24
#pragma clang fp contract(off)
  const double x2 = x * x;
  double ps = 0.0, pc = 0.0;
  for (int n = 12; n >= 1; --n) {
    ps = 1.0 - ps * x2 / (double)((2 * n) * (2 * n + 1));
    pc = 1.0 - pc * x2 / (double)((2 * n - 1) * (2 * n));
  }
  *s = x * ps;
  *c = pc;
}
DIG_HD inline double kv_cos2pi(double u) {                                 // cos(2 pi u), u in [0, 1)
#pragma clang fp contract(off)
  const double a = 4.0 * u;
  const int q = (int)floor(a);
  double s, c;
  sincos_poly((a - (double)q) * 1.5707963267948966, &s, &c);
  return q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
}
DIG_HD inline double kv_log(double x) {                                    // x > 0
#pragma clang fp contract(off)
  int e;
  const double m = frexp(x, &e);                                           // x = m 2^e, m in [0.5, 1)
  const double z = (m - 1.0) / (m + 1.0), z2 = z * z;
  double p = 0.0;
  for (int k = 30; k >= 0; --k) p = 1.0 / (double)(2 * k + 1) + z2 * p;   // atanh(z) / z
  return (double)e * 0.6931471805599453 + 2.0 * z * p;
}
DIG_HD inline double kv_exp(double x) {                                    // x in [-700, 700]
#pragma clang fp contract(off)
  const double kf = floor(x / 0.6931471805599453 + 0.5);
  const double r = x - kf * 0.6931471805599453;
  double p = 1.0;
  for (int n = 22; n >= 1; --n) p = 1.0 + p * r / (double)n;
  return ldexp(p, (int)kf);
}

struct Rng {
  unsigned img, step, k0, k1;
  DIG_HD unsigned bits(unsigned d) const { return dig_pillow::philox_first(img, step, d, TAG, k0, k1); }
  DIG_HD float u(unsigned d) const { return (float)(bits(d) >> 8) * (1.0f / 16777216.0f); }
  DIG_HD float uniform(unsigned d, float lo, float hi) const {
#pragma clang fp contract(off)
    return lo + (hi - lo) * u(d);
  }
  DIG_HD unsigned below(unsigned d, unsigned n) const { return (unsigned)(((unsigned long long)bits(d) * n) >> 32); }
  DIG_HD float normal(unsigned d) const {
#pragma clang fp contract(off)
    const double u1 = (double)((bits(d) >> 8) + 1u) * (1.0 / 16777216.0);
    const double u2 = (double)u(d + 1);
    return (float)(sqrt(-2.0 * kv_log(u1)) * kv_cos2pi(u2));
  }
};

// Fisher-Yates over the nibbles of a 64-bit word (no runtime-indexed array)
template <class G>
DIG_HD inline unsigned long long shuffle_nibbles(const G& g, unsigned d0, int n, unsigned long long perm) {
  for (int i = n - 1; i >= 1; --i) {
    const int j = (int)g.below(d0 + (unsigned)(n - 1 - i), (unsigned)(i + 1));
    const unsigned long long a = (perm >> (4 * i)) & 15ull, b = (perm >> (4 * j)) & 15ull;
    perm &= ~((15ull << (4 * i)) | (15ull << (4 * j)));
    perm |= (a << (4 * j)) | (b << (4 * i));
  }
  return perm;
}

DIG_HD inline int round_crop(float p, int n) { return (int)floor((double)p * (double)n + 0.5); }

// the table of image `img` (H x W) at (seed, step)
DIG_HD inline void sample_one(dig_kv_params* __restrict__ P, int img, int H, int W, unsigned long long seed, unsigned step) {
#pragma clang fp contract(off)
  const Rng g{(unsigned)img, step, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)};
  P->n_ops = 2 + (int)g.below(KV_D_N, 4);
  const unsigned long long perm = shuffle_nibbles(g, KV_D_PERM, 10, 0x9876543210ull);
  for (int k = 0; k < DIG_KV_MAX_OPS; ++k) P->ops[k] = k < P->n_ops ? (int)((perm >> (4 * k)) & 15ull) : -1;
  // raw draws
  P->contrast_alpha = g.uniform(KV_D_CONTRAST, 0.5f, 1.0f);
  P->blur_sigma = g.uniform(KV_D_SIGMA, 0.5f, 1.5f);
  P->crop_tb[0] = g.uniform(KV_D_CROP_TB, 0.f, 0.3f);
  P->crop_tb[1] = g.uniform(KV_D_CROP_TB + 1, 0.f, 0.3f);
  P->crop_lr[0] = g.uniform(KV_D_CROP_LR, 0.f, 0.1f);
  P->crop_lr[1] = g.uniform(KV_D_CROP_LR + 1, 0.f, 0.1f);
  P->sharpen_alpha = g.uniform(KV_D_SHARPEN, 0.f, 0.5f);
  P->sharpen_lightness = g.uniform(KV_D_SHARPEN + 1, 0.f, 0.5f);
  P->rotate_deg = g.uniform(KV_D_ROT, -10.f, 10.f);
  P->pa_scale = g.uniform(KV_D_PA_S, 0.03f, 0.04f);
  for (int k = 0; k < 16; ++k) {
    P->pa_dy[k] = (float)((double)g.normal(KV_D_PA_N + 2 * k) * (double)P->pa_scale * (double)H);
    P->pa_dx[k] = (float)((double)g.normal(KV_D_PA_N + 32 + 2 * k) * (double)P->pa_scale * (double)W);
  }
  P->persp_sigma = g.uniform(KV_D_PS_S, 0.05f, 0.1f);
  for (int k = 0; k < 8; ++k) P->persp_d[k] = (float)fabs((double)g.normal(KV_D_PS_N + 2 * k) * (double)P->persp_sigma);
  P->solar_tau = g.uniform(KV_D_SOLAR, 32.f, 128.f);
  P->solar_above = g.u(KV_D_SOLAR + 1) < 0.5f ? 1 : 0;
  P->gray_alpha = g.uniform(KV_D_GRAY_A, 0.f, 1.f);
  // derived: Gaussian taps
  const double sg = (double)P->blur_sigma;
  const int r = (int)ceil(3.0 * sg);
  P->blur_radius = r;
  double sum = 0.0;
  for (int d = -r; d <= r; ++d) sum += kv_exp(-(double)(d * d) / (2.0 * sg * sg));
  for (int t = 0; t < DIG_KV_MAX_TAPS; ++t) {
    const int d = t - r;
    P->blur_taps[t] = t <= 2 * r ? (float)(kv_exp(-(double)(d * d) / (2.0 * sg * sg)) / sum) : 0.f;
  }
  // sharpen kernel
  const double sa = (double)P->sharpen_alpha;
  for (int t = 0; t < 9; ++t) P->sharpen_k[t] = (float)(-sa);
  P->sharpen_k[4] = (float)((1.0 - sa) + sa * (8.0 + (double)P->sharpen_lightness));
  // crop windows
  {
    int a = round_crop(P->crop_tb[0], H), b = round_crop(P->crop_tb[1], H);
    if (H - a - b < 1) { b = H - 1 - a; if (b < 0) { a = H - 1; b = 0; } }
    P->crop_y[0] = a; P->crop_y[1] = H - a - b;
    a = round_crop(P->crop_lr[0], W); b = round_crop(P->crop_lr[1], W);
    if (W - a - b < 1) { b = W - 1 - a; if (b < 0) { a = W - 1; b = 0; } }
    P->crop_x[0] = a; P->crop_x[1] = W - a - b;
  }
  // rotation about the centre: source = R(theta) (p - c) + c
  {
    const double th = (double)P->rotate_deg * 3.141592653589793 / 180.0;
    double s, c;
    sincos_poly(th, &s, &c);
    const double cx = 0.5 * (double)(W - 1), cy = 0.5 * (double)(H - 1);
    P->rot[0] = (float)c; P->rot[1] = (float)s; P->rot[2] = (float)(cx - c * cx - s * cy);
    P->rot[3] = (float)(-s); P->rot[4] = (float)c; P->rot[5] = (float)(cy + s * cx - c * cy);
  }
  // homography: Heckbert's unit-square-to-quad, composed with (x, y) -> (x / (W-1), y / (H-1))
  {
    const double w1 = (double)(W - 1), h1 = (double)(H - 1);
    const double x0 = (double)P->persp_d[0] * W, y0 = (double)P->persp_d[1] * H;
    const double x1 = w1 - (double)P->persp_d[2] * W, y1 = (double)P->persp_d[3] * H;
    const double x2 = w1 - (double)P->persp_d[4] * W, y2 = h1 - (double)P->persp_d[5] * H;
    const double x3 = (double)P->persp_d[6] * W, y3 = h1 - (double)P->persp_d[7] * H;
    const double sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
    const double dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
    const double den = dx1 * dy2 - dx2 * dy1;
    if (W < 2 || H < 2 || fabs(den) < 1e-9) {
      for (int t = 0; t < 9; ++t) P->homog[t] = (t % 4 == 0) ? 1.f : 0.f;
    } else {
      const double gg = (sx * dy2 - dx2 * sy) / den, hh = (dx1 * sy - sx * dy1) / den;
      P->homog[0] = (float)((x1 - x0 + gg * x1) / w1); P->homog[1] = (float)((x3 - x0 + hh * x3) / h1); P->homog[2] = (float)x0;
      P->homog[3] = (float)((y1 - y0 + gg * y1) / w1); P->homog[4] = (float)((y3 - y0 + hh * y3) / h1); P->homog[5] = (float)y0;
      P->homog[6] = (float)(gg / w1); P->homog[7] = (float)(hh / h1); P->homog[8] = 1.f;
    }
  }
  // stage B
  P->jitter = g.u(KV_D_JIT) < 0.8f ? 1 : 0;
  const unsigned long long jp = shuffle_nibbles(g, KV_D_JPERM, 4, 0x3210ull);
  for (int k = 0; k < 4; ++k) P->jit_order[k] = (int)((jp >> (4 * k)) & 15ull);
  P->jit_factor[0] = g.uniform(KV_D_JF, 0.6f, 1.4f);
  P->jit_factor[1] = g.uniform(KV_D_JF + 1, 0.6f, 1.4f);
  P->jit_factor[2] = g.uniform(KV_D_JF + 2, 0.8f, 1.2f);
  P->jit_factor[3] = g.uniform(KV_D_JF + 3, -0.1f, 0.1f);
  P->hue_shift = ((int)trunc((double)P->jit_factor[3] * 255.0)) & 255;
  P->gray = g.u(KV_D_GRAY) < 0.2f ? 1 : 0;
  for (int t = 0; t < 17; ++t) P->pad[t] = 0;
}

// ------------------------------------------------------------------------------------------------------------------------ stage A
DIG_HD inline unsigned char round_u8(float t) {
  const float r = floorf(t + 0.5f);
  return r <= 0.f ? (unsigned char)0 : (r >= 255.f ? (unsigned char)255 : (unsigned char)(int)r);
}

DIG_HD inline int refl101(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  i %= period;
  if (i < 0) i += period;
  return i >= n ? period - i : i;
}

DIG_HD inline int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

DIG_HD inline int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// OpenCV's interpolateCubic coefficients (A = -0.75) for fraction x
DIG_HD inline void cubic_coeffs(float x, float w[4]) {
#pragma clang fp contract(off)
  const float A = -0.75f;
  w[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
  w[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  w[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
  w[3] = 1.f - w[0] - w[1] - w[2];
}

// bilinear sample of the three channels at (sx, sy); zero = true: 0 outside the image, else the border is replicated
DIG_HD inline void bilinear(const unsigned char* __restrict__ src, int H, int W, float sx, float sy, bool zero, unsigned char* out) {
#pragma clang fp contract(off)
  sx = fminf(fmaxf(sx, -2.f), (float)W + 1.f);
  sy = fminf(fmaxf(sy, -2.f), (float)H + 1.f);
  const float xf = floorf(sx), yf = floorf(sy);
  const float fx = sx - xf, fy = sy - yf, gx = 1.f - fx, gy = 1.f - fy;
  const int x0 = (int)xf, y0 = (int)yf;
  const bool in_x0 = x0 >= 0 && x0 < W, in_x1 = x0 + 1 >= 0 && x0 + 1 < W, in_y0 = y0 >= 0 && y0 < H, in_y1 = y0 + 1 >= 0 && y0 + 1 < H;
  const int cx0 = clampi(x0, 0, W - 1), cx1 = clampi(x0 + 1, 0, W - 1), cy0 = clampi(y0, 0, H - 1), cy1 = clampi(y0 + 1, 0, H - 1);
  const unsigned char* p00 = src + ((size_t)cy0 * W + cx0) * 3;
  const unsigned char* p01 = src + ((size_t)cy0 * W + cx1) * 3;
  const unsigned char* p10 = src + ((size_t)cy1 * W + cx0) * 3;
  const unsigned char* p11 = src + ((size_t)cy1 * W + cx1) * 3;
  const bool k00 = !zero || (in_y0 && in_x0), k01 = !zero || (in_y0 && in_x1), k10 = !zero || (in_y1 && in_x0), k11 = !zero || (in_y1 && in_x1);
  for (int c = 0; c < 3; ++c) {
    const float v00 = k00 ? (float)p00[c] : 0.f, v01 = k01 ? (float)p01[c] : 0.f;
    const float v10 = k10 ? (float)p10[c] : 0.f, v11 = k11 ? (float)p11[c] : 0.f;
    const float top = v00 * gx + v01 * fx, bot = v10 * gx + v11 * fx;
    out[c] = round_u8(top * gy + bot * fy);
  }
}

// output pixel (y, x) of op `op` on the H x W HWC image at src -> out[3]
DIG_HD inline void op_pixel(int op, const dig_kv_params& P, const unsigned char* __restrict__ src, int H, int W, int y, int x,
                            unsigned char* out) {
#pragma clang fp contract(off)
  const unsigned char* px = src + ((size_t)y * W + x) * 3;
  const float fx = (float)x, fy = (float)y;
  switch (op) {
    case 0: {
      const float a = P.contrast_alpha;
      for (int c = 0; c < 3; ++c) out[c] = round_u8(127.5f + a * ((float)px[c] - 127.5f));
      break;
    }
    case 1: {
      const int r = clampi(P.blur_radius, 0, (DIG_KV_MAX_TAPS - 1) / 2);
      float acc[3] = {0.f, 0.f, 0.f};
      for (int j = -r; j <= r; ++j) {
        const unsigned char* row = src + (size_t)refl101(y + j, H) * W * 3;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
        for (int i = -r; i <= r; ++i) {
          const float t = P.blur_taps[r + i];
          const unsigned char* q = row + (size_t)refl101(x + i, W) * 3;
          h0 = h0 + t * (float)q[0];
          h1 = h1 + t * (float)q[1];
          h2 = h2 + t * (float)q[2];
        }
        const float tj = P.blur_taps[r + j];
        acc[0] = acc[0] + tj * h0;
        acc[1] = acc[1] + tj * h1;
        acc[2] = acc[2] + tj * h2;
      }
      for (int c = 0; c < 3; ++c) out[c] = round_u8(acc[c]);
      break;
    }
    case 2:
    case 3: {
      const bool rows = op == 2;
      const int n = rows ? H : W;
      const int* win = rows ? P.crop_y : P.crop_x;
      const int first = clampi(win[0], 0, n - 1), len = clampi(win[1], 1, n - first);
      const float s = ((rows ? fy : fx) + 0.5f) * ((float)len / (float)n) - 0.5f;
      const float sf = floorf(s);
      float w[4];
      cubic_coeffs(s - sf, w);
      const int i0 = (int)sf - 1;
      float acc[3] = {0.f, 0.f, 0.f};
      for (int k = 0; k < 4; ++k) {
        const int i = first + clampi(i0 + k, 0, len - 1);
        const unsigned char* q = rows ? src + ((size_t)i * W + x) * 3 : src + ((size_t)y * W + i) * 3;
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + w[k] * (float)q[c];
      }
      for (int c = 0; c < 3; ++c) out[c] = round_u8(acc[c]);
      break;
    }
    case 4: {
      float acc[3] = {0.f, 0.f, 0.f};
      for (int dy = -1; dy <= 1; ++dy) {
        const unsigned char* row = src + (size_t)refl101(y + dy, H) * W * 3;
        for (int dx = -1; dx <= 1; ++dx) {
          const float k = P.sharpen_k[(dy + 1) * 3 + dx + 1];
          const unsigned char* q = row + (size_t)refl101(x + dx, W) * 3;
          for (int c = 0; c < 3; ++c) acc[c] = acc[c] + k * (float)q[c];
        }
      }
      for (int c = 0; c < 3; ++c) out[c] = round_u8(acc[c]);
      break;
    }
    case 5: {
      const float sx = (P.rot[0] * fx + P.rot[1] * fy) + P.rot[2], sy = (P.rot[3] * fx + P.rot[4] * fy) + P.rot[5];
      bilinear(src, H, W, sx, sy, true, out);
      break;
    }
    case 6: {
      float u = W > 1 ? (fx * 3.f) / (float)(W - 1) : 0.f, v = H > 1 ? (fy * 3.f) / (float)(H - 1) : 0.f;
      const int ci = u < 2.f ? (int)u : 2, ri = v < 2.f ? (int)v : 2;
      u = u - (float)ci;
      v = v - (float)ri;
      const int k00 = ri * 4 + ci;
      float dx, dy;
      if (u >= v) {
        dx = (P.pa_dx[k00] + u * (P.pa_dx[k00 + 1] - P.pa_dx[k00])) + v * (P.pa_dx[k00 + 5] - P.pa_dx[k00 + 1]);
        dy = (P.pa_dy[k00] + u * (P.pa_dy[k00 + 1] - P.pa_dy[k00])) + v * (P.pa_dy[k00 + 5] - P.pa_dy[k00 + 1]);
      } else {
        dx = (P.pa_dx[k00] + v * (P.pa_dx[k00 + 4] - P.pa_dx[k00])) + u * (P.pa_dx[k00 + 5] - P.pa_dx[k00 + 4]);
        dy = (P.pa_dy[k00] + v * (P.pa_dy[k00 + 4] - P.pa_dy[k00])) + u * (P.pa_dy[k00 + 5] - P.pa_dy[k00 + 4]);
      }
      bilinear(src, H, W, fx + dx, fy + dy, false, out);
      break;
    }
    case 7: {
      const float* h = P.homog;
      const float den = (h[6] * fx + h[7] * fy) + h[8];
      const float sx = ((h[0] * fx + h[1] * fy) + h[2]) / den, sy = ((h[3] * fx + h[4] * fy) + h[5]) / den;
      bilinear(src, H, W, sx, sy, true, out);
      break;
    }
    case 8: {
      const float tau = P.solar_tau;
      for (int c = 0; c < 3; ++c) {
        const int v = px[c];
        const bool inv = P.solar_above ? ((float)v >= tau) : ((float)v < tau);
        out[c] = (unsigned char)(inv ? 255 - v : v);
      }
      break;
    }
    case 9: {
      const float a = P.gray_alpha, b = 1.f - a;
      const float g = (float)luma(px[0], px[1], px[2]);
      for (int c = 0; c < 3; ++c) out[c] = round_u8(b * (float)px[c] + a * g);
      break;
    }
    default:                                            // (not an op id: the image passes through)
      for (int c = 0; c < 3; ++c) out[c] = px[c];
  }
}

// the op image `P` runs at stage-A launch L (0..N_LAUNCH-1).  Its ops are right-aligned: op j runs at launch N_LAUNCH - n + j, reading
// the crop (j = 0) or the half the previous launch wrote, and writing the first half of the workspace at even L, the second at odd L --
// so the last op of every image lands in the first half (N_LAUNCH - 1 is even), where stage B reads.  -1: nothing at this launch;
// -2: copy the crop through (an image without ops, at the last launch).
DIG_HD inline int op_at_launch(const dig_kv_params& P, int L, int* j_out) {
  const int n = clampi(P.n_ops, 0, DIG_KV_MAX_OPS);
  const int j = L - (N_LAUNCH - n);
  *j_out = j;
  if (j < 0) return (n == 0 && L == N_LAUNCH - 1) ? -2 : -1;
  return P.ops[j];
}

// ------------------------------------------------------------------------------------------------------------------------ stage B
DIG_HD inline int blend(int d, int v, float f) {
#pragma clang fp contract(off)
  const float t = (float)d + f * (float)(v - d);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

DIG_HD inline int clip8i(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's rgb2hsv_row (Convert.c): float / double mix as the C source has it
DIG_HD inline void rgb2hsv(int r, int g, int b, int* uh, int* us, int* uv) {
#pragma clang fp contract(off)
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  *uv = maxc;
  if (minc == maxc) { *uh = 0; *us = 0; return; }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
  else h = (float)((4.0 + (double)gc) - (double)rc);
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  *uh = clip8i((int)((double)h * 255.0));
  *us = clip8i((int)((double)s * 255.0));
}

// Pillow's hsv2rgb (Convert.c)
DIG_HD inline void hsv2rgb(int h, int s, int v, int* r, int* g, int* b) {
#pragma clang fp contract(off)
  if (s == 0) { *r = v; *g = v; *b = v; return; }
  const int i = (int)floor((double)(float)h * 6.0 / 255.0);
  const float f = (float)((double)(float)h * 6.0 / 255.0 - (double)(float)i);
  const float fs = (float)((double)(float)s / 255.0);
  const int p = clip8i((int)round((double)(float)v * (1.0 - (double)fs)));
  const int q = clip8i((int)round((double)(float)v * (1.0 - (double)(fs * f))));
  const int t = clip8i((int)round((double)(float)v * (1.0 - (double)fs * (1.0 - (double)f))));
  switch (i % 6) {
    case 0: *r = v; *g = t; *b = p; break;
    case 1: *r = q; *g = v; *b = p; break;
    case 2: *r = p; *g = v; *b = t; break;
    case 3: *r = p; *g = q; *b = v; break;
    case 4: *r = t; *g = p; *b = v; break;
    default: *r = v; *g = p; *b = q; break;
  }
}

// one jitter op on one pixel (contrast: d = the image's mean L, computed by the caller); factors / hue_shift as in dig_kv_params
DIG_HD inline void jitter_apply(int op, const float* jit_factor, int hue_shift, int contrast_mean, int* c) {
  const float f = jit_factor[op & 3];
  switch (op & 3) {
    case 0: for (int k = 0; k < 3; ++k) c[k] = blend(0, c[k], f); break;
    case 1: for (int k = 0; k < 3; ++k) c[k] = blend(contrast_mean, c[k], f); break;
    case 2: {
      const int l = luma(c[0], c[1], c[2]);
      for (int k = 0; k < 3; ++k) c[k] = blend(l, c[k], f);
      break;
    }
    default: {
      int h, s, v;
      rgb2hsv(c[0], c[1], c[2], &h, &s, &v);
      hsv2rgb((h + hue_shift) & 255, s, v, &c[0], &c[1], &c[2]);
    }
  }
}
DIG_HD inline void jitter_pixel(int op, const dig_kv_params& P, int contrast_mean, int* c) {
  jitter_apply(op, P.jit_factor, P.hue_shift, contrast_mean, c);
}

using dig_rules::stage_b_lds_bytes;   // dynamic LDS bytes of stage B (abi_rules.h: the rule and the launcher share it)

// Pillow's ImageStat mean of L over n pixels (sum in a double), + 0.5, truncated
DIG_HD inline int contrast_mean(long long sum_l, int n) { return (int)((double)sum_l / (double)n + 0.5); }

}  // namespace dig_kv
