// ABINet augmentation of fine-tuning (--num_view 2 --use_abi_aug; transforms.py:188-504, dataset/dataset_lmdb.py:36-47 of the reference):
// the per-image sampler, the warp, the three deterioration ops and the tail (ColorJitter at the warped resolution, Pillow's bicubic
// resize, Normalize).  Host-and-device code included by abiaug.hip and by the plain-C++ build, so both builds run one definition;
// tests/abiaug_model.py restates it in numpy.  Table layout: include/dig_aug_types.h (dig_abi_run, dig_abi_params).
//
// Run parameters (dig_abi_run): drawn once per run by the caller (dig_amd/augment.py), as the reference's constructors draw them.
//
// Sampler (one image; counter-based).  Draws are the first word of Philox4x32-10 under key (seed lo, seed hi), counter (image, step,
// draw index, TAG); uniforms / below(n) as keyview.inc.  Beta(4, 4) is the 4th smallest of 7 uniforms, Beta(1, 4) the smallest of 4
// (order statistics: the same law, no libm).  sym(m) = (Beta(4,4) - 0.5) 2 m.  Gates u < 0.5, 0.25, 0.25.  Every raw parameter is drawn
// whatever the gates and the run's geometry (fixed draw indices, AB_D_* below).  The derived geometry is computed in double from
// sincos_poly (keyview.inc), not libm:
//   rotation    cv2.getRotationMatrix2D((W/2, H/2), angle, 1); canvas int(H|sin| + W|cos|) x int(H|cos| + W|sin|), centred.
//   affine      torchvision 0.4's _get_inverse_affine_matrix((W/2, H/2), angle, (0, 0), scale, shear) used as the FORWARD matrix; the
//               corners (0,0) (W-1,0) (W-1,H-1) (0,H-1) projected and truncated with int(); their minimum-area rectangle (rotating
//               calipers over the four edges in order, double, the first minimal edge wins), its corners truncated; canvas (max - min)
//               per axis, centred as the reference shifts M.
//   perspective corners moved inward by the offsets; the homography of the four point pairs (Heckbert's square-to-quad, scaled);
//               canvas (max_x, max_y) of the corners' minimum-area rectangle, cropped at [max(min_y, 0):, max(min_x, 0):].
//   A canvas side of 0 (crops of one or two pixels) becomes 1.  minv = the inverse map (cv2's invertAffineTransform / the adjugate),
//   with the perspective crop folded in, rounded to float.
//   Motion blur: kernel of the run's size d = the d x d image with row d/2 set to 1, warped by getRotationMatrix2D((d/2, d/2), angle, 1)
//   (linear, 0 outside, the 1/32 grid below, in double), divided by d, rounded to float.
//
// Resamplers (the project's definitions; cv2's geometry and borders, integer arithmetic):
//   warp       output (x, y) -> source (sx, sy) by minv in float32; q = floor(s 32 + 0.5) per axis (s first clamped to [-4, n + 3]);
//              nearest: index (q + 16) >> 5; linear: index q >> 5, weights (32 - f) 64, f 64 (f = q & 31); cubic: indices q >> 5 - 1 .. + 2,
//              weights round(2048 cubic(f / 32)) (OpenCV's A = -0.75 form); BORDER_REPLICATE (indices clamped).
//   resize     cv2.resize's source positions: nearest floor(x src / dst); linear / cubic s = (x + 0.5) src / dst - 0.5 (linear: s < 0 -> 0,
//              s >= n - 1 -> n - 1, fraction 0); area with both axes shrinking: cv2's box cells (cell = min(scale, n - x scale), partial
//              cells above 1e-3); area otherwise: linear taps at floor(x scale), fraction (x + 1) - (floor(x scale) + 1) / scale (<= 0 -> 0,
//              else its fractional part).  Weights round(2048 w) (floor(t + 0.5) in float).
//   Both: value = clamp((sum_y wy sum_x wx v + 2^21) >> 22, 0, 255), 64-bit sum, separable weights, indices clamped into the image.
//   pyrDown    5 x 5 [1 4 6 4 1]^2, reflect-101, output ((n + 1) / 2), (sum + 128) >> 8.
//   noise      element e = 3 p + c: Box-Muller (keyview.inc) on the draws 2e, 2e + 1 of counter (image, noise_step, ., TAG_NOISE) under
//              noise_key, times sqrt(var), in double; v + n clipped to [0, 255] and truncated (astype(uint8)).
//   blur       filter2D: correlation with anchor (d/2, d/2), reflect-101, float32 sum row-major, floor(t + 0.5) clipped.
//   rescale    resize to 128 x 512 (rs_interp[0]), pyrDown factor times, resize back (rs_interp[1]); factor 0: the op is skipped.
//
// Workspace of one image (dig_abiaug_workspace_bytes): nothing when no gate of geometry / deterioration fired; else region A (the warp's
// output), and with deterioration region B and, for a rescale factor > 0, region R (128 x 512 x 3 + 64 x 256 x 3: the pyramid ping-pong).
// A and B are round256(wh ww 3) bytes.  Deterioration op j of the run (noise / blur / rescale, the rescale left out at factor 0) reads
// (j = 0: A if the geometry fired, else the crop; else the previous op's output) and writes B at even j, A at odd j.
//
// Tail (bit-exact with Pillow + torchvision): if `jit`, the four ColorJitter ops in jit_order on every pixel of the image the tail reads
// (contrast: the mean L of the whole image after the ops before it, keyview.inc contrast_mean), Pillow's bicubic resize, ToTensor,
// Normalize.  The jitter is applied to each source pixel as the resize reads it (pillow_resize.h resize_pixel_f).
#pragma once

#include "keyview.inc"

namespace dig_abi {

constexpr unsigned TAG = 0x41424941u;        // c3 of the sampler counters
constexpr unsigned TAG_NOISE = 0x41424E5Au;  // c3 of the noise counters
constexpr int RS_H = 128, RS_W = 512;        // CVRescale's base size
constexpr long long RS_BYTES = 3LL * RS_H * RS_W + 3LL * (RS_H / 2) * (RS_W / 2);
enum {
  AB_D_GEOM = 0, AB_D_DET = 1, AB_D_JIT = 2, AB_D_ANGLE = 3 /* 7 draws: ..9 */, AB_D_SCALE = 10, AB_D_SHX = 11 /* ..17 */,
  AB_D_SHY = 18 /* ..24 */, AB_D_OW = 25 /* 4 x 4 draws: ..40 */, AB_D_OH = 41 /* ..56 */, AB_D_INTERP = 57, AB_D_RS = 58 /* ..59 */,
  AB_D_JPERM = 60 /* ..62 */, AB_D_JF = 63 /* ..66 */
};

struct Rng {
  unsigned img, step, k0, k1;
  DIG_HD unsigned bits(unsigned d) const { return dig_pillow::philox_first(img, step, d, TAG, k0, k1); }
  DIG_HD float u(unsigned d) const { return (float)(bits(d) >> 8) * (1.0f / 16777216.0f); }
  DIG_HD float uniform(unsigned d, float lo, float hi) const {
#pragma clang fp contract(off)
    return lo + (hi - lo) * u(d);
  }
  DIG_HD unsigned below(unsigned d, unsigned n) const { return (unsigned)(((unsigned long long)bits(d) * n) >> 32); }
  // k-th smallest (1-based) of n uniforms at draws d .. d + n - 1: Beta(k, n + 1 - k)
  DIG_HD float order_stat(unsigned d, int n, int k) const {
    float v[7];
    for (int i = 0; i < 7; ++i) v[i] = i < n ? u(d + (unsigned)i) : 2.f;
    for (int i = 1; i < 7; ++i)                                             // insertion sort of 7 values
      for (int j = i; j > 0 && v[j - 1] > v[j]; --j) { const float t = v[j]; v[j] = v[j - 1]; v[j - 1] = t; }
    float r = v[0];
    for (int i = 1; i < 7; ++i) r = (i == k - 1) ? v[i] : r;
    return r;
  }
  DIG_HD float sym(unsigned d, float m) const {
#pragma clang fp contract(off)
    return (float)(((double)order_stat(d, 7, 4) - 0.5) * 2.0 * (double)m);
  }
};

DIG_HD inline long long round256(long long b) { return (b + 255) / 256 * 256; }

DIG_HD inline long long image_bytes(int geom, int det, int wh, int ww, int rescale_factor) {
  if (!geom && !det) return 0;
  const long long rb = round256(3LL * wh * ww);
  return det ? 2 * rb + (rescale_factor > 0 ? RS_BYTES : 0) : rb;
}

DIG_HD inline int n_det_ops(const dig_abi_run& R) { return R.rescale_factor > 0 ? 3 : 2; }
// the run's k-th deterioration op (the rescale left out at factor 0)
DIG_HD inline int det_op(const dig_abi_run& R, int k) {
  int j = 0;
  for (int i = 0; i < 3; ++i) {
    const int op = R.det_order[i];
    if (op == 2 && R.rescale_factor <= 0) continue;
    if (j == k) return op;
    ++j;
  }
  return -1;
}

DIG_HD inline double deg2rad(double a) { return a * 3.141592653589793 / 180.0; }
DIG_HD inline void sincos_deg(double a, double* s, double* c) { dig_kv::sincos_poly(deg2rad(a), s, c); }

// cv2.invertAffineTransform of the 2 x 3 matrix m -> out (2 x 3)
DIG_HD inline void invert_affine(const double* m, double* out) {
#pragma clang fp contract(off)
  double D = m[0] * m[4] - m[1] * m[3];
  D = D != 0.0 ? 1.0 / D : 0.0;
  const double a11 = m[4] * D, a22 = m[0] * D, a12 = -m[1] * D, a21 = -m[3] * D;
  out[0] = a11; out[1] = a12; out[2] = -a11 * m[2] - a12 * m[5];
  out[3] = a21; out[4] = a22; out[5] = -a21 * m[2] - a22 * m[5];
}

// the minimum-area rectangle of four points in order (px, py) -> the truncated bounds of its corners
DIG_HD inline void min_area_box(const double* px, const double* py, int* min_x, int* min_y, int* max_x, int* max_y) {
#pragma clang fp contract(off)
  double best = -1.0;
  double bx[4] = {px[0], px[0], px[0], px[0]}, by[4] = {py[0], py[0], py[0], py[0]};
  for (int e = 0; e < 4; ++e) {
    const double ex = px[(e + 1) & 3] - px[e], ey = py[(e + 1) & 3] - py[e];
    const double len = sqrt(ex * ex + ey * ey);
    if (len == 0.0) continue;
    const double ux = ex / len, uy = ey / len, vx = -uy, vy = ux;
    double u0 = 0.0, u1 = 0.0, v0 = 0.0, v1 = 0.0;
    for (int k = 0; k < 4; ++k) {
      const double dx = px[k] - px[e], dy = py[k] - py[e];
      const double su = dx * ux + dy * uy, sv = dx * vx + dy * vy;
      u0 = su < u0 ? su : u0; u1 = su > u1 ? su : u1;
      v0 = sv < v0 ? sv : v0; v1 = sv > v1 ? sv : v1;
    }
    const double area = (u1 - u0) * (v1 - v0);
    if (best < 0.0 || area < best) {
      best = area;
      const double cu[4] = {u0, u1, u1, u0}, cv[4] = {v0, v0, v1, v1};
      for (int k = 0; k < 4; ++k) {
        bx[k] = (px[e] + cu[k] * ux) + cv[k] * vx;
        by[k] = (py[e] + cu[k] * uy) + cv[k] * vy;
      }
    }
  }
  int x0 = (int)bx[0], x1 = x0, y0 = (int)by[0], y1 = y0;
  for (int k = 1; k < 4; ++k) {
    const int xi = (int)bx[k], yi = (int)by[k];
    x0 = xi < x0 ? xi : x0; x1 = xi > x1 ? xi : x1;
    y0 = yi < y0 ? yi : y0; y1 = yi > y1 ? yi : y1;
  }
  *min_x = x0; *min_y = y0; *max_x = x1; *max_y = y1;
}

// OpenCV's cubic (A = -0.75) at fraction f / 32, as 11-bit integer weights
DIG_HD inline void cubic_w(int f, int w[4]) {
#pragma clang fp contract(off)
  float c[4];
  dig_kv::cubic_coeffs((float)f * (1.0f / 32.0f), c);
  for (int k = 0; k < 4; ++k) w[k] = (int)floorf(c[k] * 2048.f + 0.5f);
}

// the geometry of table P for run geometry type `type` (raw draws already in P): wh / ww / minv
DIG_HD inline void derive_geometry(dig_abi_params* __restrict__ P, int type) {
#pragma clang fp contract(off)
  const int H = P->h, W = P->w;
  double m[6], inv[6];
  int wh = H, ww = W;
  double hm[9];
  bool persp = false;
  if (type == 0) {
    double s, c;
    sincos_deg((double)P->angle, &s, &c);
    const double cx = (double)W / 2.0, cy = (double)H / 2.0;
    m[0] = c; m[1] = s; m[2] = (1.0 - c) * cx - s * cy;
    m[3] = -s; m[4] = c; m[5] = s * cx + (1.0 - c) * cy;
    const double as = fabs(m[1]), ac = fabs(m[0]);
    ww = (int)((double)H * as + (double)W * ac);
    wh = (int)((double)H * ac + (double)W * as);
    m[2] += (double)(ww - W) / 2.0;
    m[5] += (double)(wh - H) / 2.0;
  } else if (type == 1) {
    double sr, cr, sxs, sxc, sys, syc, rss, rsc;
    sincos_deg((double)P->angle, &sr, &cr);
    sincos_deg((double)P->shear[0], &sxs, &sxc);
    sincos_deg((double)P->shear[1], &sys, &syc);
    dig_kv::sincos_poly(deg2rad((double)P->angle) - deg2rad((double)P->shear[1]), &rss, &rsc);
    const double tsx = sxs / sxc;
    const double a = rsc / syc, b = -rsc * tsx / syc - sr, c = rss / syc, d = -rss * tsx / syc + cr;
    const double sc = (double)P->scale;
    m[0] = d / sc; m[1] = -b / sc; m[2] = 0.0 / sc; m[3] = -c / sc; m[4] = a / sc; m[5] = 0.0 / sc;
    const double cx = (double)W / 2.0, cy = (double)H / 2.0;
    m[2] += m[0] * -cx + m[1] * -cy;
    m[5] += m[3] * -cx + m[4] * -cy;
    m[2] += cx;
    m[5] += cy;
    const double sx[4] = {0.0, (double)(W - 1), (double)(W - 1), 0.0}, sy[4] = {0.0, 0.0, (double)(H - 1), (double)(H - 1)};
    double px[4], py[4];
    for (int k = 0; k < 4; ++k) {
      px[k] = (double)(int)((m[0] * sx[k] + m[1] * sy[k]) + m[2]);
      py[k] = (double)(int)((m[3] * sx[k] + m[4] * sy[k]) + m[5]);
    }
    int x0, y0, x1, y1;
    min_area_box(px, py, &x0, &y0, &x1, &y1);
    ww = x1 - x0;
    wh = y1 - y0;
    m[2] += (double)(ww - W) / 2.0;
    m[5] += (double)(wh - H) / 2.0;
  } else {
    persp = true;
    const double w1 = (double)(W - 1), h1 = (double)(H - 1);
    const double qx[4] = {(double)P->persp_ow[0], w1 - (double)P->persp_ow[1], w1 - (double)P->persp_ow[2], (double)P->persp_ow[3]};
    const double qy[4] = {(double)P->persp_oh[0], (double)P->persp_oh[1], h1 - (double)P->persp_oh[2], h1 - (double)P->persp_oh[3]};
    int x0, y0, x1, y1;
    min_area_box(qx, qy, &x0, &y0, &x1, &y1);
    x0 = x0 > 0 ? x0 : 0;
    y0 = y0 > 0 ? y0 : 0;
    ww = x1 - x0;
    wh = y1 - y0;
    // forward homography: unit square -> quad (Heckbert), composed with (x, y) -> (x / (W-1), y / (H-1))
    double f[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double sxq = qx[0] - qx[1] + qx[2] - qx[3], syq = qy[0] - qy[1] + qy[2] - qy[3];
    const double dx1 = qx[1] - qx[2], dx2 = qx[3] - qx[2], dy1 = qy[1] - qy[2], dy2 = qy[3] - qy[2];
    const double den = dx1 * dy2 - dx2 * dy1;
    if (W >= 2 && H >= 2 && den != 0.0) {
      const double g = (sxq * dy2 - dx2 * syq) / den, hh = (dx1 * syq - sxq * dy1) / den;
      f[0] = (qx[1] - qx[0] + g * qx[1]) / w1; f[1] = (qx[3] - qx[0] + hh * qx[3]) / h1; f[2] = qx[0];
      f[3] = (qy[1] - qy[0] + g * qy[1]) / w1; f[4] = (qy[3] - qy[0] + hh * qy[3]) / h1; f[5] = qy[0];
      f[6] = g / w1; f[7] = hh / h1; f[8] = 1.0;
    }
    // inverse = adjugate (the scale of a homography is free), then the crop offset folded in
    double a[9];
    a[0] = f[4] * f[8] - f[5] * f[7]; a[1] = f[2] * f[7] - f[1] * f[8]; a[2] = f[1] * f[5] - f[2] * f[4];
    a[3] = f[5] * f[6] - f[3] * f[8]; a[4] = f[0] * f[8] - f[2] * f[6]; a[5] = f[2] * f[3] - f[0] * f[5];
    a[6] = f[3] * f[7] - f[4] * f[6]; a[7] = f[1] * f[6] - f[0] * f[7]; a[8] = f[0] * f[4] - f[1] * f[3];
    const double ox = (double)x0, oy = (double)y0;
    for (int r = 0; r < 3; ++r) {
      hm[3 * r] = a[3 * r];
      hm[3 * r + 1] = a[3 * r + 1];
      hm[3 * r + 2] = (a[3 * r] * ox + a[3 * r + 1] * oy) + a[3 * r + 2];
    }
  }
  if (!persp) {
    invert_affine(m, inv);
    for (int k = 0; k < 6; ++k) hm[k] = inv[k];
    hm[6] = 0.0; hm[7] = 0.0; hm[8] = 1.0;
  }
  for (int k = 0; k < 9; ++k) P->minv[k] = (float)hm[k];
  P->wh = wh > 0 ? wh : 1;
  P->ww = ww > 0 ? ww : 1;
}

// the run's motion-blur kernel (d x d, row-major) into k[25]
DIG_HD inline void motion_kernel(const dig_abi_run& R, float* k) {
#pragma clang fp contract(off)
  const int d = R.mb_size < 1 ? 1 : (R.mb_size > DIG_ABI_MB_MAX ? DIG_ABI_MB_MAX : R.mb_size);
  const double c0 = (double)(d / 2);
  double s, c;
  sincos_deg((double)R.mb_angle, &s, &c);
  const double m[6] = {c, s, (1.0 - c) * c0 - s * c0, -s, c, s * c0 + (1.0 - c) * c0};
  double inv[6];
  invert_affine(m, inv);
  for (int t = 0; t < DIG_ABI_MB_MAX * DIG_ABI_MB_MAX; ++t) k[t] = 0.f;
  for (int y = 0; y < d; ++y)
    for (int x = 0; x < d; ++x) {
      const double sx = (inv[0] * (double)x + inv[1] * (double)y) + inv[2], sy = (inv[3] * (double)x + inv[4] * (double)y) + inv[5];
      const int qx = (int)floor(sx * 32.0 + 0.5), qy = (int)floor(sy * 32.0 + 0.5);
      const int ix = qx >> 5, iy = qy >> 5;
      const double fx = (double)(qx & 31) / 32.0, fy = (double)(qy & 31) / 32.0;
      double v = 0.0;
      for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) {
          const int xx = ix + i, yy = iy + j;
          const double src = (yy == d / 2 && xx >= 0 && xx < d) ? 1.0 : 0.0;
          v += (i ? fx : 1.0 - fx) * (j ? fy : 1.0 - fy) * src;
        }
      k[y * d + x] = (float)(v / (double)d);
    }
}

// the table of image `img` (H x W) at (seed, step) under run R; ws_off is left to the caller (a prefix sum over the images)
DIG_HD inline void sample_one(dig_abi_params* __restrict__ P, int img, int H, int W, const dig_abi_run& R, unsigned long long seed,
                              unsigned step) {
#pragma clang fp contract(off)
  const Rng g{(unsigned)img, step, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)};
  P->geom = g.u(AB_D_GEOM) < 0.5f ? 1 : 0;
  P->det = g.u(AB_D_DET) < 0.25f ? 1 : 0;
  P->jit = g.u(AB_D_JIT) < 0.25f ? 1 : 0;
  P->geom_interp = (int)g.below(AB_D_INTERP, 4);
  P->angle = g.sym(AB_D_ANGLE, 45.f);
  P->scale = g.uniform(AB_D_SCALE, 0.5f, 2.0f);
  P->shear[0] = g.sym(AB_D_SHX, 45.f);
  P->shear[1] = g.sym(AB_D_SHY, 15.f);
  for (int k = 0; k < 4; ++k) {
    P->persp_ow[k] = (int)((double)g.order_stat(AB_D_OW + 4 * k, 4, 1) * (0.5 * (double)W / 2.0));
    P->persp_oh[k] = (int)((double)g.order_stat(AB_D_OH + 4 * k, 4, 1) * (0.5 * (double)H / 2.0));
  }
  P->h = H;
  P->w = W;
  derive_geometry(P, R.geom_type);
  if (!P->geom) { P->wh = H; P->ww = W; }
  P->rs_interp[0] = (int)g.below(AB_D_RS, 4);
  P->rs_interp[1] = (int)g.below(AB_D_RS + 1, 4);
  motion_kernel(R, P->mb_k);
  const unsigned long long jp = dig_kv::shuffle_nibbles(g, AB_D_JPERM, 4, 0x3210ull);
  for (int k = 0; k < 4; ++k) P->jit_order[k] = (int)((jp >> (4 * k)) & 15ull);
  P->jit_factor[0] = g.uniform(AB_D_JF, 0.5f, 1.5f);
  P->jit_factor[1] = g.uniform(AB_D_JF + 1, 0.5f, 1.5f);
  P->jit_factor[2] = g.uniform(AB_D_JF + 2, 0.5f, 1.5f);
  P->jit_factor[3] = g.uniform(AB_D_JF + 3, -0.1f, 0.1f);
  P->hue_shift = ((int)trunc((double)P->jit_factor[3] * 255.0)) & 255;
  P->noise_key[0] = (unsigned)(seed & 0xffffffffull);
  P->noise_key[1] = (unsigned)(seed >> 32);
  P->noise_step = step;
  P->final_buf = P->det ? ((n_det_ops(R) & 1) ? 2 : 1) : (P->geom ? 1 : 0);
  P->pad0 = 0;
  P->ws_off = 0;
  for (int t = 0; t < 24; ++t) P->pad[t] = 0;
}

// ------------------------------------------------------------------------------------------------------------------------ pixels
DIG_HD inline int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }
DIG_HD inline unsigned char sat_shift22(long long acc) {
  const long long v = (acc + (1LL << 21)) >> 22;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one axis of a warp: source coordinate s on an axis of n pixels -> first index, tap count, 11-bit weights
DIG_HD inline int warp_taps(float s, int n, int interp, int* w) {
#pragma clang fp contract(off)
  s = fminf(fmaxf(s, -4.f), (float)n + 3.f);
  const int q = (int)floorf(s * 32.f + 0.5f);
  if (interp == 0) { w[0] = 2048; return (q + 16) >> 5; }
  const int f = q & 31;
  if (interp == 2) { cubic_w(f, w); return (q >> 5) - 1; }
  w[0] = (32 - f) * 64; w[1] = f * 64;
  return q >> 5;
}
DIG_HD inline int warp_ntaps(int interp) { return interp == 0 ? 1 : (interp == 2 ? 4 : 2); }

// output pixel (y, x) of the warp of the H x W crop at src by table P -> out[3]
DIG_HD inline void warp_pixel(const dig_abi_params& P, const unsigned char* __restrict__ src, int H, int W, int y, int x, unsigned char* out) {
#pragma clang fp contract(off)
  const float fx = (float)x, fy = (float)y;
  const float* m = P.minv;
  const float den = (m[6] * fx + m[7] * fy) + m[8];
  const float sx = ((m[0] * fx + m[1] * fy) + m[2]) / den, sy = ((m[3] * fx + m[4] * fy) + m[5]) / den;
  const int interp = P.geom_interp == 3 ? 1 : clampi(P.geom_interp, 0, 2);
  int wx[4], wy[4];
  const int x0 = warp_taps(sx, W, interp, wx), y0 = warp_taps(sy, H, interp, wy), nt = warp_ntaps(interp);
  long long a0 = 0, a1 = 0, a2 = 0;
  for (int j = 0; j < nt; ++j) {
    const unsigned char* row = src + (size_t)clampi(y0 + j, 0, H - 1) * W * 3;
    long long h0 = 0, h1 = 0, h2 = 0;
    for (int i = 0; i < nt; ++i) {
      const unsigned char* q = row + (size_t)clampi(x0 + i, 0, W - 1) * 3;
      h0 += (long long)wx[i] * q[0]; h1 += (long long)wx[i] * q[1]; h2 += (long long)wx[i] * q[2];
    }
    a0 += wy[j] * h0; a1 += wy[j] * h1; a2 += wy[j] * h2;
  }
  out[0] = sat_shift22(a0); out[1] = sat_shift22(a1); out[2] = sat_shift22(a2);
}

// one axis of cv2.resize from n to m pixels, output index x: calls tap(index, 11-bit weight) for each tap.  area_box: the image-level
// choice of cv2's box cells (interp 3 and both axes shrinking).
template <class F>
DIG_HD inline void resize_taps(int interp, bool area_box, int x, int n, int m, const F& tap) {
#pragma clang fp contract(off)
  const double scale = (double)n / (double)m;
  if (interp == 0) {
    tap(clampi((int)floor((double)x * scale), 0, n - 1), 2048);
    return;
  }
  if (interp == 3 && area_box) {
    const double fsx1 = (double)x * scale, fsx2 = fsx1 + scale;
    const double cell = scale < (double)n - fsx1 ? scale : (double)n - fsx1;
    const int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
    if ((double)sx1 - fsx1 > 1e-3) tap(clampi(sx1 - 1, 0, n - 1), (int)floorf((float)(((double)sx1 - fsx1) / cell) * 2048.f + 0.5f));
    for (int s = sx1; s < sx2 && s < n; ++s) tap(s, (int)floorf((float)(1.0 / cell) * 2048.f + 0.5f));
    if (fsx2 - (double)sx2 > 1e-3 && sx2 < n) {
      double part = fsx2 - (double)sx2;
      part = part < 1.0 ? part : 1.0;
      part = part < cell ? part : cell;
      tap(sx2, (int)floorf((float)(part / cell) * 2048.f + 0.5f));
    }
    return;
  }
  int sx;
  float f;
  if (interp == 3) {
    sx = (int)floor((double)x * scale);
    f = (float)((double)(x + 1) - (double)(sx + 1) / scale);
    f = f <= 0.f ? 0.f : f - floorf(f);
  } else {
    const float s = (float)(((double)x + 0.5) * scale - 0.5);
    sx = (int)floorf(s);
    f = s - (float)sx;
  }
  if (interp == 2) {
    float c[4];
    dig_kv::cubic_coeffs(f, c);
    for (int k = 0; k < 4; ++k) tap(clampi(sx - 1 + k, 0, n - 1), (int)floorf(c[k] * 2048.f + 0.5f));
    return;
  }
  if (sx < 0) { f = 0.f; sx = 0; }
  if (sx >= n - 1) { f = 0.f; sx = n - 1; }
  tap(sx, (int)floorf((1.f - f) * 2048.f + 0.5f));
  tap(clampi(sx + 1, 0, n - 1), (int)floorf(f * 2048.f + 0.5f));
}

// output pixel (y, x) of cv2.resize(src (sh x sw) -> dh x dw, interp) -> out[3]
DIG_HD inline void resize_cv_pixel(const unsigned char* __restrict__ src, int sh, int sw, int dh, int dw, int interp, int y, int x,
                                   unsigned char* out) {
  interp = clampi(interp, 0, 3);
  const bool box = interp == 3 && sh >= dh && sw >= dw;
  long long a0 = 0, a1 = 0, a2 = 0;
  resize_taps(interp, box, y, sh, dh, [&](int iy, int wy) {
    const unsigned char* row = src + (size_t)iy * sw * 3;
    long long h0 = 0, h1 = 0, h2 = 0;
    resize_taps(interp, box, x, sw, dw, [&](int ix, int wx) {
      const unsigned char* q = row + (size_t)ix * 3;
      h0 += (long long)wx * q[0]; h1 += (long long)wx * q[1]; h2 += (long long)wx * q[2];
    });
    a0 += wy * h0; a1 += wy * h1; a2 += wy * h2;
  });
  out[0] = sat_shift22(a0); out[1] = sat_shift22(a1); out[2] = sat_shift22(a2);
}

// output pixel (y, x) of cv2.pyrDown of src (sh x sw) -> out[3]
DIG_HD inline void pyrdown_pixel(const unsigned char* __restrict__ src, int sh, int sw, int y, int x, unsigned char* out) {
  const int k[5] = {1, 4, 6, 4, 1};
  int a0 = 0, a1 = 0, a2 = 0;
  for (int j = 0; j < 5; ++j) {
    const unsigned char* row = src + (size_t)dig_kv::refl101(2 * y + j - 2, sh) * sw * 3;
    int h0 = 0, h1 = 0, h2 = 0;
    for (int i = 0; i < 5; ++i) {
      const unsigned char* q = row + (size_t)dig_kv::refl101(2 * x + i - 2, sw) * 3;
      h0 += k[i] * q[0]; h1 += k[i] * q[1]; h2 += k[i] * q[2];
    }
    a0 += k[j] * h0; a1 += k[j] * h1; a2 += k[j] * h2;
  }
  out[0] = (unsigned char)((a0 + 128) >> 8); out[1] = (unsigned char)((a1 + 128) >> 8); out[2] = (unsigned char)((a2 + 128) >> 8);
}

// motion blur (filter2D with the table's kernel of size d) of pixel (y, x) -> out[3]
DIG_HD inline void blur_pixel(const dig_abi_params& P, int d, const unsigned char* __restrict__ src, int H, int W, int y, int x,
                              unsigned char* out) {
#pragma clang fp contract(off)
  d = clampi(d, 1, DIG_ABI_MB_MAX);
  const int a = d / 2;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < d; ++j) {
    const unsigned char* row = src + (size_t)dig_kv::refl101(y + j - a, H) * W * 3;
    for (int i = 0; i < d; ++i) {
      const float k = P.mb_k[j * d + i];
      const unsigned char* q = row + (size_t)dig_kv::refl101(x + i - a, W) * 3;
      acc[0] = acc[0] + k * (float)q[0];
      acc[1] = acc[1] + k * (float)q[1];
      acc[2] = acc[2] + k * (float)q[2];
    }
  }
  for (int c = 0; c < 3; ++c) out[c] = dig_kv::round_u8(acc[c]);
}

// Gaussian noise on byte e (= 3 p + c) of image `img` with value v
DIG_HD inline unsigned char noise_byte(const dig_abi_params& P, int img, int var, long long e, unsigned char v) {
#pragma clang fp contract(off)
  const unsigned d = (unsigned)(2 * e);
  const unsigned b1 = dig_pillow::philox_first((unsigned)img, P.noise_step, d, TAG_NOISE, P.noise_key[0], P.noise_key[1]);
  const unsigned b2 = dig_pillow::philox_first((unsigned)img, P.noise_step, d + 1u, TAG_NOISE, P.noise_key[0], P.noise_key[1]);
  const double u1 = (double)((b1 >> 8) + 1u) * (1.0 / 16777216.0);
  const double u2 = (double)((float)(b2 >> 8) * (1.0f / 16777216.0f));
  const double z = sqrt(-2.0 * dig_kv::kv_log(u1)) * dig_kv::kv_cos2pi(u2);
  double t = (double)v + z * sqrt((double)(var < 0 ? 0 : var));
  t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
  return (unsigned char)(int)t;
}

// ------------------------------------------------------------------------------------------------------------------------ tail
// the jitter ops of P before (stop = 1) or all of them (stop = 0), contrast with mean cm
DIG_HD inline void jitter_ops(const dig_abi_params& P, int cm, bool stop_at_contrast, int* c) {
  for (int k = 0; k < 4; ++k) {
    const int op = P.jit_order[k];
    if (op < 0 || op > 3) continue;
    if (op == 1 && stop_at_contrast) return;
    dig_kv::jitter_apply(op, P.jit_factor, P.hue_shift, cm, c);
  }
}
DIG_HD inline bool has_contrast(const dig_abi_params& P) {
  for (int k = 0; k < 4; ++k) if (P.jit_order[k] == 1) return true;
  return false;
}

struct FetchJitter {
  const dig_abi_params* P;
  int cm;
  DIG_HD void operator()(const unsigned char* p, int c[3]) const {
    c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
    jitter_ops(*P, cm, false, c);
  }
};

// the image the tail (and the deterioration's first op) read: pointers into the crop / the image's workspace
DIG_HD inline const unsigned char* tail_src(const dig_abi_params& P, const unsigned char* crop, const unsigned char* work) {
  if (P.final_buf == 0) return crop;
  const long long rb = round256(3LL * P.wh * P.ww);
  return work + P.ws_off + (P.final_buf == 2 ? rb : 0);
}

}  // namespace dig_abi
