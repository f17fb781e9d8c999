// Pillow's bicubic resize of 8-bit RGB (ImagingResample) and the Philox4x32-10 counter hash: the pieces the input transform (input.hip)
// and the key-view augmentation (keyview.hip) share.  Host-and-device code (plain C++ where no HIP compiler is in use), so the plain-C++
// build of the key-view entry points compiles the very same functions.
//
// Resize: separable horizontal-then-vertical passes on 8-bit pixels, double-precision bicubic (a = -0.5) coefficients over a support of
// 2*max(scale,1), normalised, rounded to 22-bit fixed point, int32 accumulation from 1<<21, clip to [0,255] after >>22 (restated in
// oracle/input_oracle.py, pinned against Pillow).  A pass that keeps the size is skipped, as ImagingResample does.
#pragma once

#if defined(__HIPCC__)
#define DIG_HD __host__ __device__
#else
#define DIG_HD
#endif

#include <cmath>

#include "abi_rules.h"

namespace dig_pillow {

constexpr int PRECISION_BITS = 32 - 8 - 2;

DIG_HD inline double bicubic_filter(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for output index xx (same operation order, no FMA contraction)
DIG_HD inline void coeffs_for(int xx, int in_size, int out_size, int ksize, int* __restrict__ kk, int* __restrict__ bounds) {
#pragma clang fp contract(off)
  double scale = (double)in_size / (double)out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 2.0 * filterscale;
  const double center = ((double)xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += bicubic_filter(((double)(x + xmin) - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double w = bicubic_filter(((double)(x + xmin) - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    kk[xx * ksize + x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
  }
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

DIG_HD inline int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

using dig_rules::ksize_for;   // taps per output index of one axis for inputs up to in_size (abi_rules.h: the LDS rules need it too)

// the three channels of output pixel (yy, xx) of an HWC uint8 image (h x w at src): the horizontal pass is evaluated on the fly for the
// rows the vertical window needs (an 8-bit intermediate exactly as Pillow's).  kh / bh: [out_w][ksh] / [out_w][2], kv / bv: [out_h][ksv] /
// [out_h][2] from coeffs_for.
// `fetch(row pointer of pixel, c[3])` yields the three channels of one source pixel: the identity below, or a per-pixel pass applied on
// the fly (the ABINet augmentation's ColorJitter at the source resolution).
struct FetchU8 {
  DIG_HD void operator()(const unsigned char* p, int c[3]) const { c[0] = p[0]; c[1] = p[1]; c[2] = p[2]; }
};
template <class Fetch>
DIG_HD inline void resize_pixel_f(const unsigned char* __restrict__ src, int w, bool pass_h, bool pass_v, const int* kh, const int* bh,
                                  const int* kv, const int* bv, int ksh, int ksv, int yy, int xx, int r[3], const Fetch& fetch) {
  const int x0 = pass_h ? bh[2 * xx] : xx, nx = pass_h ? bh[2 * xx + 1] : 1;
  const int y0 = pass_v ? bv[2 * yy] : yy, ny = pass_v ? bv[2 * yy + 1] : 1;
  const int* kx = kh + xx * ksh;
  const int* ky = kv + yy * ksv;
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  int r0 = 0, r1 = 0, r2 = 0;
  for (int y = 0; y < ny; ++y) {
    const unsigned char* row = src + ((size_t)(y0 + y) * w + x0) * 3;
    int h0, h1, h2;
    if (pass_h) {
      int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
      for (int x = 0; x < nx; ++x) {
        const int k = kx[x];
        int c[3];
        fetch(row + 3 * x, c);
        s0 += c[0] * k;
        s1 += c[1] * k;
        s2 += c[2] * k;
      }
      h0 = clip8(s0); h1 = clip8(s1); h2 = clip8(s2);
    } else {
      int c[3];
      fetch(row, c);
      h0 = c[0]; h1 = c[1]; h2 = c[2];
    }
    if (pass_v) {
      const int k = ky[y];
      a0 += h0 * k; a1 += h1 * k; a2 += h2 * k;
    } else {
      r0 = h0; r1 = h1; r2 = h2;
    }
  }
  if (pass_v) { r0 = clip8(a0); r1 = clip8(a1); r2 = clip8(a2); }
  r[0] = r0; r[1] = r1; r[2] = r2;
}
DIG_HD inline void resize_pixel(const unsigned char* __restrict__ src, int w, bool pass_h, bool pass_v, const int* kh, const int* bh,
                                const int* kv, const int* bv, int ksh, int ksv, int yy, int xx, int r[3]) {
  resize_pixel_f(src, w, pass_h, pass_v, kh, bh, kv, bv, ksh, ksv, yy, xx, r, FetchU8{});
}

// Philox4x32-10, first output word of counter (c0, c1, c2, c3) under key (k0, k1)
DIG_HD inline unsigned philox_first(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

}  // namespace dig_pillow
