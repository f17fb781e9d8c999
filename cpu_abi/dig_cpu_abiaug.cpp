// libdig_cpu.so, fourth part: plain-C++ build of the ABINet augmentation entry points (include/dig_hip.h, dig_amd/csrc/abiaug.hip).  The
// sampler and the per-pixel definitions are the very functions the HIP build runs (dig_amd/csrc/abiaug.inc); the loops around them follow
// the kernels' structure: the sampler's prefix sum, the warp, one pass per deterioration launch, the tail per image.  Same contract as
// dig_cpu.cpp: `stream` ignored, every call synchronous.
#include <algorithm>
#include <vector>

#include "dig_cpu_common.h"
#include "../dig_amd/csrc/abiaug.inc"

namespace {

constexpr long long AB_MAX_PIX = 1LL << 26;

bool table_ok(const dig_abi_params& P, const dig_abi_run& R, long long work_bytes) {
  if (P.wh < 1 || P.ww < 1 || (long long)P.wh * P.ww > AB_MAX_PIX || P.ws_off < 0) return false;
  return P.ws_off + dig_abi::image_bytes(P.geom, P.det, P.wh, P.ww, R.rescale_factor) <= work_bytes;
}

}  // namespace

extern "C" {

int dig_abiaug_sample(dig_abi_params* params, long long* info, const int* heights, const int* widths, int n_img, const dig_abi_run* run,
                      unsigned long long seed, unsigned step, hipStream_t) {
  if (int rc = dig_rules::abiaug_sample(params, info, heights, widths, n_img, run, seed, step)) return rc;
#pragma omp parallel for
  for (int i = 0; i < n_img; ++i) dig_abi::sample_one(params + i, i, std::max(heights[i], 1), std::max(widths[i], 1), *run, seed, step);
  long long total = 0, mh = 0, mw = 0, cnt = 0;
  for (int i = 0; i < n_img; ++i) {
    dig_abi_params& P = params[i];
    const long long b = dig_abi::image_bytes(P.geom, P.det, P.wh, P.ww, run->rescale_factor);
    P.ws_off = total;
    total += b;
    mh = std::max<long long>(mh, P.wh);
    mw = std::max<long long>(mw, P.ww);
    cnt += b ? 1 : 0;
  }
  info[0] = total; info[1] = mh; info[2] = mw; info[3] = cnt;
  return DIG_OK;
}

long long dig_abiaug_workspace_bytes(int geom, int det, int wh, int ww, const dig_abi_run* run) {
  if (int rc = dig_rules::abiaug_workspace_bytes(geom, det, wh, ww, run)) return rc;
  return dig_abi::image_bytes(geom, det, wh, ww, run->rescale_factor);
}

int dig_abiaug_warp_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                       const dig_abi_params* params, const dig_abi_run* run, unsigned char* work, long long work_bytes, int max_wh, int max_ww,
                       hipStream_t) {
  if (int rc = dig_rules::abiaug_warp_u8(packed, offsets, heights, widths, n_img, params, run, work, work_bytes, max_wh, max_ww)) return rc;
  if (work_bytes == 0) return DIG_OK;
#pragma omp parallel for schedule(dynamic)
  for (int img = 0; img < n_img; ++img) {
    const dig_abi_params& P = params[img];
    if (!P.geom || !table_ok(P, *run, work_bytes)) continue;
    const unsigned char* src = packed + offsets[img];
    unsigned char* dst = work + P.ws_off;
    for (int p = 0; p < P.wh * P.ww; ++p) dig_abi::warp_pixel(P, src, heights[img], widths[img], p / P.ww, p % P.ww, dst + 3 * (size_t)p);
  }
  return DIG_OK;
}

int dig_abiaug_deteriorate_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                              const dig_abi_params* params, const dig_abi_run* run, unsigned char* work, long long work_bytes, int max_wh,
                              int max_ww, hipStream_t) {
  if (int rc = dig_rules::abiaug_deteriorate_u8(packed, offsets, heights, widths, n_img, params, run, work, work_bytes, max_wh, max_ww)) return rc;
  if (work_bytes == 0) return DIG_OK;
  const dig_abi_run R = *run;
#pragma omp parallel for schedule(dynamic)
  for (int img = 0; img < n_img; ++img) {
    const dig_abi_params& P = params[img];
    if (!P.det || !table_ok(P, R, work_bytes)) continue;
    const int wh = P.geom ? P.wh : heights[img], ww = P.geom ? P.ww : widths[img];
    if (!P.geom && (wh != P.wh || ww != P.ww)) continue;
    const long long rb = dig_abi::round256(3LL * wh * ww);
    unsigned char* A = work + P.ws_off;
    unsigned char* B = A + rb;
    unsigned char* R0 = A + 2 * rb;
    unsigned char* R1 = R0 + 3LL * dig_abi::RS_H * dig_abi::RS_W;
    for (int j = 0; j < dig_abi::n_det_ops(R); ++j) {
      const unsigned char* src = j == 0 ? (P.geom ? A : packed + offsets[img]) : (((j - 1) & 1) ? A : B);
      unsigned char* dst = (j & 1) ? A : B;
      const int op = dig_abi::det_op(R, j);
      if (op == 0) {
        for (long long e = 0; e < 3LL * wh * ww; ++e) dst[e] = dig_abi::noise_byte(P, img, R.noise_var, e, src[e]);
      } else if (op == 1) {
        for (int p = 0; p < wh * ww; ++p) dig_abi::blur_pixel(P, R.mb_size, src, wh, ww, p / ww, p % ww, dst + 3 * (size_t)p);
      } else {
        for (int p = 0; p < dig_abi::RS_H * dig_abi::RS_W; ++p)
          dig_abi::resize_cv_pixel(src, wh, ww, dig_abi::RS_H, dig_abi::RS_W, P.rs_interp[0], p / dig_abi::RS_W, p % dig_abi::RS_W, R0 + 3 * (size_t)p);
        for (int l = 1; l <= R.rescale_factor; ++l) {
          const unsigned char* s = ((l - 1) & 1) ? R1 : R0;
          unsigned char* d = (l & 1) ? R1 : R0;
          const int sh = dig_abi::RS_H >> (l - 1), sw = dig_abi::RS_W >> (l - 1);
          for (int p = 0; p < (sh / 2) * (sw / 2); ++p) dig_abi::pyrdown_pixel(s, sh, sw, p / (sw / 2), p % (sw / 2), d + 3 * (size_t)p);
        }
        const int f = R.rescale_factor;
        const unsigned char* s = (f & 1) ? R1 : R0;
        for (int p = 0; p < wh * ww; ++p)
          dig_abi::resize_cv_pixel(s, dig_abi::RS_H >> f, dig_abi::RS_W >> f, wh, ww, P.rs_interp[1], p / ww, p % ww, dst + 3 * (size_t)p);
      }
    }
  }
  return DIG_OK;
}

int dig_abiaug_tail(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                    const dig_abi_params* params, const dig_abi_run* run, const unsigned char* work, long long work_bytes, float* out, int out_h,
                    int out_w, float mean, float std_, int max_wh, int max_ww, hipStream_t) {
  if (int rc = dig_rules::abiaug_tail(packed, offsets, heights, widths, n_img, params, run, work, work_bytes, out, out_h, out_w, mean, std_, max_wh,
                                      max_ww))
    return rc;
  const int ksh = dig_pillow::ksize_for(max_ww, out_w), ksv = dig_pillow::ksize_for(max_wh, out_h);
#pragma omp parallel for
  for (int img = 0; img < n_img; ++img) {
    const dig_abi_params& P = params[img];
    const bool crop = P.final_buf == 0;
    if (!crop && !table_ok(P, *run, work_bytes)) continue;
    if (P.final_buf < 0 || P.final_buf > 2 || (P.final_buf == 2 && !P.det) || (P.final_buf == 1 && !P.geom && !P.det)) continue;
    const int h = crop ? heights[img] : P.wh, w = crop ? widths[img] : P.ww;
    if (h > max_wh || w > max_ww) continue;
    const unsigned char* src = dig_abi::tail_src(P, packed + offsets[img], work);
    std::vector<int> kh((size_t)out_w * ksh), bh(2 * (size_t)out_w), kv((size_t)out_h * ksv), bv(2 * (size_t)out_h);
    for (int t = 0; t < out_w; ++t) dig_pillow::coeffs_for(t, w, out_w, ksh, kh.data(), bh.data());
    for (int t = 0; t < out_h; ++t) dig_pillow::coeffs_for(t, h, out_h, ksv, kv.data(), bv.data());
    const bool jit = P.jit != 0;
    int cm = 0;
    if (jit && dig_abi::has_contrast(P)) {
      long long s = 0;
      for (int p = 0; p < h * w; ++p) {
        int c[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
        dig_abi::jitter_ops(P, 0, true, c);
        s += dig_kv::luma(c[0], c[1], c[2]);
      }
      cm = dig_kv::contrast_mean(s, h * w);
    }
    const int plane = out_h * out_w;
    float* o = out + (size_t)img * 3 * plane;
    for (int p = 0; p < plane; ++p) {
      int r[3];
      if (jit)
        dig_pillow::resize_pixel_f(src, w, w != out_w, h != out_h, kh.data(), bh.data(), kv.data(), bv.data(), ksh, ksv, p / out_w, p % out_w,
                                   r, dig_abi::FetchJitter{&P, cm});
      else
        dig_pillow::resize_pixel(src, w, w != out_w, h != out_h, kh.data(), bh.data(), kv.data(), bv.data(), ksh, ksv, p / out_w, p % out_w, r);
      for (int k = 0; k < 3; ++k) o[(size_t)k * plane + p] = ((float)r[k] / 255.0f - mean) / std_;
    }
  }
  return DIG_OK;
}

}  // extern "C"
