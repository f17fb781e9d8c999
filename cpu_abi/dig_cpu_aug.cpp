// libdig_cpu.so, third part: plain-C++ build of the key-view augmentation entry points (include/dig_hip.h, dig_amd/csrc/keyview.hip).  The
// sampler and the per-pixel definitions are the very functions the HIP build runs (dig_amd/csrc/keyview.inc, pillow_resize.h); the
// loops around them follow the kernels' structure: five stage-A passes ping-ponging between the two halves of the workspace, then
// stage B per image.  Same contract as dig_cpu.cpp: `stream` ignored, every call synchronous.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "dig_cpu_common.h"
#include "../dig_amd/csrc/keyview.inc"

extern "C" {

int dig_keyview_sample(dig_kv_params* params, const int* heights, const int* widths, int n_img, unsigned long long seed, unsigned step,
                       hipStream_t) {
  if (int rc = dig_rules::keyview_sample(params, heights, widths, n_img, seed, step)) return rc;
#pragma omp parallel for
  for (int i = 0; i < n_img; ++i) dig_kv::sample_one(params + i, i, std::max(heights[i], 1), std::max(widths[i], 1), seed, step);
  return DIG_OK;
}

long long dig_keyview_workspace_bytes(long long packed_bytes, int n_img) {
  if (int rc = dig_rules::keyview_workspace_bytes(packed_bytes, n_img)) return rc;
  return 2 * ((packed_bytes + 255) / 256 * 256);
}

int dig_keyview_stage_a_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                           const dig_kv_params* params, unsigned char* work, long long work_bytes, int max_h, int max_w, hipStream_t) {
  if (int rc = dig_rules::keyview_stage_a_u8(packed, offsets, heights, widths, n_img, params, work, work_bytes, max_h, max_w)) return rc;
  const long long half = work_bytes / 2;
  for (int L = 0; L < dig_kv::N_LAUNCH; ++L) {
#pragma omp parallel for schedule(dynamic)
    for (int img = 0; img < n_img; ++img) {
      const dig_kv_params& P = params[img];
      int j;
      const int op = dig_kv::op_at_launch(P, L, &j);
      if (op == -1) continue;
      const int H = heights[img], W = widths[img];
      const long long off = offsets[img];
      unsigned char* dst = work + ((L & 1) ? half : 0) + off;
      const unsigned char* src = (op == -2 || j == 0) ? packed + off : work + ((L & 1) ? 0 : half) + off;
      if (op == -2) {
        std::copy(src, src + (size_t)3 * H * W, dst);
        continue;
      }
      for (int p = 0; p < H * W; ++p) dig_kv::op_pixel(op, P, src, H, W, p / W, p % W, dst + 3 * (size_t)p);
    }
  }
  return DIG_OK;
}

int dig_keyview_stage_b(const unsigned char* stage_a, const long long* offsets, const int* heights, const int* widths, int n_img,
                        const dig_kv_params* params, float* out, int out_h, int out_w, float mean, float std_, int max_h, int max_w, hipStream_t) {
  if (int rc = dig_rules::keyview_stage_b(stage_a, offsets, heights, widths, n_img, params, out, out_h, out_w, mean, std_, max_h, max_w)) return rc;
  const int ksh = dig_pillow::ksize_for(max_w, out_w), ksv = dig_pillow::ksize_for(max_h, out_h);
#pragma omp parallel for
  for (int img = 0; img < n_img; ++img) {
    const dig_kv_params& P = params[img];
    const int h = heights[img], w = widths[img];
    const unsigned char* src = stage_a + offsets[img];
    std::vector<int> kh((size_t)out_w * ksh), bh(2 * (size_t)out_w), kv((size_t)out_h * ksv), bv(2 * (size_t)out_h);
    for (int t = 0; t < out_w; ++t) dig_pillow::coeffs_for(t, w, out_w, ksh, kh.data(), bh.data());
    for (int t = 0; t < out_h; ++t) dig_pillow::coeffs_for(t, h, out_h, ksv, kv.data(), bv.data());
    const int plane = out_h * out_w;
    std::vector<int> pix((size_t)3 * plane);
    for (int p = 0; p < plane; ++p)
      dig_pillow::resize_pixel(src, w, w != out_w, h != out_h, kh.data(), bh.data(), kv.data(), bv.data(), ksh, ksv, p / out_w, p % out_w,
                               &pix[3 * (size_t)p]);
    if (P.jitter) {
      for (int k = 0; k < 4; ++k) {
        const int op = P.jit_order[k];
        if (op < 0 || op > 3) continue;
        int cm = 0;
        if (op == 1) {
          long long s = 0;
          for (int p = 0; p < plane; ++p) s += dig_kv::luma(pix[3 * p], pix[3 * p + 1], pix[3 * p + 2]);
          cm = dig_kv::contrast_mean(s, plane);
        }
        for (int p = 0; p < plane; ++p) dig_kv::jitter_pixel(op, P, cm, &pix[3 * (size_t)p]);
      }
    }
    float* o = out + (size_t)img * 3 * plane;
    for (int p = 0; p < plane; ++p) {
      int c[3] = {pix[3 * p], pix[3 * p + 1], pix[3 * p + 2]};
      if (P.gray) c[0] = c[1] = c[2] = dig_kv::luma(c[0], c[1], c[2]);
      for (int k = 0; k < 3; ++k) o[(size_t)k * plane + p] = ((float)c[k] / 255.0f - mean) / std_;
    }
  }
  return DIG_OK;
}

}  // extern "C"
