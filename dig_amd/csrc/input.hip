// Input transform on the device: the step either side of the hot path.
//
//   dig_resize_bicubic_normalize_u8 : uint8 RGB crops of any size -> fp32 [n, 3, out_h, out_w], bit-exact with
//       transforms.Resize((h, w), interpolation=3) + ToTensor + Normalize(mean, std) of the reference
//       (dataset/datasets.py:27-42 on the PIL crops of dataset/dataset_image.py:128-160).  Resize on a PIL image is
//       Pillow's ImagingResample: separable horizontal-then-vertical passes on 8-bit pixels, double-precision bicubic
//       (a = -0.5) coefficients over a support of 2*max(scale,1), normalised, rounded to 22-bit fixed point, int32
//       accumulation from 1<<21, clip to [0,255] after >>22 (pillow_resize.h; restated in oracle/input_oracle.py, pinned against Pillow).
//   dig_random_masks : RandomMaskingGenerator (masking_generator.py:12-49) as a device generator: each row is a uniformly
//       random subset of exactly num_mask patches, chosen as the num_mask smallest Philox4x32-10 keys.
//
// HBM-bound integer work: one workgroup per crop; the fixed-point coefficient tables live in LDS; each thread produces
// output pixels (all three channels) by evaluating the horizontal pass on the fly for the rows its vertical window needs
// (an 8-bit intermediate exactly as Pillow's), so no intermediate image goes to memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "pillow_resize.h"

namespace {

using dig_pillow::coeffs_for;
using dig_pillow::ksize_for;
using dig_pillow::philox_first;

__global__ __launch_bounds__(256) void resize_normalize_kernel(const unsigned char* __restrict__ packed,
                                                               const long long* __restrict__ offsets,
                                                               const int* __restrict__ heights, const int* __restrict__ widths,
                                                               float* __restrict__ out, int out_h, int out_w, int ksh, int ksv,
                                                               float mean, float stdv) {
  extern __shared__ int lds[];
  int* kh = lds;                               // [out_w][ksh]
  int* bh = kh + out_w * ksh;                  // [out_w][2]
  int* kv = bh + 2 * out_w;                    // [out_h][ksv]
  int* bv = kv + out_h * ksv;                  // [out_h][2]
  const int img = blockIdx.x;
  const int h = heights[img], w = widths[img];
  const unsigned char* src = packed + offsets[img];
  for (int t = threadIdx.x; t < out_w + out_h; t += blockDim.x) {
    if (t < out_w) coeffs_for(t, w, out_w, ksh, kh, bh);
    else coeffs_for(t - out_w, h, out_h, ksv, kv, bv);
  }
  __syncthreads();
  const bool pass_h = (w != out_w), pass_v = (h != out_h);        // ImagingResample skips a pass that keeps the size
  const size_t plane = (size_t)out_h * out_w;
  float* o = out + (size_t)img * 3 * plane;
  for (int p = threadIdx.x; p < out_h * out_w; p += blockDim.x) {
    const int yy = p / out_w, xx = p - yy * out_w;
    int r[3];
    dig_pillow::resize_pixel(src, w, pass_h, pass_v, kh, bh, kv, bv, ksh, ksv, yy, xx, r);
    const int r0 = r[0], r1 = r[1], r2 = r[2];
    // ToTensor: uint8 / 255 in fp32; Normalize: (x - mean) / std  (IEEE division: this file is built without fast-math)
    o[p] = ((float)r0 / 255.0f - mean) / stdv;
    o[plane + p] = ((float)r1 / 255.0f - mean) / stdv;
    o[2 * plane + p] = ((float)r2 / 255.0f - mean) / stdv;
  }
}

// one wave per mask row: the num_mask patches with the smallest (key, index) are set
__global__ __launch_bounds__(64) void random_masks_kernel(unsigned char* __restrict__ mask, int n_patches, int num_mask, unsigned k0,
                                                          unsigned k1, unsigned step) {
  extern __shared__ unsigned keys[];
  const int r = blockIdx.x, lane = threadIdx.x;
  for (int p = lane; p < n_patches; p += 64) keys[p] = philox_first((unsigned)r, (unsigned)p, step, 0u, k0, k1);
  __syncthreads();
  for (int p = lane; p < n_patches; p += 64) {
    const unsigned mine = keys[p];
    int rank = 0;
    for (int q = 0; q < n_patches; ++q) {
      const unsigned kq = keys[q];
      rank += (kq < mine) || (kq == mine && q < p);
    }
    mask[(size_t)r * n_patches + p] = rank < num_mask ? 1 : 0;
  }
}

}  // namespace

// C-ABI: see include/dig_hip.h
extern "C" int dig_resize_bicubic_normalize_u8(const unsigned char* packed, const long long* offsets, const int* heights,
                                               const int* widths, int n_img, float* out, int out_h, int out_w, float mean,
                                               float std_, int max_h, int max_w, hipStream_t stream) {
  if (int rc = dig_rules::resize_bicubic_normalize_u8(packed, offsets, heights, widths, n_img, out, out_h, out_w, mean, std_, max_h, max_w))
    return rc;
  const int ksh = ksize_for(max_w, out_w), ksv = ksize_for(max_h, out_h);
  const size_t lds = dig_rules::resize_lds_bytes(out_h, out_w, ksh, ksv);
  static size_t attr = 0;
  if (lds > attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(resize_normalize_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = lds;
  }
  hipLaunchKernelGGL(resize_normalize_kernel, dim3(n_img), dim3(256), lds, stream, packed, offsets, heights, widths, out, out_h, out_w,
                     ksh, ksv, mean, std_);
  return dig_check_launch();
}

extern "C" int dig_random_masks(unsigned char* mask, int n_rows, int n_patches, int num_mask, unsigned long long seed,
                                unsigned step, hipStream_t stream) {
  if (int rc = dig_rules::random_masks(mask, n_rows, n_patches, num_mask, seed, step)) return rc;
  hipLaunchKernelGGL(random_masks_kernel, dim3(n_rows), dim3(64), n_patches * sizeof(unsigned), stream, mask, n_patches, num_mask,
                     (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), step);
  return dig_check_launch();
}
