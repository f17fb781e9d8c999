// Key-view augmentation on the device: the second (key) view of MoCo pre-training built from the crops already uploaded for the first
// view (dataset/dataset_image.py:39-50,88-120,145-149 of the reference).  Semantics, table layout and rounding: keyview.inc and
// include/dig_aug_types.h; tests/keyview_model.py is the numpy statement of both stages.
//
//   dig_keyview_sample   : one thread per image draws its dig_kv_params table (Philox4x32-10, counter (image, step, draw, TAG)).
//   dig_keyview_stage_a_u8: the seqCLR ops at the crop's resolution, one launch per op position (5 launches).  The workspace holds two
//       copies of the packed layout; launch L writes half L & 1 from the crop or the other half, and every image's ops are right-aligned
//       so its last op lands in half 0 (keyview.inc op_at_launch).  `packed` stays read-only: the first view is resized from it too.
//       Grid (image, slice): `slice` workgroups share an image's pixels, so 128 crops still spread over the 256 CUs.  Pointwise ops
//       read their own pixel; the stencils (blur, sharpen) and the resamplers read their neighbourhood / source pixels straight from
//       global memory through L1 / L2 (the crop's rows are reused by the workgroup that owns them).
//   dig_keyview_stage_b  : one workgroup per image: Pillow's bicubic resize to out_h x out_w into LDS (uint8, 3 planes), the ColorJitter
//       ops in the image's order (contrast: one LDS integer sum of L), RandomGrayscale, ToTensor + Normalize to fp32 [n, 3, out_h, out_w].
//       Every thread owns the same pixels through all passes, so only the coefficient tables and the contrast sum need a barrier.
//
// Integer / uint8 work and float32 per-pixel arithmetic only (`#pragma clang fp contract(off)` in keyview.inc): bit-exact with the model.
#include <hip/hip_runtime.h>

#include "common.h"
#include "keyview.inc"

namespace {

constexpr int KV_THREADS = 256;

__global__ __launch_bounds__(64) void keyview_sample_kernel(dig_kv_params* __restrict__ params, const int* __restrict__ heights,
                                                            const int* __restrict__ widths, int n_img, unsigned long long seed, unsigned step) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_img) return;
  dig_kv::sample_one(params + i, i, max(heights[i], 1), max(widths[i], 1), seed, step);
}

__global__ __launch_bounds__(KV_THREADS) void keyview_stage_a_kernel(int L, const unsigned char* __restrict__ packed,
                                                                     unsigned char* __restrict__ work, long long half,
                                                                     const long long* __restrict__ offsets, const int* __restrict__ heights,
                                                                     const int* __restrict__ widths, const dig_kv_params* __restrict__ params) {
  const int img = blockIdx.x;
  const dig_kv_params& P = params[img];
  int j;
  const int op = dig_kv::op_at_launch(P, L, &j);
  if (op == -1) return;
  const int H = heights[img], W = widths[img];
  const long long off = offsets[img];
  unsigned char* dst = work + ((L & 1) ? half : 0) + off;
  const unsigned char* src = (op == -2 || j == 0) ? packed + off : work + ((L & 1) ? 0 : half) + off;
  const int npix = H * W;
  const int stride = gridDim.y * KV_THREADS;
  if (op == -2) {
    for (int b = blockIdx.y * KV_THREADS + threadIdx.x; b < 3 * npix; b += stride) dst[b] = src[b];
    return;
  }
  for (int p = blockIdx.y * KV_THREADS + threadIdx.x; p < npix; p += stride) {
    const int y = p / W, x = p - y * W;
    unsigned char o[3];
    dig_kv::op_pixel(op, P, src, H, W, y, x, o);
    dst[3 * p] = o[0];
    dst[3 * p + 1] = o[1];
    dst[3 * p + 2] = o[2];
  }
}

__global__ __launch_bounds__(KV_THREADS) void keyview_stage_b_kernel(const unsigned char* __restrict__ stage_a, const long long* __restrict__ offsets,
                                                                     const int* __restrict__ heights, const int* __restrict__ widths,
                                                                     const dig_kv_params* __restrict__ params, float* __restrict__ out,
                                                                     int out_h, int out_w, int ksh, int ksv, float mean, float stdv) {
  extern __shared__ int lds[];
  int* kh = lds;                               // [out_w][ksh]
  int* bh = kh + out_w * ksh;                  // [out_w][2]
  int* kv = bh + 2 * out_w;                    // [out_h][ksv]
  int* bv = kv + out_h * ksv;                  // [out_h][2]
  const int ints = out_w * (ksh + 2) + out_h * (ksv + 2);
  unsigned long long* lsum = reinterpret_cast<unsigned long long*>(lds + ints + (ints & 1));   // [4] contrast sums, 8-byte aligned
  const int plane = out_h * out_w;
  unsigned char* pix = reinterpret_cast<unsigned char*>(lsum + 4);   // [3][plane]
  const int img = blockIdx.x;
  const dig_kv_params& P = params[img];
  const int h = heights[img], w = widths[img];
  const unsigned char* src = stage_a + offsets[img];
  for (int t = threadIdx.x; t < out_w + out_h; t += blockDim.x) {
    if (t < out_w) dig_pillow::coeffs_for(t, w, out_w, ksh, kh, bh);
    else dig_pillow::coeffs_for(t - out_w, h, out_h, ksv, kv, bv);
  }
  if (threadIdx.x < 4) lsum[threadIdx.x] = 0ull;
  __syncthreads();
  const bool pass_h = (w != out_w), pass_v = (h != out_h);
  for (int p = threadIdx.x; p < plane; p += blockDim.x) {
    const int yy = p / out_w, xx = p - yy * out_w;
    int r[3];
    dig_pillow::resize_pixel(src, w, pass_h, pass_v, kh, bh, kv, bv, ksh, ksv, yy, xx, r);
    pix[p] = (unsigned char)r[0];
    pix[plane + p] = (unsigned char)r[1];
    pix[2 * plane + p] = (unsigned char)r[2];
  }
  // (no barrier: from here on every thread reads and writes only the pixels it resized)
  if (P.jitter) {
    for (int k = 0; k < 4; ++k) {
      const int op = P.jit_order[k];
      if (op < 0 || op > 3) continue;                   // (a hand-built table may leave positions empty)
      int cm = 0;
      if (op == 1) {
        unsigned long long s = 0;
        for (int p = threadIdx.x; p < plane; p += blockDim.x) s += (unsigned long long)dig_kv::luma(pix[p], pix[plane + p], pix[2 * plane + p]);
        atomicAdd(&lsum[k], s);
        __syncthreads();
        cm = dig_kv::contrast_mean((long long)lsum[k], plane);
      }
      for (int p = threadIdx.x; p < plane; p += blockDim.x) {
        int c[3] = {pix[p], pix[plane + p], pix[2 * plane + p]};
        dig_kv::jitter_pixel(op, P, cm, c);
        pix[p] = (unsigned char)c[0];
        pix[plane + p] = (unsigned char)c[1];
        pix[2 * plane + p] = (unsigned char)c[2];
      }
    }
  }
  float* o = out + (size_t)img * 3 * plane;
  for (int p = threadIdx.x; p < plane; p += blockDim.x) {
    int c0 = pix[p], c1 = pix[plane + p], c2 = pix[2 * plane + p];
    if (P.gray) c0 = c1 = c2 = dig_kv::luma(c0, c1, c2);
    // ToTensor: uint8 / 255 in fp32; Normalize: (x - mean) / std, as input.hip
    o[p] = ((float)c0 / 255.0f - mean) / stdv;
    o[plane + p] = ((float)c1 / 255.0f - mean) / stdv;
    o[2 * plane + p] = ((float)c2 / 255.0f - mean) / stdv;
  }
}

}  // namespace

// C-ABI: see include/dig_hip.h
extern "C" int dig_keyview_sample(dig_kv_params* params, const int* heights, const int* widths, int n_img, unsigned long long seed, unsigned step,
                                  hipStream_t stream) {
  if (int rc = dig_rules::keyview_sample(params, heights, widths, n_img, seed, step)) return rc;
  hipLaunchKernelGGL(keyview_sample_kernel, dim3((n_img + 63) / 64), dim3(64), 0, stream, params, heights, widths, n_img, seed, step);
  return dig_check_launch();
}

extern "C" long long dig_keyview_workspace_bytes(long long packed_bytes, int n_img) {
  if (int rc = dig_rules::keyview_workspace_bytes(packed_bytes, n_img)) return rc;
  return 2 * ((packed_bytes + 255) / 256 * 256);
}

extern "C" int dig_keyview_stage_a_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                                      const dig_kv_params* params, unsigned char* work, long long work_bytes, int max_h, int max_w,
                                      hipStream_t stream) {
  if (int rc = dig_rules::keyview_stage_a_u8(packed, offsets, heights, widths, n_img, params, work, work_bytes, max_h, max_w)) return rc;
  const long long npix = (long long)max_h * max_w;
  const int slices = (int)std::min<long long>(16, std::max<long long>(1, npix / (4 * KV_THREADS)));
  for (int L = 0; L < dig_kv::N_LAUNCH; ++L) {
    hipLaunchKernelGGL(keyview_stage_a_kernel, dim3(n_img, slices), dim3(KV_THREADS), 0, stream, L, packed, work, work_bytes / 2, offsets,
                       heights, widths, params);
    const int rc = dig_check_launch();
    if (rc) return rc;
  }
  return DIG_OK;
}

extern "C" int dig_keyview_stage_b(const unsigned char* stage_a, const long long* offsets, const int* heights, const int* widths, int n_img,
                                   const dig_kv_params* params, float* out, int out_h, int out_w, float mean, float std_, int max_h, int max_w,
                                   hipStream_t stream) {
  if (int rc = dig_rules::keyview_stage_b(stage_a, offsets, heights, widths, n_img, params, out, out_h, out_w, mean, std_, max_h, max_w)) return rc;
  const int ksh = dig_pillow::ksize_for(max_w, out_w), ksv = dig_pillow::ksize_for(max_h, out_h);
  const size_t lds = dig_kv::stage_b_lds_bytes(out_h, out_w, ksh, ksv);
  static size_t attr = 0;
  if (lds > attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(keyview_stage_b_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = lds;
  }
  hipLaunchKernelGGL(keyview_stage_b_kernel, dim3(n_img), dim3(KV_THREADS), lds, stream, stage_a, offsets, heights, widths, params, out, out_h,
                     out_w, ksh, ksv, mean, std_);
  return dig_check_launch();
}
