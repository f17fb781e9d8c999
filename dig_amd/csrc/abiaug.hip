// ABINet augmentation of fine-tuning on the device (--num_view 2 --use_abi_aug; transforms.py:188-504 of the reference): CVGeometry,
// CVDeterioration, CVColorJitter, Resize((32, 128), BICUBIC), ToTensor, Normalize on the crops of one packed upload.  Semantics, rounding
// and the workspace layout: abiaug.inc; table layout: include/dig_aug_types.h; tests/abiaug_model.py is the numpy statement.
//
//   dig_abiaug_sample      : one workgroup.  Each thread draws the tables of a chunk's images (Philox4x32-10) with their warped size;
//       a workgroup scan turns the images' workspace bytes into offsets; info = (total bytes, max warped height, max warped width, images
//       with a workspace).
//   dig_abiaug_warp_u8     : grid (slice, image); a workgroup of an image whose geometry gate is off returns at once.  Each thread maps its
//       output pixels through minv and samples the crop (nearest / linear / cubic taps, 11-bit integer weights, replicated border).
//   dig_abiaug_deteriorate_u8: the run's noise / motion blur / rescale in order, one launch per op (the rescale: resize up, `factor`
//       pyrDowns, resize back), grid (slice, image), early exit on the deterioration gate.  Reads and writes ping-pong in the image's
//       workspace; stencil and resampler taps come through L1 / L2.
//   dig_abiaug_tail        : one workgroup per image, as key-view stage B: Pillow's coefficient tables in LDS, the contrast mean of the
//       jittered image (one LDS sum), then Pillow's bicubic resize with the jitter ops applied to each source pixel as it is read,
//       ToTensor + Normalize into fp32 [n, 3, out_h, out_w].
//
// Compiled with -ffp-contract=off (dig_amd/build.py): float32 / double arithmetic as abiaug.inc writes it, bit-exact with the CPU build.
#include <hip/hip_runtime.h>

#include "common.h"
#include "abiaug.inc"

namespace {

constexpr int AB_THREADS = 256;
constexpr long long AB_MAX_PIX = 1LL << 26;                 // a warped image larger than this is a bad table: skipped

__device__ inline bool table_ok(const dig_abi_params& P, const dig_abi_run& R, long long work_bytes) {
  if (P.wh < 1 || P.ww < 1 || (long long)P.wh * P.ww > AB_MAX_PIX || P.ws_off < 0) return false;
  return P.ws_off + dig_abi::image_bytes(P.geom, P.det, P.wh, P.ww, R.rescale_factor) <= work_bytes;
}

__global__ __launch_bounds__(AB_THREADS) void abiaug_sample_kernel(dig_abi_params* __restrict__ params, long long* __restrict__ info,
                                                                   const int* __restrict__ heights, const int* __restrict__ widths, int n_img,
                                                                   dig_abi_run run, unsigned long long seed, unsigned step) {
  __shared__ long long scan[AB_THREADS];
  __shared__ int mx[2], cnt;
  long long carry = 0;
  if (threadIdx.x == 0) { mx[0] = 0; mx[1] = 0; cnt = 0; }
  __syncthreads();
  for (int base = 0; base < n_img; base += AB_THREADS) {
    const int i = base + threadIdx.x;
    long long bytes = 0;
    if (i < n_img) {
      dig_abi_params& P = params[i];
      dig_abi::sample_one(&P, i, max(heights[i], 1), max(widths[i], 1), run, seed, step);
      bytes = dig_abi::image_bytes(P.geom, P.det, P.wh, P.ww, run.rescale_factor);
      atomicMax(&mx[0], P.wh);
      atomicMax(&mx[1], P.ww);
      if (bytes) atomicAdd(&cnt, 1);
    }
    scan[threadIdx.x] = bytes;
    __syncthreads();
    for (int o = 1; o < AB_THREADS; o <<= 1) {                // inclusive Hillis-Steele scan
      const long long v = threadIdx.x >= o ? scan[threadIdx.x - o] : 0;
      __syncthreads();
      scan[threadIdx.x] += v;
      __syncthreads();
    }
    if (i < n_img) params[i].ws_off = carry + scan[threadIdx.x] - bytes;
    carry += scan[AB_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) { info[0] = carry; info[1] = mx[0]; info[2] = mx[1]; info[3] = cnt; }
}

__global__ __launch_bounds__(AB_THREADS) void abiaug_warp_kernel(const unsigned char* __restrict__ packed, const long long* __restrict__ offsets,
                                                                 const int* __restrict__ heights, const int* __restrict__ widths,
                                                                 const dig_abi_params* __restrict__ params, dig_abi_run run,
                                                                 unsigned char* __restrict__ work, long long work_bytes) {
  const int img = blockIdx.y;
  const dig_abi_params& P = params[img];
  if (!P.geom || !table_ok(P, run, work_bytes)) return;
  const int H = heights[img], W = widths[img], wh = P.wh, ww = P.ww;
  const unsigned char* src = packed + offsets[img];
  unsigned char* dst = work + P.ws_off;
  const int npix = wh * ww;
  for (int p = blockIdx.x * AB_THREADS + threadIdx.x; p < npix; p += gridDim.x * AB_THREADS) {
    const int y = p / ww, x = p - y * ww;
    dig_abi::warp_pixel(P, src, H, W, y, x, dst + 3 * (size_t)p);
  }
}

// one deterioration launch: op position j of the run; kind 0 noise, 1 blur, 2 resize to 128 x 512, 3 pyrDown to level `lvl`, 4 resize back
__global__ __launch_bounds__(AB_THREADS) void abiaug_det_kernel(int kind, int j, int lvl, const unsigned char* __restrict__ packed,
                                                                const long long* __restrict__ offsets, const int* __restrict__ heights,
                                                                const int* __restrict__ widths, const dig_abi_params* __restrict__ params,
                                                                dig_abi_run run, unsigned char* __restrict__ work, long long work_bytes) {
  const int img = blockIdx.y;
  const dig_abi_params& P = params[img];
  if (!P.det || !table_ok(P, run, work_bytes)) return;
  const int wh = P.geom ? P.wh : heights[img], ww = P.geom ? P.ww : widths[img];
  if (!P.geom && (wh != P.wh || ww != P.ww)) return;        // (a table whose sizes disagree with the crop's)
  const long long rb = dig_abi::round256(3LL * wh * ww);
  unsigned char* A = work + P.ws_off;
  unsigned char* B = A + rb;
  unsigned char* R0 = A + 2 * rb;
  unsigned char* R1 = R0 + 3LL * dig_abi::RS_H * dig_abi::RS_W;
  const unsigned char* src_j = j == 0 ? (P.geom ? A : packed + offsets[img]) : (((j - 1) & 1) ? A : B);
  unsigned char* dst_j = (j & 1) ? A : B;
  const unsigned char* src;
  unsigned char* dst;
  int sh = wh, sw = ww, dh = wh, dw = ww;
  if (kind == 2) { src = src_j; dst = R0; dh = dig_abi::RS_H; dw = dig_abi::RS_W; }
  else if (kind == 3) {
    src = (lvl - 1) & 1 ? R1 : R0; dst = lvl & 1 ? R1 : R0;
    sh = dig_abi::RS_H >> (lvl - 1); sw = dig_abi::RS_W >> (lvl - 1); dh = sh / 2; dw = sw / 2;
  } else if (kind == 4) {
    src = lvl & 1 ? R1 : R0; dst = dst_j; sh = dig_abi::RS_H >> lvl; sw = dig_abi::RS_W >> lvl;
  } else { src = src_j; dst = dst_j; }
  const int npix = dh * dw;
  const int d = run.mb_size;
  for (int p = blockIdx.x * AB_THREADS + threadIdx.x; p < npix; p += gridDim.x * AB_THREADS) {
    const int y = p / dw, x = p - y * dw;
    unsigned char* o = dst + 3 * (size_t)p;
    switch (kind) {
      case 0:
        for (int c = 0; c < 3; ++c) o[c] = dig_abi::noise_byte(P, img, run.noise_var, 3LL * p + c, src[3 * (size_t)p + c]);
        break;
      case 1: dig_abi::blur_pixel(P, d, src, sh, sw, y, x, o); break;
      case 3: dig_abi::pyrdown_pixel(src, sh, sw, y, x, o); break;
      default: dig_abi::resize_cv_pixel(src, sh, sw, dh, dw, P.rs_interp[kind == 2 ? 0 : 1], y, x, o);
    }
  }
}

__global__ __launch_bounds__(AB_THREADS) void abiaug_tail_kernel(const unsigned char* __restrict__ packed, const long long* __restrict__ offsets,
                                                                 const int* __restrict__ heights, const int* __restrict__ widths,
                                                                 const dig_abi_params* __restrict__ params, dig_abi_run run,
                                                                 const unsigned char* __restrict__ work, long long work_bytes,
                                                                 float* __restrict__ out, int out_h, int out_w, int ksh, int ksv, int max_h,
                                                                 int max_w, float mean, float stdv) {
  extern __shared__ int lds[];
  int* kh = lds;                               // [out_w][ksh]
  int* bh = kh + out_w * ksh;                  // [out_w][2]
  int* kv = bh + 2 * out_w;                    // [out_h][ksv]
  int* bv = kv + out_h * ksv;                  // [out_h][2]
  const int ints = out_w * (ksh + 2) + out_h * (ksv + 2);
  unsigned long long* lsum = reinterpret_cast<unsigned long long*>(lds + ints + (ints & 1));
  const int img = blockIdx.x;
  const dig_abi_params& P = params[img];
  const bool crop = P.final_buf == 0;
  if (!crop && !table_ok(P, run, work_bytes)) return;
  if (P.final_buf < 0 || P.final_buf > 2 || (P.final_buf == 2 && !P.det) || (P.final_buf == 1 && !P.geom && !P.det)) return;
  const int h = crop ? heights[img] : P.wh, w = crop ? widths[img] : P.ww;
  if (h > max_h || w > max_w) return;                       // (a bad table: the coefficient tables are sized by max_h / max_w)
  const unsigned char* src = dig_abi::tail_src(P, packed + offsets[img], work);
  for (int t = threadIdx.x; t < out_w + out_h; t += blockDim.x) {
    if (t < out_w) dig_pillow::coeffs_for(t, w, out_w, ksh, kh, bh);
    else dig_pillow::coeffs_for(t - out_w, h, out_h, ksv, kv, bv);
  }
  if (threadIdx.x == 0) *lsum = 0ull;
  __syncthreads();
  const bool jit = P.jit != 0;
  int cm = 0;
  if (jit && dig_abi::has_contrast(P)) {
    unsigned long long s = 0;
    const int npix = h * w;
    for (int p = threadIdx.x; p < npix; p += blockDim.x) {
      int c[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
      dig_abi::jitter_ops(P, 0, true, c);
      s += (unsigned long long)dig_kv::luma(c[0], c[1], c[2]);
    }
    atomicAdd(lsum, s);
    __syncthreads();
    cm = dig_kv::contrast_mean((long long)*lsum, npix);
  }
  const bool pass_h = (w != out_w), pass_v = (h != out_h);
  const int plane = out_h * out_w;
  float* o = out + (size_t)img * 3 * plane;
  for (int p = threadIdx.x; p < plane; p += blockDim.x) {
    const int yy = p / out_w, xx = p - yy * out_w;
    int r[3];
    if (jit) dig_pillow::resize_pixel_f(src, w, pass_h, pass_v, kh, bh, kv, bv, ksh, ksv, yy, xx, r, dig_abi::FetchJitter{&P, cm});
    else dig_pillow::resize_pixel(src, w, pass_h, pass_v, kh, bh, kv, bv, ksh, ksv, yy, xx, r);
    o[p] = ((float)r[0] / 255.0f - mean) / stdv;
    o[plane + p] = ((float)r[1] / 255.0f - mean) / stdv;
    o[2 * plane + p] = ((float)r[2] / 255.0f - mean) / stdv;
  }
}

inline int slices_for(long long npix) { return (int)std::min<long long>(64, std::max<long long>(1, npix / (4 * AB_THREADS))); }

}  // namespace

// C-ABI: see include/dig_hip.h
extern "C" int dig_abiaug_sample(dig_abi_params* params, long long* info, const int* heights, const int* widths, int n_img,
                                 const dig_abi_run* run, unsigned long long seed, unsigned step, hipStream_t stream) {
  if (int rc = dig_rules::abiaug_sample(params, info, heights, widths, n_img, run, seed, step)) return rc;
  hipLaunchKernelGGL(abiaug_sample_kernel, dim3(1), dim3(AB_THREADS), 0, stream, params, info, heights, widths, n_img, *run, seed, step);
  return dig_check_launch();
}

extern "C" long long dig_abiaug_workspace_bytes(int geom, int det, int wh, int ww, const dig_abi_run* run) {
  if (int rc = dig_rules::abiaug_workspace_bytes(geom, det, wh, ww, run)) return rc;
  return dig_abi::image_bytes(geom, det, wh, ww, run->rescale_factor);
}

extern "C" int dig_abiaug_warp_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                                  const dig_abi_params* params, const dig_abi_run* run, unsigned char* work, long long work_bytes, int max_wh,
                                  int max_ww, hipStream_t stream) {
  if (int rc = dig_rules::abiaug_warp_u8(packed, offsets, heights, widths, n_img, params, run, work, work_bytes, max_wh, max_ww)) return rc;
  if (work_bytes == 0) return DIG_OK;                        // (no image has a workspace: no gate of the geometry fired)
  hipLaunchKernelGGL(abiaug_warp_kernel, dim3(slices_for((long long)max_wh * max_ww), n_img), dim3(AB_THREADS), 0, stream, packed, offsets,
                     heights, widths, params, *run, work, work_bytes);
  return dig_check_launch();
}

extern "C" int dig_abiaug_deteriorate_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths,
                                         int n_img, const dig_abi_params* params, const dig_abi_run* run, unsigned char* work,
                                         long long work_bytes, int max_wh, int max_ww, hipStream_t stream) {
  if (int rc = dig_rules::abiaug_deteriorate_u8(packed, offsets, heights, widths, n_img, params, run, work, work_bytes, max_wh, max_ww)) return rc;
  if (work_bytes == 0) return DIG_OK;
  const dig_abi_run R = *run;
  const int s_img = slices_for((long long)max_wh * max_ww), s_rs = slices_for((long long)dig_abi::RS_H * dig_abi::RS_W);
  auto launch = [&](int kind, int j, int lvl, int slices) {
    hipLaunchKernelGGL(abiaug_det_kernel, dim3(slices, n_img), dim3(AB_THREADS), 0, stream, kind, j, lvl, packed, offsets, heights, widths,
                       params, R, work, work_bytes);
    return dig_check_launch();
  };
  for (int j = 0; j < dig_abi::n_det_ops(R); ++j) {
    const int op = dig_abi::det_op(R, j);
    int rc = DIG_OK;
    if (op == 0 || op == 1) rc = launch(op, j, 0, s_img);
    else {
      rc = launch(2, j, 0, s_rs);
      for (int l = 1; l <= R.rescale_factor && !rc; ++l) rc = launch(3, j, l, slices_for(((long long)dig_abi::RS_H * dig_abi::RS_W) >> (2 * l)));
      if (!rc) rc = launch(4, j, R.rescale_factor, s_img);
    }
    if (rc) return rc;
  }
  return DIG_OK;
}

extern "C" int dig_abiaug_tail(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                               const dig_abi_params* params, const dig_abi_run* run, const unsigned char* work, long long work_bytes, float* out,
                               int out_h, int out_w, float mean, float std_, int max_wh, int max_ww, hipStream_t stream) {
  if (int rc = dig_rules::abiaug_tail(packed, offsets, heights, widths, n_img, params, run, work, work_bytes, out, out_h, out_w, mean, std_, max_wh,
                                      max_ww))
    return rc;
  const int ksh = dig_pillow::ksize_for(max_ww, out_w), ksv = dig_pillow::ksize_for(max_wh, out_h);
  const size_t lds = dig_rules::abiaug_tail_lds_bytes(out_h, out_w, ksh, ksv);          // (stage B without the pixel planes)
  static size_t attr = 0;
  if (lds > attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(abiaug_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = lds;
  }
  hipLaunchKernelGGL(abiaug_tail_kernel, dim3(n_img), dim3(AB_THREADS), lds, stream, packed, offsets, heights, widths, params, *run, work,
                     work_bytes, out, out_h, out_w, ksh, ksv, max_wh, max_ww, mean, std_);
  return dig_check_launch();
}
