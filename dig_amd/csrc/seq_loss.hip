// The sequence cross-entropy criteria of the recognition heads and their gradients (loss/seqCrossEntropyLoss.py,
// loss/seqLabelSmoothingCrossEntropyLoss.py of the reference).  Logit rows [B*T, C] fp32; one wave per row (csrc/row_ops.h), then a
// single block adds the row terms in a fixed order: two launches give the same bits.
//
//   dig_seq_cross_entropy         loss = sum over t < length[b] of -log_softmax(input[b,t])[target[b,t]] / B
//   dig_seq_cross_entropy_bwd     its gradient rows (bf16, pad columns zero)
//   dig_seq_ls_cross_entropy      the label-smoothing form, as the reference computes it
//   dig_seq_ls_cross_entropy_bwd  its gradient rows
// A target outside [0, C) counts as the nearest class.
#include <hip/hip_runtime.h>

#include "row_ops.h"

namespace {

// SeqCrossEntropyLoss.forward (loss/seqCrossEntropyLoss.py:47-63): row (b,t) contributes -log_softmax(input[b,t])[target[b,t]]
// when t < length[b].  One wave per row writes its term; a single block then adds the B*T terms in a fixed order.
__global__ __launch_bounds__(64) void seq_ce_rows_kernel(const float* __restrict__ input, const long long* __restrict__ target,
                                                         const long long* __restrict__ length, int T, int C, float* __restrict__ rowloss) {
  const int row = blockIdx.x, b = row / T, t = row - b * T, lane = threadIdx.x;
  if (t >= length[b]) {
    if (lane == 0) rowloss[row] = 0.f;
    return;
  }
  const float* x = input + (size_t)row * C;
  float m, s;
  row_max_sum(x, C, lane, m, s);
  if (lane == 0) rowloss[row] = -(x[clamp_class(target[row], C)] - m - __logf(s));
}

__global__ __launch_bounds__(256) void fixed_order_sum_kernel(const float* __restrict__ v, int n, float scale, float* __restrict__ out) {
  __shared__ float red[256];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += v[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0] * scale;
}

// dlogits[b,t,:] = g * (softmax(logits[b,t,:]) - onehot(target)) / B for t < length[b], else 0  (gradient of SeqCrossEntropyLoss)
__global__ __launch_bounds__(64) void seq_ce_bwd_kernel(const float* __restrict__ logits, int ld, const long long* __restrict__ target,
                                                        const long long* __restrict__ length, const float* __restrict__ g, int T, int C,
                                                        float inv_B, bf16_t* __restrict__ dlogits, int ldd) {
  const int row = blockIdx.x, b = row / T, t = row - b * T, lane = threadIdx.x;
  bf16_t* out = dlogits + (size_t)row * ldd;
  if (t >= length[b]) {
    for (int c = lane; c < ldd; c += 64) out[c] = 0;
    return;
  }
  const float* x = logits + (size_t)row * ld;
  float m, s;
  row_max_sum(x, C, lane, m, s);
  const float sc = (g ? g[0] : 1.f) * inv_B, inv = 1.f / s;
  const long long y = clamp_class(target[row], C);
  for (int c = lane; c < ldd; c += 64) out[c] = c < C ? f2bf(sc * (__expf(x[c] - m) * inv - (c == y ? 1.f : 0.f))) : (bf16_t)0;
}

// SeqLabelSmoothingCrossEntropyLoss.forward (loss/seqLabelSmoothingCrossEntropyLoss.py:48-70), as the reference computes it: the
// `nll_loss` column [BT,1] and the `smooth_loss` product of a [BT] vector with the [BT,1] mask broadcast to a [BT,BT] matrix, so
//   loss = ( confidence * BT * sum_i mask_i * nll_i  +  smoothing * (sum_i mask_i) * sum_j s_j ) / B,   s_j = -mean_c log_softmax(x_j)_c
// with s_j taken over ALL rows j (also the padded ones).  One wave per row writes (mask_i * nll_i, s_i); a single block then adds
// the terms in a fixed order.
__global__ __launch_bounds__(64) void seq_ls_ce_rows_kernel(const float* __restrict__ input, const long long* __restrict__ target,
                                                            const long long* __restrict__ length, int T, int C, float* __restrict__ rows2) {
  const int row = blockIdx.x, b = row / T, t = row - b * T, lane = threadIdx.x, n = gridDim.x;
  const float* x = input + (size_t)row * C;
  const float m = row_max(x, C, lane);
  float sx = 0.f;
  for (int c = lane; c < C; c += 64) sx += x[c];
  sx = wave_sum(sx);
  const float s = row_exp_sum(x, C, lane, m);
  if (lane == 0) {
    const float lse = m + __logf(s);
    rows2[row] = t < length[b] ? lse - x[clamp_class(target[row], C)] : 0.f;
    rows2[n + row] = lse - sx / (float)C;
  }
}

__global__ __launch_bounds__(256) void seq_ls_ce_sum_kernel(const float* __restrict__ rows2, const long long* __restrict__ length, int B, int T,
                                                            float confidence, float smoothing, float* __restrict__ out) {
  __shared__ float red[3][256];
  const int n = B * T;
  float a = 0.f, b = 0.f, cnt = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) { a += rows2[i]; b += rows2[n + i]; }
  for (int i = threadIdx.x; i < B; i += 256) { const long long l = length[i]; cnt += (float)(l < 0 ? 0 : (l > T ? T : l)); }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = cnt;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (confidence * (float)n * red[0][0] + smoothing * red[2][0] * red[1][0]) / (float)B;
}

// gradient: dL/dx[i,c] = g / B * ( confidence * BT * mask_i * (p_ic - [c == y_i]) + smoothing * M * (p_ic - 1/C) ),  M = sum_i mask_i
__global__ __launch_bounds__(64) void seq_ls_ce_bwd_kernel(const float* __restrict__ logits, int ld, const long long* __restrict__ target,
                                                           const long long* __restrict__ length, const float* __restrict__ g, int B, int T, int C,
                                                           float confidence, float smoothing, bf16_t* __restrict__ dlogits, int ldd) {
  const int row = blockIdx.x, b = row / T, t = row - b * T, lane = threadIdx.x;
  float cnt = 0.f;
  for (int i = lane; i < B; i += 64) { const long long l = length[i]; cnt += (float)(l < 0 ? 0 : (l > T ? T : l)); }
  cnt = wave_sum(cnt);
  const float* x = logits + (size_t)row * ld;
  float m, s;
  row_max_sum(x, C, lane, m, s);
  const float sc = (g ? g[0] : 1.f) / (float)B, inv = 1.f / s;
  const float wn = t < length[b] ? confidence * (float)(B * T) : 0.f, ws = smoothing * cnt;
  const long long y = clamp_class(target[row], C);
  bf16_t* out = dlogits + (size_t)row * ldd;
  for (int c = lane; c < ldd; c += 64) {
    float v = 0.f;
    if (c < C) {
      const float p = __expf(x[c] - m) * inv;
      v = sc * (wn * (p - (c == y ? 1.f : 0.f)) + ws * (p - 1.f / (float)C));
    }
    out[c] = f2bf(v);
  }
}

}  // namespace

// C-ABI: see include/dig_hip.h
extern "C" int dig_seq_cross_entropy(const float* input, const long long* target, const long long* length, int B, int T, int C,
                                     float* row_workspace, float* loss, hipStream_t stream) {
  if (int rc = dig_rules::seq_cross_entropy(input, target, length, B, T, C, row_workspace, loss)) return rc;
  hipLaunchKernelGGL(seq_ce_rows_kernel, dim3(B * T), dim3(64), 0, stream, input, target, length, T, C, row_workspace);
  hipLaunchKernelGGL(fixed_order_sum_kernel, dim3(1), dim3(256), 0, stream, row_workspace, B * T, 1.0f / (float)B, loss);
  return dig_check_launch();
}

extern "C" int dig_seq_cross_entropy_bwd(const float* logits, int ld, const long long* target, const long long* length, const float* gscalar,
                                         int B, int T, int C, void* dlogits, int ldd, hipStream_t stream) {
  if (int rc = dig_rules::seq_cross_entropy_bwd(logits, ld, target, length, gscalar, B, T, C, dlogits, ldd)) return rc;
  hipLaunchKernelGGL(seq_ce_bwd_kernel, dim3(B * T), dim3(64), 0, stream, logits, ld, target, length, gscalar, T, C, 1.0f / (float)B,
                     (bf16_t*)dlogits, ldd);
  return dig_check_launch();
}

extern "C" int dig_seq_ls_cross_entropy(const float* input, const long long* target, const long long* length, int B, int T, int C,
                                        float smoothing, float* row_workspace, float* loss, hipStream_t stream) {
  if (int rc = dig_rules::seq_ls_cross_entropy(input, target, length, B, T, C, smoothing, row_workspace, loss)) return rc;
  hipLaunchKernelGGL(seq_ls_ce_rows_kernel, dim3(B * T), dim3(64), 0, stream, input, target, length, T, C, row_workspace);
  hipLaunchKernelGGL(seq_ls_ce_sum_kernel, dim3(1), dim3(256), 0, stream, row_workspace, length, B, T, 1.f - smoothing, smoothing, loss);
  return dig_check_launch();
}

extern "C" int dig_seq_ls_cross_entropy_bwd(const float* logits, int ld, const long long* target, const long long* length, const float* gscalar,
                                            int B, int T, int C, float smoothing, void* dlogits, int ldd, hipStream_t stream) {
  if (int rc = dig_rules::seq_ls_cross_entropy_bwd(logits, ld, target, length, gscalar, B, T, C, smoothing, dlogits, ldd)) return rc;
  hipLaunchKernelGGL(seq_ls_ce_bwd_kernel, dim3(B * T), dim3(64), 0, stream, logits, ld, target, length, gscalar, B, T, C, 1.f - smoothing,
                     smoothing, (bf16_t*)dlogits, ldd);
  return dig_check_launch();
}
