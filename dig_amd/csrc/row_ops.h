// What one wave does to a row of C logits, written once for the recognition kernels (decode.hip, seq_loss.hip, ctc.hip): lane l reads the
// columns l, l + 64, ... in ascending order, a butterfly folds the 64 lanes, and every lane ends with the row's value.  The attention
// kernels keep their own online softmax: they reduce scores as they form them, not a row that lies in memory.
#pragma once
#include "common.h"

__device__ __forceinline__ float row_max(const float* __restrict__ x, int C, int lane) {
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
  return wave_max(m);
}

// sum_c exp(x[c] - m).  LIBM: expf where the site is defined by it (the CTC greedy score), __expf everywhere else
template <bool LIBM = false>
__device__ __forceinline__ float row_exp_sum(const float* __restrict__ x, int C, int lane, float m) {
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += LIBM ? expf(x[c] - m) : __expf(x[c] - m);
  return wave_sum(s);
}

// (m, s) = (max_c x[c], sum_c exp(x[c] - m)): the caller takes lse = m + log s or the softmax's 1 / s from it
__device__ __forceinline__ void row_max_sum(const float* __restrict__ x, int C, int lane, float& m, float& s) {
  m = row_max(x, C, lane);
  s = row_exp_sum(x, C, lane, m);
}

// The wave's largest (value, index) pair, the lowest index among equal values (torch.max / torch.topk wherever they define the order)
__device__ __forceinline__ void wave_argmax_first(float& m, int& am) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
}

// (m, am) = the row's maximum and its first index (0x7fffffff when no column compares greater than -inf)
__device__ __forceinline__ void row_argmax_first(const float* __restrict__ x, int C, int lane, float& m, int& am) {
  m = -INFINITY;
  am = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = x[c];
    if (v > m) { m = v; am = c; }
  }
  wave_argmax_first(m, am);
}
