// The CTC recognition head (`--decoder_type ctc`): the criterion, its gradient and the greedy decode.
//
//   dig_ctc_loss           nll[b] = -log p(labels_b | frames 0..T-1), loss = sum_b nll[b] / B     (the alpha recursion)
//   dig_ctc_loss_bwd       d loss / d logits * gscalar = gscalar / B * (softmax - posterior occupancy of the class)
//   dig_ctc_greedy_decode  the string rule of ctc_get_str_list (evaluation_metric/metrics.py:220-227) as decoder-shaped rows
//
// One wave per sample.  The extended label sequence blank, l_0, blank, l_1, ..., l_{n-1}, blank has 2n + 1 <= 127 states: lane i owns
// state 2i (the blank in front of label i; lane n: the final blank) and state 2i + 1 (label i), so a time step moves ONE value between
// lanes forwards (the label state of lane i - 1) and two backwards (both states of lane i + 1).  The recursions are fp32 in log space, and
// every step is re-centred on its largest state: the removed maxima are summed in double beside the recursion, so the states stay near 0
// whatever T is and log p does not lose digits to its own magnitude (a few hundred at T = 32).  The frame's log-softmax is taken by the
// same wave; emissions, alphas and occupancies live in LDS planes [t][lane], never in a per-lane array.  The per-class occupancy is
// gathered by the lane that owns the class, over the label positions in ascending order: repeated characters need no atomics, and two
// launches give the same bits.
// A sample with no valid alignment (n + adjacent equal labels > T: `zero_infinity`) or with a label outside [0, C) or equal to `blank`
// has nll = 0 and zero gradient rows; no index is ever formed from such a label.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int CTC_MAX_T = 64, CTC_MAX_C = 256, CTC_MAX_LDT = 63;

__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return m;
  return m + logf(expf(a - m) + expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return m;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// What the wave knows of its sample before the recursion: n labels, lane i holds label i (0 where it has none or the label is unusable),
// rep = label i equals label i - 1, ok = the sample has an alignment and every label is a class other than the blank.
struct CtcSample { int n, lab; bool rep, ok; };

__device__ __forceinline__ CtcSample ctc_sample(const long long* __restrict__ target, int ldt, const long long* __restrict__ target_len, int len_offset,
                                                int b, int lane, int T, int C, int blank) {
  CtcSample s;
  long long tl = target_len[b] - (long long)len_offset;
  tl = tl < 0 ? 0 : (tl > ldt ? ldt : tl);
  s.n = (int)tl;                                                         // <= ldt <= 63
  const long long l = lane < s.n ? target[(size_t)b * ldt + lane] : 0;
  const bool bad = lane < s.n && (l < 0 || l >= C || l == blank);
  s.lab = bad ? 0 : (int)l;
  const int prev = __shfl_up(s.lab, 1, 64);
  s.rep = lane > 0 && lane < s.n && s.lab == prev;
  const int nrep = __popcll(__ballot(s.rep));
  s.ok = __ballot(bad) == 0ull && s.n + nrep <= T;
  return s;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Frame log-softmax and the emissions of the sample's states: em[t][lane] = log p_t(label of lane) (-inf for a lane without a label),
// emb[t] = log p_t(blank), and the frame's normaliser as lmax[t] = max_c x_t[c], lsum[t] = log sum_c exp(x_t[c] - lmax[t]).  A
// log-probability near 0 (a confident frame) must not carry the rounding of the logits' own magnitude: the differences x - max are taken
// exactly (in double), the terms are summed in double, and the result is rounded to fp32 once.  The frames are independent: their loads overlap.
__device__ __forceinline__ void ctc_emissions(const float* __restrict__ x, int ld, int T, int C, int blank, const CtcSample& s, int lane,
                                              float* __restrict__ em, float* __restrict__ emb, float* __restrict__ lmax, float* __restrict__ lsum) {
  for (int t = 0; t < T; ++t) {
    const float* row = x + (size_t)t * ld;
    const float xl = row[s.lab], xb = row[blank];
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    double e = 0.0;
    for (int c = lane; c < C; c += 64) e += (double)expf((float)((double)row[c] - (double)m));
    const double ls = log(wave_sum_f64(e));
    em[t * 64 + lane] = lane < s.n ? (float)((double)xl - (double)m - ls) : -INFINITY;
    if (lane == 0) { emb[t] = (float)((double)xb - (double)m - ls); lmax[t] = m; lsum[t] = (float)ls; }
  }
}

// One step of the alpha recursion (t > 0) from the states of frame t - 1.
__device__ __forceinline__ void ctc_alpha_step(float& ab, float& al, float eb, float el, const CtcSample& s, int lane) {
  float pl = __shfl_up(al, 1, 64);                                       // the label state of lane - 1
  if (lane == 0) pl = -INFINITY;
  const float nb = lane <= s.n ? lse2(ab, pl) + eb : -INFINITY;
  const float nl = lane < s.n ? lse3(al, ab, s.rep ? -INFINITY : pl) + el : -INFINITY;
  ab = nb;
  al = nl;
}

// BWD = false: nll[b] only.  BWD = true: the gradient rows of sample b.  Dynamic LDS: T * 64 floats (emissions), and with BWD two more
// planes of the same size (the alphas of the blank and of the label states, the latter overwritten by the label occupancies).
template <bool BWD>
__global__ __launch_bounds__(64) void ctc_kernel(const float* __restrict__ logits, int ld, const long long* __restrict__ target, int ldt,
                                                 const long long* __restrict__ target_len, int len_offset, const float* __restrict__ gscalar,
                                                 int B, int T, int C, int blank, float* __restrict__ nll, void* __restrict__ dlogits, int ldd,
                                                 int d_is_f32) {
  extern __shared__ float dyn[];
  __shared__ float emb[CTC_MAX_T], lmax[CTC_MAX_T], lsum[CTC_MAX_T], bocc[CTC_MAX_T];
  __shared__ double offa[CTC_MAX_T];
  __shared__ int labs[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  float* em = dyn;
  float* pa_b = dyn + (size_t)T * 64;                                     // (BWD only)
  float* pa_l = dyn + (size_t)T * 128;
  const CtcSample s = ctc_sample(target, ldt, target_len, len_offset, b, lane, T, C, blank);
  const float* x = logits + (size_t)b * T * ld;
  float* d32 = (float*)dlogits + (size_t)b * T * ldd;
  bf16_t* d16 = (bf16_t*)dlogits + (size_t)b * T * ldd;
  bool ok = s.ok;                                                         // (wave-uniform)
  double logp = 0.0;
  if (ok) {
    ctc_emissions(x, ld, T, C, blank, s, lane, em, emb, lmax, lsum);
    labs[lane] = s.lab;
    __syncthreads();
    // ---- alpha, re-centred every step; off = the sum of the removed maxima
    float ab = lane == 0 ? emb[0] : -INFINITY;
    float al = (lane == 0 && s.n > 0) ? em[lane] : -INFINITY;
    double off = 0.0;
    for (int t = 0; t < T; ++t) {
      if (t) ctc_alpha_step(ab, al, emb[t], em[t * 64 + lane], s, lane);
      const float m = wave_max(fmaxf(ab, al));                             // finite: the all-blank prefix always has a path
      ab -= m;
      al -= m;
      off += (double)m;
      if (BWD) {
        pa_b[t * 64 + lane] = ab;
        pa_l[t * 64 + lane] = al;
        if (lane == 0) offa[t] = off;
      }
    }
    const float fb = __shfl(ab, s.n, 64);
    const float fl = s.n > 0 ? __shfl(al, s.n - 1, 64) : -INFINITY;
    const float tail = lse2(fb, fl);
    logp = off + (double)tail;
    ok = tail > -INFINITY && logp == logp && logp > -1e300;               // (an alignment whose probability underflowed: as infeasible)
  }
  if (!BWD) {
    if (lane == 0) nll[b] = ok ? (float)(-logp) : 0.f;
    return;
  }
  if (!ok) {
    for (int i = lane; i < T * ldd; i += 64) {
      if (d_is_f32) d32[i] = 0.f; else d16[i] = 0;
    }
    return;
  }
  __syncthreads();
  // ---- beta (emission of frame t included, as in alpha), re-centred the same way; occupancy of a state at frame t =
  // exp(alpha + beta - emission - log p), with the three offsets combined in double
  {
    float bb = -INFINITY, bl = -INFINITY;
    double offb = 0.0;
    const bool rep_next = __shfl_down((int)s.rep, 1, 64) != 0 && lane < 63;
    for (int t = T - 1; t >= 0; --t) {
      const float eb = emb[t], el = em[t * 64 + lane];
      if (t == T - 1) {
        bb = lane == s.n ? eb : -INFINITY;
        bl = (s.n > 0 && lane == s.n - 1) ? el : -INFINITY;
      } else {
        float nb = __shfl_down(bb, 1, 64), nl = __shfl_down(bl, 1, 64);  // both states of lane + 1
        if (lane == 63) { nb = -INFINITY; nl = -INFINITY; }
        const float b2 = lane <= s.n ? lse2(bb, bl) + eb : -INFINITY;
        const float l2 = lane < s.n ? lse3(bl, nb, rep_next ? -INFINITY : nl) + el : -INFINITY;
        bb = b2;
        bl = l2;
      }
      const float m = wave_max(fmaxf(bb, bl));
      bb -= m;
      bl -= m;
      offb += (double)m;
      const double k = offa[t] + offb - logp;                                 // (the sum below is <= 0 and small where it matters: rounded once)
      const float gb = lane <= s.n ? expf((float)((double)pa_b[t * 64 + lane] + (double)bb - (double)eb + k)) : 0.f;
      const float gl = lane < s.n ? expf((float)((double)pa_l[t * 64 + lane] + (double)bl - (double)el + k)) : 0.f;
      const float gbs = wave_sum(gb);
      pa_l[t * 64 + lane] = gl;
      if (lane == 0) bocc[t] = gbs;
    }
  }
  __syncthreads();
  // ---- rows: scale * (softmax - occupancy), pad columns zero.  The lane that owns class c adds the occupancies of the label positions
  // that carry c, in ascending order
  const float sc = (gscalar ? gscalar[0] : 1.f) * (1.0f / (float)B);
  for (int t = 0; t < T; ++t) {
    const float* row = x + (size_t)t * ld;
    const float m = lmax[t], l = lsum[t];
    for (int c = lane; c < ldd; c += 64) {
      float v = 0.f;
      if (c < C) {
        float occ = 0.f;
        if (c == blank) occ = bocc[t];
        else
          for (int i = 0; i < s.n; ++i) occ += labs[i] == c ? pa_l[t * 64 + i] : 0.f;
        v = sc * (expf((row[c] - m) - l) - occ);
      }
      if (d_is_f32) d32[(size_t)t * ldd + c] = v; else d16[(size_t)t * ldd + c] = f2bf(v);
    }
  }
}

// loss = sum_b nll[b] / B: one wave, lane-strided partial sums in double, a fixed butterfly
__global__ __launch_bounds__(64) void ctc_mean_kernel(const float* __restrict__ nll, int B, float* __restrict__ loss) {
  double a = 0.0;
  for (int i = threadIdx.x; i < B; i += 64) a += (double)nll[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (threadIdx.x == 0) loss[0] = (float)(a / (double)B);
}

// One wave per sample: lane t keeps the arg-max class (lowest id on a tie) and its softmax probability of frame t; the emitting frames
// are compacted with one ballot.
__global__ __launch_bounds__(64) void ctc_greedy_kernel(const float* __restrict__ logits, int ld, int T, int C, int blank, int eos, int padding,
                                                        long long* __restrict__ ids, float* __restrict__ score, int* __restrict__ n_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* x = logits + (size_t)b * T * ld;
  int cls = -1;
  float prob = 1.f;
  for (int t = 0; t < T; ++t) {
    const float* row = x + (size_t)t * ld;
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float v = row[c];
      if (v > m) { m = v; am = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    float e = 0.f;
    for (int c = lane; c < C; c += 64) e += expf(row[c] - m);
    e = wave_sum(e);
    if (lane == t) { cls = am; prob = 1.f / e; }
  }
  const int prev = __shfl_up(cls, 1, 64);
  const bool emit = lane < T && cls != blank && cls != eos && !(lane > 0 && prev == cls);
  const unsigned long long mask = __ballot(emit);
  const int pos = __popcll(mask & ((1ull << lane) - 1ull)), n = __popcll(mask);
  long long* idr = ids + (size_t)b * (T + 1);
  float* scr = score + (size_t)b * (T + 1);
  if (emit) { idr[pos] = cls; scr[pos] = prob; }
  for (int j = lane; j <= T; j += 64)
    if (j >= n) { idr[j] = j == n ? eos : padding; scr[j] = 1.f; }
  if (lane == 0) n_out[b] = n;
}

int ctc_check(const void* logits, int ld, const void* target, int ldt, const void* target_len, int B, int T, int C, int blank) {
  if (!logits || !target || !target_len || B < 0 || T <= 0 || C <= 0 || ldt <= 0 || ld < C || blank < 0 || blank >= C) return DIG_ERR_ARG;
  if (T > CTC_MAX_T || C < 2 || C > CTC_MAX_C || ldt > CTC_MAX_LDT) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}

}  // namespace

extern "C" int dig_ctc_loss(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset, int B,
                            int T, int C, int blank, float* nll, float* loss, hipStream_t stream) {
  if (!nll || !loss) return DIG_ERR_ARG;
  const int rc = ctc_check(logits, ld, target, ldt, target_len, B, T, C, blank);
  if (rc != DIG_OK || B == 0) return rc;
  hipLaunchKernelGGL(ctc_kernel<false>, dim3(B), dim3(64), (size_t)T * 64 * sizeof(float), stream, logits, ld, target, ldt, target_len, len_offset,
                     (const float*)nullptr, B, T, C, blank, nll, (void*)nullptr, 0, 0);
  hipLaunchKernelGGL(ctc_mean_kernel, dim3(1), dim3(64), 0, stream, nll, B, loss);
  return dig_check_launch();
}

extern "C" int dig_ctc_loss_bwd(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset,
                                const float* gscalar, int B, int T, int C, int blank, void* dlogits, int ldd, int dlogits_is_f32,
                                hipStream_t stream) {
  if (!dlogits || ldd < C) return DIG_ERR_ARG;
  const int rc = ctc_check(logits, ld, target, ldt, target_len, B, T, C, blank);
  if (rc != DIG_OK || B == 0) return rc;
  hipLaunchKernelGGL(ctc_kernel<true>, dim3(B), dim3(64), (size_t)T * 192 * sizeof(float), stream, logits, ld, target, ldt, target_len, len_offset,
                     gscalar, B, T, C, blank, (float*)nullptr, dlogits, ldd, dlogits_is_f32 ? 1 : 0);
  return dig_check_launch();
}

extern "C" int dig_ctc_greedy_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, long long* ids,
                                     float* score, int* n, hipStream_t stream) {
  if (!logits || !ids || !score || !n || B < 0 || T <= 0 || C <= 0 || ld < C) return DIG_ERR_ARG;
  if (T > CTC_MAX_T || C < 2 || C > CTC_MAX_C) return DIG_ERR_UNSUPPORTED;
  if (B == 0) return DIG_OK;
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(64), 0, stream, logits, ld, T, C, blank, eos, padding, ids, score, n);
  return dig_check_launch();
}
