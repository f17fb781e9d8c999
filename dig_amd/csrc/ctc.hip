// The CTC recognition head (`--decoder_type ctc`): the criterion, its gradient and the greedy decode.
//
//   dig_ctc_loss           nll[b] = -log p(labels_b | frames 0..T-1), loss = sum_b nll[b] / B     (the alpha recursion)
//   dig_ctc_loss_bwd       d loss / d logits * gscalar = gscalar / B * (softmax - posterior occupancy of the class)
//   dig_ctc_greedy_decode  the string rule of ctc_get_str_list (evaluation_metric/metrics.py:220-227) as decoder-shaped rows
//   dig_ctc_beam_decode    prefix beam search (`--ctc_beam_width`): the best collapsed string over all its alignments, as the same rows
//   dig_ctc_lexicon_decode the lexicon word of highest likelihood (`--ctc_lexicon`): one alpha recursion per (sample, word), as the same rows
//   dig_ctc_align          the best alignment of given labels (`--ctc_align_out`): the frames of every character and their log-probability
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

#include "row_ops.h"

namespace {

using dig_rules::CTC_MAX_T;
using dig_rules::CTC_MAX_C;

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
    const float m = row_max(row, C, lane);
    double e = 0.0;
    for (int c = lane; c < C; c += 64) e += (double)expf((float)((double)row[c] - (double)m));
    const double ls = log(wave_sum_f64(e));
    em[t * 64 + lane] = lane < s.n ? (float)((double)xl - (double)m - ls) : -INFINITY;
    if (lane == 0) { emb[t] = (float)((double)xb - (double)m - ls); lmax[t] = m; lsum[t] = (float)ls; }
  }
}

// One step of the alpha recursion (t > 0) from the states of frame t - 1.  SEG: the lanes that hold one sample (64: the whole wave;
// 16 / 32: the lexicon decode packs 4 / 2 short words into a wave), `lane` counted within them.
template <int SEG = 64>
__device__ __forceinline__ void ctc_alpha_step(float& ab, float& al, float eb, float el, const CtcSample& s, int lane) {
  float pl = __shfl_up(al, 1, SEG);                                      // the label state of lane - 1
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

// Forced alignment (the rule: include/dig_hip.h at dig_ctc_align): the max-product twin of the alpha recursion above with back-pointers and
// a back-trace, one wave per sample, lane i owning states 2i and 2i + 1 as in ctc_kernel.  The states are held in double: a step is one
// add and two or three compares per state, there is no sum to keep small and so nothing to re-centre, and the score of the path is the
// double sum of its fp32 emissions rounded once.  A step moves one value up a lane (the label state of lane - 1), as ctc_alpha_step does.
// Dynamic LDS: the T x 64 float emission plane, then T x 64 bytes of back-pointers: byte [t][lane] holds the choice of the lane's blank
// state in bits 0-1 (0 stay, 1 step) and of its label state in bits 2-3 (0 stay, 1 step, 2 skip), which is also the number of states the
// back-trace moves down.  The back-trace is wave-uniform (every lane reads the same byte: a broadcast) and leaves the frame's state in
// path[t]; lane k then walks the row for the span of label k and sums its emissions in ascending t.
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ logits, int ld, const long long* __restrict__ target, int ldt,
                                                       const long long* __restrict__ target_len, int len_offset, int T, int C, int blank,
                                                       int* __restrict__ start, int* __restrict__ end, float* __restrict__ char_logp,
                                                       float* __restrict__ path_logp, int* __restrict__ frame_label) {
  extern __shared__ float dyn[];
  __shared__ float emb[CTC_MAX_T], lmax[CTC_MAX_T], lsum[CTC_MAX_T];
  __shared__ int path[CTC_MAX_T];
  const int b = blockIdx.x, lane = threadIdx.x;
  float* em = dyn;
  unsigned char* bp = (unsigned char*)(dyn + (size_t)T * 64);
  const CtcSample s = ctc_sample(target, ldt, target_len, len_offset, b, lane, T, C, blank);
  int* st = start + (size_t)b * ldt;
  int* en = end + (size_t)b * ldt;
  float* cl = char_logp + (size_t)b * ldt;
  bool ok = s.ok;                                                         // (wave-uniform)
  double best = -INFINITY;
  int state = 0;
  if (ok) {
    ctc_emissions(logits + (size_t)b * T * ld, ld, T, C, blank, s, lane, em, emb, lmax, lsum);
    __syncthreads();
    double vb = lane == 0 ? (double)emb[0] : -INFINITY;
    double vl = (lane == 0 && s.n > 0) ? (double)em[lane] : -INFINITY;
    for (int t = 1; t < T; ++t) {
      double pl = __shfl_up(vl, 1, 64);                                    // the label state of lane - 1
      if (lane == 0) pl = -INFINITY;
      // the predecessors in the order stay, step, skip: a later one wins only when strictly larger
      const bool b_step = pl > vb;
      const double mb = b_step ? pl : vb;
      const bool l_step = vb > vl;
      double ml = l_step ? vb : vl;
      const bool l_skip = !s.rep && pl > ml;
      ml = l_skip ? pl : ml;
      bp[t * 64 + lane] = (unsigned char)((b_step ? 1 : 0) | ((l_skip ? 2 : (l_step ? 1 : 0)) << 2));
      vb = lane <= s.n ? mb + (double)emb[t] : -INFINITY;
      vl = lane < s.n ? ml + (double)em[t * 64 + lane] : -INFINITY;
    }
    const double fb = __shfl(vb, s.n, 64);
    const double fl = s.n > 0 ? __shfl(vl, s.n - 1, 64) : -INFINITY;
    state = fl > fb ? 2 * s.n - 1 : 2 * s.n;
    best = fl > fb ? fl : fb;
    ok = best > -INFINITY;                                                // (a path of probability 0, which finite logits never give: as no alignment)
  }
  if (!ok) {
    if (lane < ldt) { st[lane] = -1; en[lane] = -1; cl[lane] = 0.f; }
    if (lane == 0) path_logp[b] = -INFINITY;
    if (frame_label && lane < T) frame_label[(size_t)b * T + lane] = -2;
    return;
  }
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    if (lane == 0) path[t] = state;
    if (t) {
      const int c = bp[t * 64 + (state >> 1)];
      state = max(state - ((state & 1) ? (c >> 2) & 3 : c & 3), 0);        // (never below 0: lane 0 has no step into its blank and no skip)
    }
  }
  __syncthreads();
  if (lane < ldt) {
    int t0 = -1, t1 = -1;
    double sum = 0.0;
    if (lane < s.n)
      for (int t = 0; t < T; ++t)
        if (path[t] == 2 * lane + 1) {
          if (t0 < 0) t0 = t;
          t1 = t + 1;
          sum += (double)em[t * 64 + lane];
        }
    st[lane] = t0;
    en[lane] = t1;
    cl[lane] = (float)sum;
  }
  if (lane == 0) path_logp[b] = (float)best;
  if (frame_label && lane < T) {
    const int p = path[lane];
    frame_label[(size_t)b * T + lane] = (p & 1) ? p >> 1 : -1;
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
    float m;
    int am;
    row_argmax_first(row, C, lane, m, am);
    const float e = row_exp_sum<true>(row, C, lane, m);                     // (expf, not __expf: the score is defined by it)
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

// CTC prefix beam search (the rule: include/dig_hip.h), one wave per sample.  Lane j owns the hypothesis of rank j: lb, ln, the length and
// the last symbol of its prefix in registers, the prefix bytes in an LDS row (two sets of rows: a frame reads one and writes the other).  A
// frame fills the candidate table cs (dynamic LDS, W rows of CP = C rounded up to 64 floats) with every candidate's tot, laid out in the
// order in which the rule touches the prefixes: row i = hypothesis i, column 0 = "i stays", then "i extended by c" for the classes other
// than the blank in ascending order; the columns past C hold NaN, which no comparison selects.  An extension that lands on a live prefix is
// found by the lane of that prefix, which compares lengths, then the last symbols, then the bytes: the two are one candidate, kept in
// whichever of the two cells comes first (where the prefix was first touched), the other cell struck out with NaN.  The W best are taken one
// per round by a maximum of (tot, lowest cell index): lane l owns the cells 4 l .. 4 l + 3 of every block of 256 and keeps its best, a DPP
// reduction and a ballot pick among the lanes, and the wave together finds the winning lane's next best.  A candidate at -inf (probability
// 0) is never taken: neither it nor a descendant can become the result.  After the selection every state is re-centred on the best tot,
// whose sum is kept in double, as the alpha recursion above does.  The next frame's logits are loaded before the search of the current
// one.  LDS at W = 32, C = 256: 32 KB table + 1 KB log-softmax + 4.3 KB prefixes.
constexpr int CTC_MAX_W = dig_rules::CTC_MAX_W, CTC_PFX_WORDS = 17;                          // 64 prefix bytes and a pad word: row j starts on bank 17 j

// The value of lane l (wave-uniform l) as a scalar: v_readlane, where __shfl would go through the LDS crossbar.
__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The wave's maximum as a scalar, through the DPP network (row shifts 1, 2, 4, 8 leave a row's maximum in its lane 15; the two row
// broadcasts carry it on: lane 63 ends with the maximum of all 64) where a __shfl_xor butterfly would make six trips through the LDS crossbar.
__device__ __forceinline__ float wave_max_dpp(float v) {
  const int ninf = __float_as_int(-INFINITY);
#define CTC_DPP_MAX(ctrl, rows) v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), ctrl, rows, 0xf, false)))
  CTC_DPP_MAX(0x111, 0xf);                                                 // row_shr:1
  CTC_DPP_MAX(0x112, 0xf);                                                 // row_shr:2
  CTC_DPP_MAX(0x114, 0xf);                                                 // row_shr:4
  CTC_DPP_MAX(0x118, 0xf);                                                 // row_shr:8
  CTC_DPP_MAX(0x142, 0xa);                                                 // row_bcast:15 into rows 1 and 3
  CTC_DPP_MAX(0x143, 0xc);                                                 // row_bcast:31 into rows 2 and 3
#undef CTC_DPP_MAX
  return lane_f(v, 63);
}

__device__ __forceinline__ void ctc_load_row(const float* __restrict__ row, int C, int lane, float (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = lane + 64 * k < C ? row[lane + 64 * k] : -INFINITY;
}

__global__ __launch_bounds__(64) void ctc_beam_kernel(const float* __restrict__ logits, int ld, int T, int C, int blank, int eos, int padding, int W,
                                                      long long* __restrict__ ids, float* __restrict__ score, float* __restrict__ logp_out,
                                                      int* __restrict__ n_out) {
  extern __shared__ float4 beam_dyn[];                                     // (float4: the table is read 16 bytes at a time)
  __shared__ float lpv[CTC_MAX_C], selv[CTC_MAX_W];
  __shared__ unsigned pfx[2][CTC_MAX_W * CTC_PFX_WORDS];
  __shared__ int sel[CTC_MAX_W], srow[CTC_MAX_W];
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* x = logits + (size_t)b * T * ld;
  float* cs = (float*)beam_dyn;
  const int CJ = (C + 63) >> 6, CP = CJ * 64;
  for (int i = lane; i < ((W * CP + 255) & ~255); i += 64) cs[i] = NAN;
  float lb = lane == 0 ? 0.f : -INFINITY, ln = -INFINITY;
  int len = 0, last = -1, nl = 1, cur = 0;                                 // last = -1: the empty prefix (equal to no class)
  double off = 0.0;
  float xn[4];
  ctc_load_row(x, C, lane, xn);
  for (int t = 0; t < T; ++t) {
    float xr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xr[k] = xn[k];
    if (t + 1 < T) ctc_load_row(x + (size_t)(t + 1) * ld, C, lane, xn);
    // ---- the frame's log-softmax, as ctc_emissions takes it
    const float m = wave_max_dpp(fmaxf(fmaxf(xr[0], xr[1]), fmaxf(xr[2], xr[3])));
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (lane + 64 * k < C) e += (double)expf((float)((double)xr[k] - (double)m));
    const double ls = log(wave_sum_f64(e));
    float lpr[4];                                                           // lp of the classes lane, lane + 64, ...: kept for the extensions
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lpr[k] = (float)((double)xr[k] - (double)m - ls);
      if (lane + 64 * k < C) lpv[lane + 64 * k] = lpr[k];
    }
    // ---- par = the live hypothesis whose prefix is this lane's without its last symbol (at most one), or -1
    const unsigned* P = pfx[cur];
    int par = -1;
    for (int i = 0; i < nl; ++i) {
      const int li = lane_i(len, i), lasti = lane_i(last, i);
      if (lane < nl && par < 0 && len == li + 1) {
        const unsigned* a = P + i * CTC_PFX_WORDS;
        const unsigned* q = P + lane * CTC_PFX_WORDS;
        bool same = li == 0 || lasti == (int)((q[(li - 1) >> 2] >> (8 * ((li - 1) & 3))) & 255u);
        const int fw = li >> 2, rem = li & 3;
        for (int k = 0; k < fw && same; ++k) same = a[k] == q[k];
        if (same && rem) same = ((a[fw] ^ q[fw]) & ((1u << (8 * rem)) - 1u)) == 0u;
        if (same) par = i;
      }
    }
    __syncthreads();
    // ---- extensions: cell (i, 1 + c or c, the blank's column skipped) = (lb_i when c repeats the prefix's last symbol, else tot_i) + lp[c]
    const float tot = lse2(lb, ln);
    for (int i = 0; i < nl; ++i) {
      const float ti = lane_f(tot, i), lbi = lane_f(lb, i);
      const int lasti = lane_i(last, i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < C && c != blank) cs[i * CP + c + (c < blank ? 1 : 0)] = (c == lasti ? lbi : ti) + lpr[k];
      }
    }
    __syncthreads();
    // ---- stay, with the parent's extension merged in: one candidate in the earlier of the two cells (mc), the later one struck out
    const int sp = par < 0 ? 0 : par;
    const float plb = __shfl(lb, sp, 64), ptot = __shfl(tot, sp, 64);
    const int plast = __shfl(last, sp, 64);
    float nlb = -INFINITY, nln = -INFINITY;
    int mc = -1;
    if (lane < nl) {
      nlb = tot + lpv[blank];
      if (len > 0) nln = ln + lpv[last];
      mc = lane * CP;
      if (par >= 0) {
        nln = lse2(nln, (plast == last ? plb : ptot) + lpv[last]);
        const int xc = par * CP + last + (last < blank ? 1 : 0);
        cs[max(mc, xc)] = NAN;
        mc = min(mc, xc);
      }
      cs[mc] = lse2(nlb, nln);
    }
    __syncthreads();
    // ---- the W best by (tot, cell index), one per round.  Lane l scans its own cells (4 l .. 4 l + 3 of every block of 256) once and keeps
    // its best; a round picks among the lanes, strikes the winner's cell, and all 64 lanes together look through the winner's cells (one or
    // two each) for its next best.  A round that finds nothing ends the selection (fewer than W candidates)
    const int nq = (nl * CP + 255) >> 8;                                    // blocks; rows past nl in the last one hold NaN
    float bv = -INFINITY;
    int bi = -1;
    {
      const float4* cs4 = (const float4*)cs + lane;
      int be = -1;
      for (int q = 0; q < nq; q += 2) {
        const float4 a = cs4[q * 64];
        const float4 c4 = q + 1 < nq ? cs4[(q + 1) * 64] : make_float4(NAN, NAN, NAN, NAN);
        const float v[8] = {a.x, a.y, a.z, a.w, c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int u = 0; u < 8; ++u) {                                        // (strict: the first of equal values)
          const bool take = v[u] > bv;
          bv = take ? v[u] : bv;
          be = take ? q * 4 + u : be;
        }
      }
      if (be >= 0) bi = (be >> 2) * 256 + lane * 4 + (be & 3);
    }
    int nn = 0;
    for (int r = 0; r < W; ++r) {
      const float gv = wave_max_dpp(bv);
      unsigned long long tie = __ballot(bi >= 0 && bv == gv);              // the lanes holding the largest tot: nearly always one
      if (tie == 0ull) break;                                               // (wave-uniform)
      int gi = 0x7fffffff;
      for (; tie; tie &= tie - 1ull) gi = min(gi, lane_i(bi, __ffsll((long long)tie) - 1));
      const int wl = (gi & 255) >> 2;                                       // the winner's lane
      if (lane == wl) { cs[gi] = NAN; sel[r] = gi; selv[r] = gv; }
      nn = r + 1;
      __syncthreads();
      // the winner's remaining cells in ascending order: k = 4 q + sub, lane l reads k = l and k = 64 + l
      const int k0 = lane, k1 = 64 + lane;
      const float v0 = (k0 >> 2) < nq ? cs[(k0 >> 2) * 256 + wl * 4 + (k0 & 3)] : NAN;
      const float v1 = (k1 >> 2) < nq ? cs[(k1 >> 2) * 256 + wl * 4 + (k1 & 3)] : NAN;
      const float nv = wave_max_dpp(fmaxf(fmaxf(v0, v1), -INFINITY));       // (fmaxf drops a NaN operand)
      int nk = -1;
      if (nv > -INFINITY) {
        const unsigned long long t0 = __ballot(v0 == nv);
        nk = t0 ? __ffsll((long long)t0) - 1 : 64 + __ffsll((long long)__ballot(v1 == nv)) - 1;
      }
      if (lane == wl) {
        bv = nv;
        bi = nk < 0 ? -1 : (nk >> 2) * 256 + wl * 4 + (nk & 3);
      }
    }
    // ---- the next frame's hypotheses: lane r takes the candidate of cell sel[r], which is "src stays" when it is the cell of a live
    // prefix and an extension otherwise; prefixes are copied row to row, then the new symbol is appended
    const int s = lane < nn ? sel[lane] : -2;
    int src = -1;
    for (int i = 0; i < nl; ++i)
      if (lane_i(mc, i) == s) src = i;
    const bool live = lane < nn, stay = src >= 0;
    const int row = live ? s / CP : 0, col = live ? s - row * CP : 0;
    const int pi = stay ? src : row, c = col - (col <= blank ? 1 : 0);       // (c: read for an extension only, col >= 1)
    const float v = live ? selv[lane] : -INFINITY;
    const float snlb = __shfl(nlb, pi, 64), snln = __shfl(nln, pi, 64);
    const int slen = __shfl(len, pi, 64), slast = __shfl(last, pi, 64);
    if (live) srow[lane] = pi;
    __syncthreads();
    unsigned* Q = pfx[cur ^ 1];
    for (int idx = lane; idx < nn * 16; idx += 64) Q[(idx >> 4) * CTC_PFX_WORDS + (idx & 15)] = P[srow[idx >> 4] * CTC_PFX_WORDS + (idx & 15)];
    __syncthreads();
    if (live && !stay) ((unsigned char*)(Q + lane * CTC_PFX_WORDS))[slen] = (unsigned char)c;   // slen <= t <= 63
    lb = live && stay ? snlb : -INFINITY;
    ln = live ? (stay ? snln : v) : -INFINITY;
    len = live ? slen + (stay ? 0 : 1) : 0;
    last = live ? (stay ? slast : c) : -1;
    const float m0 = lane_f(lse2(lb, ln), 0);                                // rank 0: the largest tot
    if (m0 > -INFINITY && m0 < INFINITY) { lb -= m0; ln -= m0; off += (double)m0; }
    nn = __builtin_amdgcn_readfirstlane(nn);
    if (nn < nl)                                                            // (a shrinking beam: its abandoned rows must not be scanned again)
      for (int i = nn * CP + lane; i < nl * CP; i += 64) cs[i] = NAN;
    nl = nn;
    cur ^= 1;
    __syncthreads();
  }
  // ---- the row of rank 0 without EOS, compacted with one ballot
  const unsigned char* best = (const unsigned char*)pfx[cur];
  const int n0 = lane_i(len, 0);
  const float lp0 = (float)(off + (double)lane_f(lse2(lb, ln), 0));
  const int sym = lane < n0 ? (int)best[lane] : -1;
  const bool emit = lane < n0 && sym != eos;
  const unsigned long long mask = __ballot(emit);
  const int pos = __popcll(mask & ((1ull << lane) - 1ull)), n = __popcll(mask);
  long long* idr = ids + (size_t)b * (T + 1);
  float* scr = score + (size_t)b * (T + 1);
  if (emit) idr[pos] = sym;
  for (int j = lane; j <= T; j += 64) {
    if (j >= n) idr[j] = j == n ? eos : padding;
    scr[j] = j == 0 ? (float)exp((double)lp0) : 1.f;                        // (expf loses |logp| * 2^-24 of relative accuracy)
  }
  if (lane == 0) { n_out[b] = n; logp_out[b] = lp0; }
}

// ---- lexicon decode (the rule: include/dig_hip.h at dig_ctc_lexicon_decode): s(b, w) = log p(labels_w | frames of b) for every word of the
// sample's range, and the best (s, lowest pool index) pair.  Three launches.  (1) ctc_lex_softmax_kernel: the log-softmax of every frame,
// once per sample, as ctc_emissions takes it (differences and sum in double, rounded to fp32 once), into the workspace as [B][T][C].
// (2) ctc_lex_score_kernel: workgroup (chunk, sample) of 4 waves copies the sample's table into LDS (dynamic, T * C floats) and walks the
// CTC_LEX_CHUNK words of its chunk.  Lexicon words are short, so a wave carries 64 / SEG of them at once: the chunk's longest word picks
// SEG = 16 (up to 15 labels), 32 (up to 31) or 64, each word on SEG consecutive lanes with the state layout of ctc_kernel (lane i of the
// segment: the blank in front of label i and label i; lane n: the final blank), the same ctc_alpha_step, the same re-centring and the
// same double offset, so a score has the bits of ctc_kernel<false>'s -nll.  A word's emissions are gathered from the LDS table by the
// lane's label.  The chunk's best pair is kept as one 64-bit key (the score's bits made monotonic, then the complement of the pool index:
// the larger key is the larger score, and among equal scores the lower index) and left in the workspace; keys are distinct, so their
// maximum does not depend on the cut.  (3) ctc_lex_fold_kernel: one wave per sample takes the largest key and writes the outputs.
// (One word per wave for every chunk was measured at 2.5 to 4 times the time: profiles/README.md.)
constexpr int CTC_LEX_CHUNK = DIG_CTC_LEX_CHUNK, CTC_LEX_WAVES = 4;
constexpr unsigned long long CTC_LEX_NONE = 0ull;                          // (below the key of any score above -inf)

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned long long ctc_lex_key(float s, int w) {
  if (!(s > -INFINITY)) return CTC_LEX_NONE;
  if (s == 0.f) s = 0.f;                                                   // (-0 and +0 are one score)
  const unsigned u = __float_as_uint(s);
  const unsigned mono = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)mono << 32) | (unsigned)~(unsigned)w;
}
__device__ __forceinline__ float ctc_lex_key_score(unsigned long long key) {
  const unsigned mono = (unsigned)(key >> 32);
  return __uint_as_float((mono & 0x80000000u) ? (mono & 0x7fffffffu) : ~mono);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(64) void ctc_lex_softmax_kernel(const float* __restrict__ logits, int ld, int C, float* __restrict__ lp) {
  const int lane = threadIdx.x;
  const float* row = logits + (size_t)blockIdx.x * ld;                     // frame (b, t) = blockIdx.x
  float* out = lp + (size_t)blockIdx.x * C;
  const float m = row_max(row, C, lane);
  double e = 0.0;
  for (int c = lane; c < C; c += 64) e += (double)expf((float)((double)row[c] - (double)m));
  const double ls = log(wave_sum_f64(e));
  for (int c = lane; c < C; c += 64) out[c] = (float)((double)row[c] - (double)m - ls);
}

// The words k0 + slot, k0 + slot + 256 / SEG, ... of the chunk (slot = the thread's segment within the workgroup): returns the best key
// of the thread's segment on its lane 0, CTC_LEX_NONE on the other lanes.
template <int SEG>
__device__ __forceinline__ unsigned long long ctc_lex_words(const float* __restrict__ tab, int T, int C, int blank, const int* __restrict__ words,
                                                            const int* __restrict__ word_len, int ldw, int w0, int nw, float* __restrict__ srow) {
  constexpr int PER = CTC_LEX_WAVES * 64 / SEG;                            // words in flight per workgroup
  const int lane = threadIdx.x & 63, li = lane & (SEG - 1), sbase = lane & ~(SEG - 1), slot = (int)threadIdx.x / SEG;
  const unsigned long long smask = SEG == 64 ? ~0ull : ((1ull << SEG) - 1ull);
  unsigned long long best = CTC_LEX_NONE;
  for (int k0 = 0; k0 < nw; k0 += PER) {
    if (k0 + (int)(threadIdx.x >> 6) * (64 / SEG) >= nw) break;            // (wave-uniform: none of the wave's segments has a word)
    const int k = k0 + slot;
    const bool have = k < nw;
    const int w = w0 + (have ? k : 0);
    CtcSample s;
    s.n = have ? clamp_i(word_len[w], 0, min(ldw, SEG - 1)) : 0;
    const int l = li < s.n ? words[(size_t)w * ldw + li] : 0;
    const bool bad = li < s.n && (l < 0 || l >= C || l == blank);
    s.lab = bad ? 0 : l;
    const int prev = __shfl_up(s.lab, 1, SEG);
    s.rep = li > 0 && li < s.n && s.lab == prev;
    const int nrep = __popcll((__ballot(s.rep) >> sbase) & smask);
    s.ok = ((__ballot(bad) >> sbase) & smask) == 0ull && s.n + nrep <= T;
    float ab = li == 0 ? tab[blank] : -INFINITY;
    float al = (li == 0 && s.n > 0) ? tab[s.lab] : -INFINITY;
    double off = 0.0;
    for (int t = 0; t < T; ++t) {
      const float* row = tab + t * C;
      if (t) ctc_alpha_step<SEG>(ab, al, row[blank], li < s.n ? row[s.lab] : -INFINITY, s, li);
      float m = fmaxf(ab, al);
#pragma unroll
      for (int o = SEG / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));   // the segment's maximum: finite (the all-blank prefix)
      ab -= m;
      al -= m;
      off += (double)m;
    }
    const float fb = __shfl(ab, s.n, SEG);
    const float fl = s.n > 0 ? __shfl(al, s.n - 1, SEG) : -INFINITY;
    const float tail = lse2(fb, fl);
    const double logp = off + (double)tail;
    const bool ok = s.ok && tail > -INFINITY && logp == logp && logp > -1e300;
    const float sc = ok ? (float)logp : -INFINITY;
    if (have && li == 0) {
      if (srow) srow[k] = sc;
      const unsigned long long key = ctc_lex_key(sc, w);
      best = key > best ? key : best;
    }
  }
  return best;
}

__global__ __launch_bounds__(CTC_LEX_WAVES * 64) void ctc_lex_score_kernel(const float* __restrict__ lp, int T, int C, int blank,
                                                                          const int* __restrict__ words, const int* __restrict__ word_len, int ldw,
                                                                          int W, const int* __restrict__ lex_begin, const int* __restrict__ lex_count,
                                                                          int max_count, int n_chunks, unsigned long long* __restrict__ partial,
                                                                          float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) float lex_tab[];          // [T][C]; filled 16 bytes at a time where the source allows
  __shared__ unsigned long long wbest[CTC_LEX_WAVES];
  const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
  const int begin = clamp_i(lex_begin[b], 0, W);
  const int count = clamp_i(lex_count[b], 0, min(W - begin, max_count));
  const int c0 = chunk * CTC_LEX_CHUNK;                                    // (n_chunks * CHUNK < 2^31 + CHUNK: the launcher sees to it)
  const int nw = min(count - c0, CTC_LEX_CHUNK);                           // the chunk's words; <= 0: past the range
  float* srow = scores ? scores + (size_t)b * max_count + c0 : nullptr;
  if (srow)
    for (int j = tid; j < CTC_LEX_CHUNK; j += CTC_LEX_WAVES * 64)
      if (j >= nw && j < max_count - c0) srow[j] = -INFINITY;
  if (nw <= 0) {                                                           // (workgroup-uniform)
    if (tid == 0) partial[(size_t)b * n_chunks + chunk] = CTC_LEX_NONE;
    return;
  }
  const int w0 = begin + c0;
  int len = 0;
  for (int j = tid; j < nw; j += CTC_LEX_WAVES * 64) len = max(len, clamp_i(word_len[w0 + j], 0, ldw));
  const int over31 = __syncthreads_or(len > 31), over15 = __syncthreads_or(len > 15);
  {
    const float* src = lp + (size_t)b * T * C;
    const int n = T * C;
    if ((n & 3) == 0 && (((uintptr_t)src) & 15u) == 0) {
      for (int i = tid; i < (n >> 2); i += CTC_LEX_WAVES * 64) ((float4*)lex_tab)[i] = ((const float4*)src)[i];
    } else {
      for (int i = tid; i < n; i += CTC_LEX_WAVES * 64) lex_tab[i] = src[i];
    }
  }
  __syncthreads();
  unsigned long long best;
  if (over31) best = ctc_lex_words<64>(lex_tab, T, C, blank, words, word_len, ldw, w0, nw, srow);
  else if (over15) best = ctc_lex_words<32>(lex_tab, T, C, blank, words, word_len, ldw, w0, nw, srow);
  else best = ctc_lex_words<16>(lex_tab, T, C, blank, words, word_len, ldw, w0, nw, srow);
  best = wave_max_u64(best);
  if ((tid & 63) == 0) wbest[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < CTC_LEX_WAVES; ++i) best = wbest[i] > best ? wbest[i] : best;
    partial[(size_t)b * n_chunks + chunk] = best;
  }
}

// One wave per sample: the largest key of its chunks, then the decoder-shaped row of the chosen word (the empty row when there is none).
__global__ __launch_bounds__(64) void ctc_lex_fold_kernel(const unsigned long long* __restrict__ partial, int n_chunks, const int* __restrict__ words,
                                                          const int* __restrict__ word_len, int ldw, int T, int eos, int padding,
                                                          int* __restrict__ best_index, float* __restrict__ logp, long long* __restrict__ ids,
                                                          float* __restrict__ score, int* __restrict__ n_out) {
  const int lane = threadIdx.x, b = blockIdx.x;
  unsigned long long key = CTC_LEX_NONE;
  for (int c = lane; c < n_chunks; c += 64) {
    const unsigned long long o = partial[(size_t)b * n_chunks + c];
    key = o > key ? o : key;
  }
  key = wave_max_u64(key);
  const bool none = key == CTC_LEX_NONE;
  const int w = none ? -1 : (int)~(unsigned)key;
  const float lpb = none ? -INFINITY : ctc_lex_key_score(key);
  const int n = none ? 0 : clamp_i(word_len[w], 0, min(ldw, T));           // (a scored word has n + repeats <= T)
  long long* idr = ids + (size_t)b * (T + 1);
  float* scr = score + (size_t)b * (T + 1);
  for (int j = lane; j <= T; j += 64) {
    idr[j] = j < n ? (long long)words[(size_t)w * ldw + j] : (j == n ? eos : padding);
    scr[j] = j == 0 ? (none ? 0.f : (float)exp((double)lpb)) : 1.f;
  }
  if (lane == 0) { best_index[b] = w; logp[b] = lpb; n_out[b] = n; }
}

}  // namespace

extern "C" int dig_ctc_loss(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset, int B,
                            int T, int C, int blank, float* nll, float* loss, hipStream_t stream) {
  if (int rc = dig_rules::ctc_loss(logits, ld, target, ldt, target_len, len_offset, B, T, C, blank, nll, loss)) return rc;
  if (B == 0) return DIG_OK;
  hipLaunchKernelGGL(ctc_kernel<false>, dim3(B), dim3(64), (size_t)T * 64 * sizeof(float), stream, logits, ld, target, ldt, target_len, len_offset,
                     (const float*)nullptr, B, T, C, blank, nll, (void*)nullptr, 0, 0);
  hipLaunchKernelGGL(ctc_mean_kernel, dim3(1), dim3(64), 0, stream, nll, B, loss);
  return dig_check_launch();
}

extern "C" int dig_ctc_loss_bwd(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset,
                                const float* gscalar, int B, int T, int C, int blank, void* dlogits, int ldd, int dlogits_is_f32,
                                hipStream_t stream) {
  if (int rc = dig_rules::ctc_loss_bwd(logits, ld, target, ldt, target_len, len_offset, gscalar, B, T, C, blank, dlogits, ldd, dlogits_is_f32))
    return rc;
  if (B == 0) return DIG_OK;
  hipLaunchKernelGGL(ctc_kernel<true>, dim3(B), dim3(64), (size_t)T * 192 * sizeof(float), stream, logits, ld, target, ldt, target_len, len_offset,
                     gscalar, B, T, C, blank, (float*)nullptr, dlogits, ldd, dlogits_is_f32 ? 1 : 0);
  return dig_check_launch();
}

extern "C" int dig_ctc_align(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset, int B,
                             int T, int C, int blank, int* start, int* end, float* char_logp, float* path_logp, int* frame_label,
                             hipStream_t stream) {
  if (int rc = dig_rules::ctc_align(logits, ld, target, ldt, target_len, len_offset, B, T, C, blank, start, end, char_logp, path_logp, frame_label))
    return rc;
  if (B == 0) return DIG_OK;
  hipLaunchKernelGGL(ctc_align_kernel, dim3(B), dim3(64), (size_t)T * 64 * (sizeof(float) + 1), stream, logits, ld, target, ldt, target_len,
                     len_offset, T, C, blank, start, end, char_logp, path_logp, frame_label);
  return dig_check_launch();
}

extern "C" int dig_ctc_greedy_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, long long* ids,
                                     float* score, int* n, hipStream_t stream) {
  if (int rc = dig_rules::ctc_greedy_decode(logits, ld, B, T, C, blank, eos, padding, ids, score, n)) return rc;
  if (B == 0) return DIG_OK;
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(64), 0, stream, logits, ld, T, C, blank, eos, padding, ids, score, n);
  return dig_check_launch();
}

extern "C" int dig_ctc_beam_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, int beam_width,
                                   long long* ids, float* score, float* logp, int* n, hipStream_t stream) {
  if (int rc = dig_rules::ctc_beam_decode(logits, ld, B, T, C, blank, eos, padding, beam_width, ids, score, logp, n)) return rc;
  if (B == 0) return DIG_OK;
  hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(64), (size_t)((beam_width * ((C + 63) / 64 * 64) + 255) & ~255) * sizeof(float), stream, logits, ld, T, C, blank, eos, padding,
                     beam_width, ids, score, logp, n);
  return dig_check_launch();
}

extern "C" int dig_ctc_lexicon_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, const int* words,
                                      const int* word_len, int ldw, int W, const int* lex_begin, const int* lex_count, int max_count,
                                      int* best_index, float* logp, long long* ids, float* score, int* n, float* scores, void* workspace,
                                      long long workspace_bytes, hipStream_t stream) {
  if (int rc = dig_rules::ctc_lexicon_decode(logits, ld, B, T, C, blank, eos, padding, words, word_len, ldw, W, lex_begin, lex_count, max_count,
                                             best_index, logp, ids, score, n, scores, workspace, workspace_bytes))
    return rc;
  if (B == 0) return DIG_OK;
  const int n_chunks = (int)dig_rules::ctc_lex_chunks(max_count);                     // 0 with max_count == 0: nothing to score
  unsigned long long* partial = (unsigned long long*)workspace;
  float* lp = (float*)(partial + (size_t)B * std::max(1, n_chunks));
  if (n_chunks > 0) {
    const size_t lds = (size_t)T * C * sizeof(float);                      // 12.5 KB at the recipe shape, 64 KB at the limits
    static bool attr_set[DIG_MAX_DEVICES] = {};
    const int dev = dig_device();
    if (!attr_set[dev]) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ctc_lex_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CTC_MAX_T * CTC_MAX_C * (int)sizeof(float));
      attr_set[dev] = true;
    }
    hipLaunchKernelGGL(ctc_lex_softmax_kernel, dim3(B * T), dim3(64), 0, stream, logits, ld, C, lp);
    hipLaunchKernelGGL(ctc_lex_score_kernel, dim3(n_chunks, B), dim3(CTC_LEX_WAVES * 64), lds, stream, (const float*)lp, T, C, blank, words, word_len,
                       ldw, W, lex_begin, lex_count, max_count, n_chunks, partial, scores);
  }
  hipLaunchKernelGGL(ctc_lex_fold_kernel, dim3(B), dim3(64), 0, stream, (const unsigned long long*)partial, n_chunks, words, word_len, ldw, T, eos,
                     padding, best_index, logp, ids, score, n);
  return dig_check_launch();
}
