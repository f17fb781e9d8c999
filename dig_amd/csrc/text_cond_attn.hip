// Text-conditional cross-attention of the recognition decoder (`--text_cond_vis`: TextConditionalMultiHeadAttention,
// models/transformer_layer.py:284-383), FOLDED.  The reference builds a key/value memory per query,
//     cond[t,k] = mem[k] + LN_cond(tanh(gamma[t]) * vk[k] + tanh(beta[t])),        vk = LN_vis(vis_proj(mem)),
// and projects the [B, Lq, Lk, d] tensor through linear_k / linear_v.  Both projections have no bias, so they fold across the attention:
//     logit[t,h,k] = u[t,h] . cond[t,k]            with u[t,h] = scale * Wk_h^T q_h[t]      (a GEMM before this kernel)
//     c[t,h]       = sum_k w[t,h,k] cond[t,k]      and  out_h[t] = Wv_h c[t,h]              (a GEMM behind it)
// cond is produced one row at a time in registers and never exists in memory.  d = 64 * C columns, C = d / 64 heads; a lane owns C contiguous
// columns of a row, a wave takes key rows in turn, plain fp32 vector code.
//   forward     : one workgroup per query row.  Sweep 1: logits and LN_cond's statistics of every key -> LDS; softmax over the keys; head-mean
//                 weights (the reference's vis_attn_maps, before dropout); dropout; sweep 2 rebuilds cond from the kept statistics and sums c.
//   backward (q): one workgroup per query row: a sweep over the keys for delta = dc . c in fp32, a second one for du, dfilm and this row's
//                 share of vis_cond_norm's gradients.
//   backward (k): one workgroup per 8 keys of a memory, a loop over the memory's Lq queries: dvk and the residual term of dmem.
//   fold        : vis_cond_norm's gradient shares summed over the query rows in row order.
// Every sum has a fixed order: no floating-point atomics, two runs are bit-identical, and a query row's results do not depend on the batch.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

using dig_rules::TCV_MAXN;
using dig_rules::TCV_MAXQ;
constexpr int TCV_KEYS = 8;                    // keys per workgroup of the key-owning backward (two per wave)

struct TcvParams {
  const bf16_t *film, *u, *vk, *mem;
  const float *lnc_g, *lnc_b;
  float eps;
  int S, Lq, N, spm;
  dig_dropout_t drop;
};

template <int C>
__device__ __forceinline__ void load_cols(const bf16_t* __restrict__ row, int lane, float (&r)[C]) {
  const unsigned* p = reinterpret_cast<const unsigned*>(row + lane * C);
#pragma unroll
  for (int e = 0; e < C / 2; ++e) {
    const unsigned w = p[e];
    r[2 * e] = bf2f((bf16_t)(w & 0xffff));
    r[2 * e + 1] = bf2f((bf16_t)(w >> 16));
  }
}

template <int C>
__device__ __forceinline__ void store_cols(bf16_t* __restrict__ row, int lane, const float (&r)[C]) {
  unsigned* p = reinterpret_cast<unsigned*>(row + lane * C);
#pragma unroll
  for (int e = 0; e < C / 2; ++e) p[e] = pack_bf2(r[2 * e], r[2 * e + 1]);
}

template <int C>
__device__ __forceinline__ float dot_cols(const float (&a)[C], const float (&b)[C]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < C; ++j) s += a[j] * b[j];
  return s;
}

__device__ __forceinline__ float tcv_keep(const dig_dropout_t& d, int t, int k, int sh) {
  if (!d.thr) return 1.f;
  return dig_drop_keep(d.k0, d.k1, ((unsigned)t << 16) | (unsigned)k, (unsigned)sh, d.thr) ? d.scale : 0.f;
}

// z = g * vk + b over the d columns of one key row: LayerNorm statistics (two-pass, in registers)
template <int C>
__device__ __forceinline__ void cond_stats(const float (&g)[C], const float (&b)[C], const float (&vk)[C], float eps, float& mean, float& rstd) {
  float z[C], s = 0.f;
#pragma unroll
  for (int j = 0; j < C; ++j) { z[j] = g[j] * vk[j] + b[j]; s += z[j]; }
  mean = wave_sum(s) * (1.f / (64 * C));
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < C; ++j) { const float e = z[j] - mean; v += e * e; }
  rstd = rsqrtf(wave_sum(v) * (1.f / (64 * C)) + eps);
}

template <int C>
__device__ __forceinline__ void cond_row(const float (&g)[C], const float (&b)[C], const float (&vk)[C], const float (&mem)[C], const float (&lg)[C],
                                         const float (&lb)[C], float mean, float rstd, float (&zh)[C], float (&cond)[C]) {
#pragma unroll
  for (int j = 0; j < C; ++j) {
    zh[j] = (g[j] * vk[j] + b[j] - mean) * rstd;
    cond[j] = mem[j] + zh[j] * lg[j] + lb[j];
  }
}

template <int C>
__device__ __forceinline__ void load_film(const bf16_t* __restrict__ film_row, int lane, float (&g)[C], float (&b)[C]) {
  load_cols<C>(film_row, lane, g);
  load_cols<C>(film_row + 64 * C, lane, b);
#pragma unroll
  for (int j = 0; j < C; ++j) { g[j] = tanhf(g[j]); b[j] = tanhf(b[j]); }
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int C>
__global__ __launch_bounds__(256) void tcv_fwd_kernel(TcvParams p, bf16_t* __restrict__ c_out, float* __restrict__ lse, float* __restrict__ wmean) {
  constexpr int d = 64 * C, HD = C * d;
  __shared__ float W[C * TCV_MAXN];            // logits, then weights [head][key]
  __shared__ float stat[2 * TCV_MAXN];         // LN_cond's (mean, rstd) per key
  __shared__ float red[HD];                    // c of the row, summed over the waves in wave order
  const int r = blockIdx.x, s = r / p.Lq, t = r - s * p.Lq, N = p.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t mrow = (size_t)(s / p.spm) * N;
  float g[C], b[C], lg[C], lb[C];
  load_film<C>(p.film + (size_t)r * 2 * d, lane, g, b);
#pragma unroll
  for (int j = 0; j < C; ++j) { lg[j] = p.lnc_g[lane * C + j]; lb[j] = p.lnc_b[lane * C + j]; }
  {
    float u[C][C];
#pragma unroll
    for (int h = 0; h < C; ++h) load_cols<C>(p.u + (size_t)r * HD + h * d, lane, u[h]);
    for (int k = wave; k < N; k += 4) {
      float vk[C], mem[C], zh[C], cond[C], mean, rstd;
      load_cols<C>(p.vk + (mrow + k) * d, lane, vk);
      load_cols<C>(p.mem + (mrow + k) * d, lane, mem);
      cond_stats<C>(g, b, vk, p.eps, mean, rstd);
      cond_row<C>(g, b, vk, mem, lg, lb, mean, rstd, zh, cond);
#pragma unroll
      for (int h = 0; h < C; ++h) {
        const float a = wave_sum(dot_cols<C>(u[h], cond));
        if (lane == 0) W[h * TCV_MAXN + k] = a;
      }
      if (lane == 0) { stat[2 * k] = mean; stat[2 * k + 1] = rstd; }
    }
  }
  __syncthreads();
  for (int h = wave; h < C; h += 4) {                                    // one wave per head: softmax over the keys
    float m = -INFINITY;
    for (int k = lane; k < N; k += 64) m = fmaxf(m, W[h * TCV_MAXN + k]);
    m = wave_max(m);
    float sum = 0.f;
    for (int k = lane; k < N; k += 64) { const float e = __expf(W[h * TCV_MAXN + k] - m); W[h * TCV_MAXN + k] = e; sum += e; }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int k = lane; k < N; k += 64) W[h * TCV_MAXN + k] *= inv;
    if (lane == 0) lse[(size_t)r * C + h] = m + __logf(sum);
  }
  __syncthreads();
  for (int k = tid; k < N; k += 256) {                                   // head mean before dropout, then dropout after the normalisation
    float a = 0.f;
#pragma unroll
    for (int h = 0; h < C; ++h) a += W[h * TCV_MAXN + k];
    if (wmean) wmean[(size_t)r * N + k] = a * (1.f / C);
    if (p.drop.thr) {
#pragma unroll
      for (int h = 0; h < C; ++h) W[h * TCV_MAXN + k] *= tcv_keep(p.drop, t, k, s * C + h);
    }
  }
  __syncthreads();
  float acc[C][C];
#pragma unroll
  for (int h = 0; h < C; ++h)
#pragma unroll
    for (int j = 0; j < C; ++j) acc[h][j] = 0.f;
  for (int k = wave; k < N; k += 4) {
    float vk[C], mem[C], zh[C], cond[C];
    load_cols<C>(p.vk + (mrow + k) * d, lane, vk);
    load_cols<C>(p.mem + (mrow + k) * d, lane, mem);
    cond_row<C>(g, b, vk, mem, lg, lb, stat[2 * k], stat[2 * k + 1], zh, cond);
#pragma unroll
    for (int h = 0; h < C; ++h) {
      const float w = W[h * TCV_MAXN + k];
#pragma unroll
      for (int j = 0; j < C; ++j) acc[h][j] += w * cond[j];
    }
  }
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int h = 0; h < C; ++h)
#pragma unroll
        for (int j = 0; j < C; ++j) {
          const int e = h * d + lane * C + j;
          red[e] = wv ? red[e] + acc[h][j] : acc[h][j];
        }
    }
    __syncthreads();
  }
  unsigned* out = reinterpret_cast<unsigned*>(c_out + (size_t)r * HD);
  for (int e = tid; e < HD / 2; e += 256) out[e] = pack_bf2(red[2 * e], red[2 * e + 1]);
}

// ---------------------------------------------------------------------------------------------------------------- backward
// One (query, key) pair: rebuilds cond, the weights w[h] = exp(logit - lse) and
//   dlogit[h] = w (m (dc_h . cond) - delta[h]),   dcond = sum_h (w m dc_h + dlogit u_h),   dz = LN_cond's backward of dcond
// (m: the dropout factor).  zh / cond / dcond / dz / dl are left for the caller's sums.
template <int C>
__device__ __forceinline__ void tcv_pair_bwd(const TcvParams& p, int t, int k, int sh0, const float (&g)[C], const float (&b)[C], const float (&vk)[C],
                                             const float (&mem)[C], const float (&lg)[C], const float (&lb)[C], const float (&u)[C][C],
                                             const float (&dc)[C][C], const float (&lse)[C], const float (&delta)[C], float (&zh)[C],
                                             float (&cond)[C], float (&dcond)[C], float (&dz)[C], float (&dl)[C]) {
  float mean, rstd;
  cond_stats<C>(g, b, vk, p.eps, mean, rstd);
  cond_row<C>(g, b, vk, mem, lg, lb, mean, rstd, zh, cond);
#pragma unroll
  for (int j = 0; j < C; ++j) dcond[j] = 0.f;
#pragma unroll
  for (int h = 0; h < C; ++h) {
    const float lgt = wave_sum(dot_cols<C>(u[h], cond));
    const float ph = wave_sum(dot_cols<C>(dc[h], cond));
    const float w = __expf(lgt - lse[h]), m = tcv_keep(p.drop, t, k, sh0 + h);
    dl[h] = w * (m * ph - delta[h]);
    const float wm = w * m;
#pragma unroll
    for (int j = 0; j < C; ++j) dcond[j] += wm * dc[h][j] + dl[h] * u[h][j];
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < C; ++j) { const float a = dcond[j] * lg[j]; s1 += a; s2 += a * zh[j]; }
  s1 = wave_sum(s1) * (1.f / (64 * C));
  s2 = wave_sum(s2) * (1.f / (64 * C));
#pragma unroll
  for (int j = 0; j < C; ++j) dz[j] = rstd * (dcond[j] * lg[j] - s1 - zh[j] * s2);
}

// ws: [R][2d] this row's share of (dlnc_g | dlnc_b), then [R][C] delta
template <int C>
__global__ __launch_bounds__(256) void tcv_bwd_q_kernel(TcvParams p, const float* __restrict__ lse_in,
                                                        const bf16_t* __restrict__ dc_in, bf16_t* __restrict__ du_out, bf16_t* __restrict__ dfilm,
                                                        float* __restrict__ ws) {
  constexpr int d = 64 * C, HD = C * d;
  __shared__ float red[HD + 4 * d];            // du | dgamma | dbeta | dlnc_g | dlnc_b, summed over the waves in wave order
  __shared__ float dpart[4 * C];               // the waves' shares of delta
  const int r = blockIdx.x, s = r / p.Lq, t = r - s * p.Lq, N = p.N, R = p.S * p.Lq;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t mrow = (size_t)(s / p.spm) * N;
  float g[C], b[C], lg[C], lb[C], u[C][C], dc[C][C], lse[C], delta[C];
  load_film<C>(p.film + (size_t)r * 2 * d, lane, g, b);
#pragma unroll
  for (int j = 0; j < C; ++j) { lg[j] = p.lnc_g[lane * C + j]; lb[j] = p.lnc_b[lane * C + j]; }
#pragma unroll
  for (int h = 0; h < C; ++h) {
    load_cols<C>(p.u + (size_t)r * HD + h * d, lane, u[h]);
    load_cols<C>(dc_in + (size_t)r * HD + h * d, lane, dc[h]);
    lse[h] = lse_in[(size_t)r * C + h];
    delta[h] = 0.f;
  }
  // delta[h] = dc_h . c_h = sum_k w m (dc_h . cond[k]), summed here in fp32 over the keys: dlogit sums to zero over the keys when delta is
  // exact, so du = sum_k dlogit cond[k] loses what the rows of cond have in common -- and an error in delta (the bf16 rounding of the stored c)
  // does not cancel: with similar memory rows it would dominate du
  for (int k = wave; k < N; k += 4) {
    float vk[C], mem[C], zh[C], cond[C], mean, rstd;
    load_cols<C>(p.vk + (mrow + k) * d, lane, vk);
    load_cols<C>(p.mem + (mrow + k) * d, lane, mem);
    cond_stats<C>(g, b, vk, p.eps, mean, rstd);
    cond_row<C>(g, b, vk, mem, lg, lb, mean, rstd, zh, cond);
#pragma unroll
    for (int h = 0; h < C; ++h) {
      const float lgt = wave_sum(dot_cols<C>(u[h], cond));
      const float ph = wave_sum(dot_cols<C>(dc[h], cond));
      delta[h] += __expf(lgt - lse[h]) * tcv_keep(p.drop, t, k, s * C + h) * ph;
    }
  }
#pragma unroll
  for (int h = 0; h < C; ++h)
    if (lane == 0) dpart[wave * C + h] = delta[h];
  __syncthreads();
#pragma unroll
  for (int h = 0; h < C; ++h) delta[h] = (dpart[h] + dpart[C + h]) + (dpart[2 * C + h] + dpart[3 * C + h]);
#pragma unroll
  for (int h = 0; h < C; ++h)
    if (tid == h) ws[(size_t)R * 2 * d + (size_t)r * C + h] = delta[h];
  float du[C][C], dga[C], dbe[C], dlg[C], dlb[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    dga[j] = dbe[j] = dlg[j] = dlb[j] = 0.f;
#pragma unroll
    for (int h = 0; h < C; ++h) du[h][j] = 0.f;
  }
  for (int k = wave; k < N; k += 4) {
    float vk[C], mem[C], zh[C], cond[C], dcond[C], dz[C], dl[C];
    load_cols<C>(p.vk + (mrow + k) * d, lane, vk);
    load_cols<C>(p.mem + (mrow + k) * d, lane, mem);
    tcv_pair_bwd<C>(p, t, k, s * C, g, b, vk, mem, lg, lb, u, dc, lse, delta, zh, cond, dcond, dz, dl);
#pragma unroll
    for (int j = 0; j < C; ++j) {
      dlg[j] += dcond[j] * zh[j];
      dlb[j] += dcond[j];
      dga[j] += dz[j] * vk[j];
      dbe[j] += dz[j];
#pragma unroll
      for (int h = 0; h < C; ++h) du[h][j] += dl[h] * cond[j];
    }
  }
#pragma unroll
  for (int j = 0; j < C; ++j) { dga[j] *= 1.f - g[j] * g[j]; dbe[j] *= 1.f - b[j] * b[j]; }   // through the tanh
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int j = 0; j < C; ++j) {
        const int col = lane * C + j;
#pragma unroll
        for (int h = 0; h < C; ++h) red[h * d + col] = wv ? red[h * d + col] + du[h][j] : du[h][j];
        red[HD + col] = wv ? red[HD + col] + dga[j] : dga[j];
        red[HD + d + col] = wv ? red[HD + d + col] + dbe[j] : dbe[j];
        red[HD + 2 * d + col] = wv ? red[HD + 2 * d + col] + dlg[j] : dlg[j];
        red[HD + 3 * d + col] = wv ? red[HD + 3 * d + col] + dlb[j] : dlb[j];
      }
    }
    __syncthreads();
  }
  unsigned* o1 = reinterpret_cast<unsigned*>(du_out + (size_t)r * HD);
  for (int e = tid; e < HD / 2; e += 256) o1[e] = pack_bf2(red[2 * e], red[2 * e + 1]);
  unsigned* o2 = reinterpret_cast<unsigned*>(dfilm + (size_t)r * 2 * d);
  for (int e = tid; e < d; e += 256) o2[e] = pack_bf2(red[HD + 2 * e], red[HD + 2 * e + 1]);
  for (int e = tid; e < 2 * d; e += 256) ws[(size_t)r * 2 * d + e] = red[HD + 2 * d + e];
}

// grid (ceil(N / 8), M); slots_per_mem = 1: memory m belongs to sequence m.  delta [R][C] comes from the query-owning kernel's launch.
template <int C>
__global__ __launch_bounds__(256) void tcv_bwd_k_kernel(TcvParams p, const float* __restrict__ lse_in, const bf16_t* __restrict__ dc_in,
                                                        const float* __restrict__ delta_in, bf16_t* __restrict__ dvk, bf16_t* __restrict__ dmem) {
  constexpr int d = 64 * C, HD = C * d;
  const int s = blockIdx.y, N = p.N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = blockIdx.x * TCV_KEYS + wave * 2;
  if (k0 >= N) return;                                                   // (wave-uniform; no barrier below)
  const bool two = k0 + 1 < N;
  const size_t mrow = (size_t)s * N;
  float lg[C], lb[C], vk0[C], mem0[C], vk1[C], mem1[C], av0[C], am0[C], av1[C], am1[C];
#pragma unroll
  for (int j = 0; j < C; ++j) { lg[j] = p.lnc_g[lane * C + j]; lb[j] = p.lnc_b[lane * C + j]; av0[j] = am0[j] = av1[j] = am1[j] = 0.f; }
  load_cols<C>(p.vk + (mrow + k0) * d, lane, vk0);
  load_cols<C>(p.mem + (mrow + k0) * d, lane, mem0);
  load_cols<C>(p.vk + (mrow + k0 + (two ? 1 : 0)) * d, lane, vk1);
  load_cols<C>(p.mem + (mrow + k0 + (two ? 1 : 0)) * d, lane, mem1);
  for (int t = 0; t < p.Lq; ++t) {
    const size_t r = (size_t)s * p.Lq + t;
    float g[C], b[C], u[C][C], dc[C][C], lse[C], delta[C], zh[C], cond[C], dcond[C], dz[C], dl[C];
    load_film<C>(p.film + r * 2 * d, lane, g, b);
#pragma unroll
    for (int h = 0; h < C; ++h) {
      load_cols<C>(p.u + r * HD + h * d, lane, u[h]);
      load_cols<C>(dc_in + r * HD + h * d, lane, dc[h]);
      lse[h] = lse_in[r * C + h];
      delta[h] = delta_in[r * C + h];
    }
    tcv_pair_bwd<C>(p, t, k0, s * C, g, b, vk0, mem0, lg, lb, u, dc, lse, delta, zh, cond, dcond, dz, dl);
#pragma unroll
    for (int j = 0; j < C; ++j) { av0[j] += g[j] * dz[j]; am0[j] += dcond[j]; }
    if (two) {
      tcv_pair_bwd<C>(p, t, k0 + 1, s * C, g, b, vk1, mem1, lg, lb, u, dc, lse, delta, zh, cond, dcond, dz, dl);
#pragma unroll
      for (int j = 0; j < C; ++j) { av1[j] += g[j] * dz[j]; am1[j] += dcond[j]; }
    }
  }
  store_cols<C>(dvk + (mrow + k0) * d, lane, av0);
  store_cols<C>(dmem + (mrow + k0) * d, lane, am0);
  if (two) {
    store_cols<C>(dvk + (mrow + k0 + 1) * d, lane, av1);
    store_cols<C>(dmem + (mrow + k0 + 1) * d, lane, am1);
  }
}

// out[col] += sum_r parts[r][col], rows in order (four interleaved chains with a fixed pairing: one order)
__global__ __launch_bounds__(64) void tcv_fold_kernel(const float* __restrict__ parts, int R, int cols, float* __restrict__ out_g, float* __restrict__ out_b) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= cols) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int r = 0;
  for (; r + 3 < R; r += 4) {
    a0 += parts[(size_t)r * cols + col];
    a1 += parts[(size_t)(r + 1) * cols + col];
    a2 += parts[(size_t)(r + 2) * cols + col];
    a3 += parts[(size_t)(r + 3) * cols + col];
  }
  for (; r < R; ++r) a0 += parts[(size_t)r * cols + col];
  const float tot = (a0 + a1) + (a2 + a3);
  const int d = cols / 2;
  if (col < d) out_g[col] += tot;
  else out_b[col - d] += tot;
}

}  // namespace

// C-ABI: see include/dig_hip.h
extern "C" int dig_tcv_attn_fwd(const void* film, const void* u, const void* vk, const void* mem, const float* lnc_g, const float* lnc_b, float eps,
                                void* c, float* lse, float* wmean, int S, int Lq, int N, int heads, int d, int slots_per_mem,
                                const dig_dropout_t* drop, hipStream_t stream) {
  if (int rc = dig_rules::tcv_attn_fwd(film, u, vk, mem, lnc_g, lnc_b, eps, c, lse, wmean, S, Lq, N, heads, d, slots_per_mem, drop)) return rc;
  TcvParams p{(const bf16_t*)film, (const bf16_t*)u, (const bf16_t*)vk, (const bf16_t*)mem, lnc_g, lnc_b, eps, S, Lq, N, slots_per_mem,
              drop ? *drop : dig_dropout_t{}};
  // consecutive workgroups = the queries of one sequence, then the slots of one memory: they re-read its vk / mem rows from L2 together
  const dim3 grid((unsigned)(S * Lq)), block(256);
  if (heads == 2) hipLaunchKernelGGL(tcv_fwd_kernel<2>, grid, block, 0, stream, p, (bf16_t*)c, lse, wmean);
  else if (heads == 6) hipLaunchKernelGGL(tcv_fwd_kernel<6>, grid, block, 0, stream, p, (bf16_t*)c, lse, wmean);
  else hipLaunchKernelGGL(tcv_fwd_kernel<8>, grid, block, 0, stream, p, (bf16_t*)c, lse, wmean);
  return dig_check_launch();
}

extern "C" int dig_tcv_attn_bwd(const void* film, const void* u, const void* vk, const void* mem, const float* lnc_g, const float* lnc_b, float eps,
                                const void* c, const float* lse, const void* dc, void* du, void* dfilm, void* dvk, void* dmem, float* dlnc_g,
                                float* dlnc_b, float* workspace, int S, int Lq, int N, int heads, int d, int slots_per_mem,
                                const dig_dropout_t* drop, hipStream_t stream) {
  if (int rc = dig_rules::tcv_attn_bwd(film, u, vk, mem, lnc_g, lnc_b, eps, c, lse, dc, du, dfilm, dvk, dmem, dlnc_g, dlnc_b, workspace, S, Lq, N,
                                       heads, d, slots_per_mem, drop))
    return rc;
  TcvParams p{(const bf16_t*)film, (const bf16_t*)u, (const bf16_t*)vk, (const bf16_t*)mem, lnc_g, lnc_b, eps, S, Lq, N, 1,
              drop ? *drop : dig_dropout_t{}};
  const int R = S * Lq;
  const float* delta = workspace + (size_t)R * 2 * d;
  const dim3 gq((unsigned)R), gk((unsigned)((N + TCV_KEYS - 1) / TCV_KEYS), (unsigned)S), block(256);
#define TCV_BWD(Cn)                                                                                                                              \
  hipLaunchKernelGGL(tcv_bwd_q_kernel<Cn>, gq, block, 0, stream, p, lse, (const bf16_t*)dc, (bf16_t*)du, (bf16_t*)dfilm, workspace); \
  hipLaunchKernelGGL(tcv_bwd_k_kernel<Cn>, gk, block, 0, stream, p, lse, (const bf16_t*)dc, delta, (bf16_t*)dvk, (bf16_t*)dmem)
  if (heads == 2) { TCV_BWD(2); }
  else if (heads == 6) { TCV_BWD(6); }
  else { TCV_BWD(8); }
#undef TCV_BWD
  hipLaunchKernelGGL(tcv_fold_kernel, dim3((unsigned)((2 * d + 63) / 64)), dim3(64), 0, stream, workspace, R, 2 * d, dlnc_g, dlnc_b);
  return dig_check_launch();
}
