// libdig_cpu.so -- a plain-C++ build of the hot-path part of the C ABI in include/dig_hip.h (last bullet).
//
// What this is: the same entry points (names, argument lists, error codes, in-place / accumulate conventions, bf16 storage with
// round-to-nearest-even) as libdig_hip.so for the operators of the PRE-TRAINING step, written as
// straightforward loops over host memory; `stream` is ignored and every call is synchronous.  It exists so that the operator-level
// parity tests (tests/test_gpu_kernels.py) and the host logic of dig_amd/ops.py above the ABI run in a container without a GPU.
//
// What this is NOT: it is not the oracle (tests compare it, like the HIP library, against fp32 torch references and oracle/), and
// it is not a fallback -- nothing under dig_amd/ loads it; the product raises without libdig_hip.so (dig_amd/_lib.py).  Entry
// points outside the pre-training step (recognition decode, fine-tune sequence attention, GRU head, input transform) are in
// dig_cpu_rec.cpp; together the two files export every entry point the header declares (tests/test_cpu_abi.py).
//
// Build: make -C cpu_abi   (g++ -O2 -fopenmp -shared -fPIC; __graft_entry__.build() runs it)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dig_cpu_common.h"

namespace {

inline float gelu_f(float x) { return 0.5f * x * (1.0f + std::erf(x * 0.70710678118654752f)); }
inline float dgelu_f(float x) {
  const float cdf = 0.5f * (1.0f + std::erf(x * 0.70710678118654752f));
  return cdf + x * 0.39894228040143268f * std::exp(-0.5f * x * x);
}
// element (i, j) of a [rows, cols] tensor under element dropout + drop-path (common.h dig_drop_apply8; a dropped element is +0)
inline float drop_apply(float v, const dig_dropout_t& d, long long i, int j, int cols) {
  float s = 1.f;
  if (d.pthr) s = drop_keep(d.pk0, d.pk1, (unsigned)(i / d.rows_per_sample), 0u, d.pthr) ? d.pscale : 0.f;
  if (d.thr) {
    s *= d.scale;
    return drop_keep(d.k0, d.k1, (unsigned)i * (unsigned)cols + (unsigned)j, 0u, d.thr) ? v * s : 0.f;
  }
  return v * s;
}

constexpr int BR = 64, N_TOK = 256, DH = 64;

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------------------------ GEMM
int dig_gemm_bf16_dropout(const void* A_, const void* B_, void* C_, int I, int J, int R, int lda, int ldb, int ldc, int trans_a,
                          int trans_b, int out_kind, const float* bias, const void* resid_, int ldr, void* pre_, int ldp, float alpha,
                          int alpha_cols, int act, int splits, int a_rows, int b_rows, int bk, float* colsum_partials,
                          const dig_dropout_t* drop, hipStream_t) {
  if (int rc = dig_rules::gemm_bf16_dropout(A_, B_, C_, I, J, R, lda, ldb, ldc, trans_a, trans_b, out_kind, bias, resid_, ldr, pre_, ldp, alpha,
                                            alpha_cols, act, splits, a_rows, b_rows, bk, colsum_partials, drop))
    return rc;
  const bool dropping = drop && (drop->thr || drop->pthr);
  const int per = (int)dig_rules::gemm_rows_per_split(R, splits);
  const bf16_t* A = (const bf16_t*)A_;
  const bf16_t* B = (const bf16_t*)B_;
  const bf16_t* resid = (const bf16_t*)resid_;
  bf16_t* pre = (bf16_t*)pre_;
  const int arows = a_rows > 0 ? a_rows : (trans_a ? R : I);
  const int brows = b_rows > 0 ? b_rows : (trans_b ? R : J);
  // operands as dense fp32 [I][R] / [J][R] (rows past a_rows / b_rows read as zero -- and, as through the HIP build's buffer descriptors of
  // a_rows x lda / b_rows x ldb elements, anything past the operand's last element: a direct operand whose reduction runs past its row pitch
  // (ConvPatchNet's 2592-column weight rows under a 2624-column zero-padded im2col matrix) wraps into the next row and ends in zeros)
  const size_t a_elems = (size_t)arows * lda, b_elems = (size_t)brows * ldb;
  std::vector<float> a((size_t)I * R), b((size_t)J * R);
#pragma omp parallel for
  for (int i = 0; i < I; ++i)
    for (int r = 0; r < R; ++r) {
      const int row = trans_a ? r : i;
      const size_t at = trans_a ? (size_t)r * lda + i : (size_t)i * lda + r;
      a[(size_t)i * R + r] = (row < arows && at < a_elems) ? bf2f(A[at]) : 0.f;
    }
#pragma omp parallel for
  for (int j = 0; j < J; ++j)
    for (int r = 0; r < R; ++r) {
      const int row = trans_b ? r : j;
      const size_t at = trans_b ? (size_t)r * ldb + j : (size_t)j * ldb + r;
      b[(size_t)j * R + r] = (row < brows && at < b_elems) ? bf2f(B[at]) : 0.f;
    }
  if (out_kind == 2) {
    float* C = (float*)C_;
#pragma omp parallel for collapse(2)
    for (int s = 0; s < splits; ++s)
      for (int i = 0; i < I; ++i) {
        const int r0 = s * per, r1 = std::min(R, r0 + per);
        for (int j = 0; j < J; ++j) {
          float acc = 0.f;
          for (int r = r0; r < r1; ++r) acc += a[(size_t)i * R + r] * b[(size_t)j * R + r];
          C[((size_t)s * I + i) * J + j] = acc;
        }
      }
    return DIG_OK;
  }
  const int groups = (I + 63) / 64;
  std::vector<float> csum(colsum_partials ? (size_t)groups * J : 0, 0.f);
#pragma omp parallel for
  for (int g = 0; g < groups; ++g)
    for (int i = g * 64; i < std::min(I, g * 64 + 64); ++i)
      for (int j = 0; j < J; ++j) {
        float acc = 0.f;
        for (int r = 0; r < R; ++r) acc += a[(size_t)i * R + r] * b[(size_t)j * R + r];
        float v = (acc + (bias ? bias[j] : 0.f)) * (j < alpha_cols ? alpha : 1.0f);
        if (act == 1) {
          if (pre) pre[(size_t)i * ldp + j] = f2bf(v);
          v = gelu_f(v);
          if (dropping) v = drop_apply(v, *drop, i, j, J);
        } else if (act == 2) {
          v *= dgelu_f(bf2f(resid[(size_t)i * ldr + j]));
          if (dropping) v = drop_apply(v, *drop, i, j, J);
          if (colsum_partials) csum[(size_t)g * J + j] += v;
        } else if (dropping) {
          v = drop_apply(v, *drop, i, j, J);
        }
        if (resid && act != 2) v += bf2f(resid[(size_t)i * ldr + j]);
        if (out_kind == 0) ((bf16_t*)C_)[(size_t)i * ldc + j] = f2bf(v);
        else ((float*)C_)[(size_t)i * ldc + j] = v;
      }
  if (colsum_partials) std::memcpy(colsum_partials, csum.data(), csum.size() * sizeof(float));
  return DIG_OK;
}

int dig_gemm_bf16(const void* A, const void* B, void* C, int I, int J, int R, int lda, int ldb, int ldc, int trans_a, int trans_b,
                  int out_kind, const float* bias, const void* resid, int ldr, void* pre_act, int ldp, float alpha, int alpha_cols,
                  int act, int splits, int a_rows, int b_rows, int bk, float* colsum_partials, hipStream_t stream) {
  return dig_gemm_bf16_dropout(A, B, C, I, J, R, lda, ldb, ldc, trans_a, trans_b, out_kind, bias, resid, ldr, pre_act, ldp, alpha, alpha_cols,
                               act, splits, a_rows, b_rows, bk, colsum_partials, nullptr, stream);
}

int dig_reduce_partials_bf16(const float* partials, int splits, long long n, void* out_, hipStream_t) {
  if (int rc = dig_rules::reduce_partials_bf16(partials, splits, n, out_)) return rc;
  bf16_t* out = (bf16_t*)out_;
  for (long long e = 0; e < n; ++e) {
    float a = 0.f;
    for (int s = 0; s < splits; ++s) a += partials[(long long)s * n + e];
    out[e] = f2bf(a);
  }
  return DIG_OK;
}
int dig_reduce_partials(const float* partials, int splits, long long n, float* out, int accumulate, hipStream_t) {
  if (int rc = dig_rules::reduce_partials(partials, splits, n, out, accumulate)) return rc;
#pragma omp parallel for
  for (long long e = 0; e < n; ++e) {
    float acc = accumulate ? out[e] : 0.f;
    for (int s = 0; s < splits; ++s) acc += partials[(long long)s * n + e];
    out[e] = acc;
  }
  return DIG_OK;
}

int dig_reduce_partials_multi(const dig_reduce_seg_t* segs, int n_segs, hipStream_t stream) {
  if (int rc = dig_rules::reduce_partials_multi(segs, n_segs)) return rc;
  for (int k = 0; k < n_segs; ++k) {
    const int rc = dig_reduce_partials(segs[k].partials, segs[k].splits, segs[k].n, segs[k].out, 1, stream);
    if (rc) return rc;
  }
  return DIG_OK;
}

int dig_colsum_partials_multi(const dig_colsum_seg_t* segs, int n_segs, hipStream_t) {
  if (int rc = dig_rules::colsum_partials_multi(segs, n_segs)) return rc;
  for (int k = 0; k < n_segs; ++k) {
    const dig_colsum_seg_t& g = segs[k];
    for (int c = 0; c < g.C; ++c) {
      float a = 0.f;
      for (int b = 0; b < g.n_parts; ++b) a += g.partials[(size_t)b * g.stride + c];
      g.out[c] += a;
    }
  }
  return DIG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ attention
int dig_attn_fwd_dropout(const void* qkv_, void* ctx_, float* lse, int n_img, int heads, int embed_dim, const dig_dropout_t* drop,
                         int q_rows, hipStream_t) {
  if (int rc = dig_rules::attn_fwd_dropout(qkv_, ctx_, lse, n_img, heads, embed_dim, drop, q_rows)) return rc;
  const bf16_t* qkv = (const bf16_t*)qkv_;
  bf16_t* ctx = (bf16_t*)ctx_;
  const int D = embed_dim, ld = 3 * D, nq = (q_rows + 31) / 32 * 32;
  const bool dropping = drop && drop->thr;
#pragma omp parallel for collapse(2)
  for (int b = 0; b < n_img; ++b)
    for (int h = 0; h < heads; ++h) {
      std::vector<float> s(N_TOK);
      for (int i = 0; i < nq; ++i) {
        const bf16_t* q = qkv + ((size_t)b * N_TOK + i) * ld + h * DH;
        float mx = -3.0e38f;
        for (int j = 0; j < N_TOK; ++j) {
          const bf16_t* k = qkv + ((size_t)b * N_TOK + j) * ld + D + h * DH;
          float acc = 0.f;
          for (int c = 0; c < DH; ++c) acc += bf2f(q[c]) * bf2f(k[c]);
          s[j] = acc;
          mx = std::max(mx, acc);
        }
        float sum = 0.f;
        for (int j = 0; j < N_TOK; ++j) { s[j] = std::exp(s[j] - mx); sum += s[j]; }
        lse[((size_t)b * heads + h) * N_TOK + i] = mx + std::log(sum);
        const float inv = 1.0f / sum;
        float o[DH];
        for (int c = 0; c < DH; ++c) o[c] = 0.f;
        for (int j = 0; j < N_TOK; ++j) {
          float p = s[j] * inv;
          if (dropping) p = drop_keep(drop->k0, drop->k1, ((unsigned)i << 16) | (unsigned)j, (unsigned)(b * heads + h), drop->thr) ? p * drop->scale : 0.f;
          const bf16_t* v = qkv + ((size_t)b * N_TOK + j) * ld + 2 * D + h * DH;
          for (int c = 0; c < DH; ++c) o[c] += p * bf2f(v[c]);
        }
        for (int c = 0; c < DH; ++c) ctx[((size_t)b * N_TOK + i) * D + h * DH + c] = f2bf(o[c]);
      }
    }
  return DIG_OK;
}

int dig_attn_fwd(const void* qkv, void* ctx, float* lse, int n_img, int heads, int embed_dim, hipStream_t stream) {
  return dig_attn_fwd_dropout(qkv, ctx, lse, n_img, heads, embed_dim, nullptr, N_TOK, stream);
}

// (one backward form in this build: the switch of the HIP build is accepted and ignored)
int dig_attn_bwd_mode(int) { return 0; }
int dig_attn_bwd_store(int) { return 0; }   // (one store form in the CPU build)

// the attention sub-block in one call (HIP: csrc/attn_block.hip): here the same three steps, one after the other.  qkv / lse null: the
// momentum branch keeps nothing (the q | k | v rows then live in a temporary)
int dig_attn_block_fwd(const void* ln1, const void* x, const void* qkv_w, const float* qkv_b, const void* proj_w, const float* proj_b,
                       void* qkv, void* ctx, float* lse, void* x_mid, int n_img, int heads, int embed_dim, float scale, hipStream_t stream) {
  if (int rc = dig_rules::attn_block_fwd(ln1, x, qkv_w, qkv_b, proj_w, proj_b, qkv, ctx, lse, x_mid, n_img, heads, embed_dim, scale)) return rc;
  const int D = embed_dim, R = n_img * N_TOK;
  std::vector<bf16_t> tq;
  std::vector<float> tl;
  if (!qkv) {
    tq.resize((size_t)R * 3 * D + 8);
    tl.resize((size_t)n_img * heads * N_TOK);
    qkv = (void*)(((uintptr_t)tq.data() + 15) & ~(uintptr_t)15);
    lse = tl.data();
  }
  int rc = dig_gemm_bf16(ln1, qkv_w, qkv, R, 3 * D, D, D, D, 3 * D, 0, 0, 0, qkv_b, nullptr, 0, nullptr, 0, scale, D, 0, 1, 0, 0, 0, nullptr, stream);
  if (rc) return rc;
  rc = dig_attn_fwd(qkv, ctx, lse, n_img, heads, D, stream);
  if (rc) return rc;
  return dig_gemm_bf16(ctx, proj_w, x_mid, R, D, D, D, D, D, 0, 0, 0, proj_b, x, D, nullptr, 0, 1.0f, 0, 0, 1, 0, 0, 0, nullptr, stream);
}

int dig_attn_bwd_dropout(const void* qkv_, const void* ctx_, const void* dctx_, const float* lse, void* dqkv_, int n_img, int heads,
                         int embed_dim, float scale, float* q_colsum, float* v_colsum, const dig_dropout_t* drop, int q_rows, hipStream_t) {
  if (int rc = dig_rules::attn_bwd_dropout(qkv_, ctx_, dctx_, lse, dqkv_, n_img, heads, embed_dim, scale, q_colsum, v_colsum, drop, q_rows))
    return rc;
  const int nqb = (q_rows + 31) / 32;
  const bf16_t* qkv = (const bf16_t*)qkv_;
  const bf16_t* ctx = (const bf16_t*)ctx_;
  const bf16_t* dctx = (const bf16_t*)dctx_;
  bf16_t* dqkv = (bf16_t*)dqkv_;
  const int D = embed_dim, ld = 3 * D, nq = nqb * 32;
  const bool dropping = drop && drop->thr;
#pragma omp parallel for
  for (int b = 0; b < n_img; ++b) {
    std::vector<float> qs(q_colsum ? D : 0, 0.f), vs(q_colsum ? D : 0, 0.f);
    for (int h = 0; h < heads; ++h) {
      std::vector<float> dk((size_t)N_TOK * DH, 0.f), dv((size_t)N_TOK * DH, 0.f), p(N_TOK), dp(N_TOK);
      for (int i = 0; i < nq; ++i) {
        const size_t row = (size_t)b * N_TOK + i;
        const bf16_t* q = qkv + row * ld + h * DH;
        const bf16_t* o = ctx + row * D + h * DH;
        const bf16_t* go = dctx + row * D + h * DH;
        const float l = lse[((size_t)b * heads + h) * N_TOK + i];
        float delta = 0.f;
        for (int c = 0; c < DH; ++c) delta += bf2f(go[c]) * bf2f(o[c]);
        for (int j = 0; j < N_TOK; ++j) {
          const bf16_t* k = qkv + ((size_t)b * N_TOK + j) * ld + D + h * DH;
          const bf16_t* v = qkv + ((size_t)b * N_TOK + j) * ld + 2 * D + h * DH;
          float s = 0.f, d = 0.f;
          for (int c = 0; c < DH; ++c) { s += bf2f(q[c]) * bf2f(k[c]); d += bf2f(go[c]) * bf2f(v[c]); }
          p[j] = std::exp(s - l);
          dp[j] = d;
        }
        float dq[DH];
        for (int c = 0; c < DH; ++c) dq[c] = 0.f;
        for (int j = 0; j < N_TOK; ++j) {
          float keep = 1.f;
          if (dropping) keep = drop_keep(drop->k0, drop->k1, ((unsigned)i << 16) | (unsigned)j, (unsigned)(b * heads + h), drop->thr) ? drop->scale : 0.f;
          // (both rounded to bf16, as the HIP kernels pack them for the matrix unit: with fp32 values here a sum whose terms cancel exactly
          //  in the kernel came out as round-off, 1e-6 where the kernel writes 0)
          const float pd = bf2f(f2bf(p[j] * keep));                   // the probability that multiplied V in the forward
          const float ds = bf2f(f2bf(p[j] * (dp[j] * keep - delta))); // d(score): softmax backward through the (dropped) probabilities
          const bf16_t* k = qkv + ((size_t)b * N_TOK + j) * ld + D + h * DH;
          for (int c = 0; c < DH; ++c) {
            dq[c] += ds * bf2f(k[c]);
            dk[(size_t)j * DH + c] += ds * bf2f(q[c]);
            dv[(size_t)j * DH + c] += pd * bf2f(go[c]);
          }
        }
        for (int c = 0; c < DH; ++c) {
          dqkv[row * ld + h * DH + c] = f2bf(dq[c] * scale);
          if (q_colsum) qs[h * DH + c] += dq[c] * scale;
        }
      }
      for (int j = 0; j < N_TOK; ++j)
        for (int c = 0; c < DH; ++c) {
          dqkv[((size_t)b * N_TOK + j) * ld + D + h * DH + c] = f2bf(dk[(size_t)j * DH + c]);
          dqkv[((size_t)b * N_TOK + j) * ld + 2 * D + h * DH + c] = f2bf(dv[(size_t)j * DH + c]);
          if (q_colsum) vs[h * DH + c] += dv[(size_t)j * DH + c];
        }
    }
    if (q_colsum) {
      std::memcpy(q_colsum + (size_t)b * D, qs.data(), D * sizeof(float));
      std::memcpy(v_colsum + (size_t)b * D, vs.data(), D * sizeof(float));
    }
  }
  return DIG_OK;
}

int dig_attn_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int n_img, int heads, int embed_dim,
                 float scale, float* q_colsum, float* v_colsum, hipStream_t stream) {
  return dig_attn_bwd_dropout(qkv, ctx, dctx, lse, dqkv, n_img, heads, embed_dim, scale, q_colsum, v_colsum, nullptr, N_TOK, stream);
}

// the projection's data gradient in front of the backward: d(ctx) = bf16(dy Wproj) with fp32 accumulation, then the plain backward
int dig_attn_bwd_proj(const void* qkv, const void* ctx, const void* dy_, const void* projt_, const float* lse, void* dqkv, int n_img, int heads,
                      int embed_dim, float scale, float* q_colsum, float* v_colsum, hipStream_t stream) {
  if (int rc = dig_rules::attn_bwd_proj(qkv, ctx, dy_, projt_, lse, dqkv, n_img, heads, embed_dim, scale, q_colsum, v_colsum)) return rc;
  const int D = embed_dim;
  const long R = (long)n_img * N_TOK;
  const uint16_t* dy = (const uint16_t*)dy_;
  const uint16_t* wt = (const uint16_t*)projt_;                       // [in i][out o]
  std::vector<float> w((size_t)D * D);
  for (size_t k = 0; k < w.size(); ++k) w[k] = bf2f(wt[k]);
  std::vector<uint16_t> dctx((size_t)R * D);
#pragma omp parallel for
  for (long r = 0; r < R; ++r) {
    std::vector<float> row(D);
    for (int o = 0; o < D; ++o) row[o] = bf2f(dy[r * D + o]);
    for (int i = 0; i < D; ++i) {
      float a = 0.f;
      for (int o = 0; o < D; ++o) a += row[o] * w[(size_t)i * D + o];
      dctx[r * D + i] = f2bf(a);
    }
  }
  return dig_attn_bwd(qkv, ctx, dctx.data(), lse, dqkv, n_img, heads, embed_dim, scale, q_colsum, v_colsum, stream);
}

// ------------------------------------------------------------------------------------------------------------------ LayerNorm

int dig_layernorm_fwd(const void* x_, const float* gamma, const float* beta, void* y_, float* mean, float* rstd, int rows, int D, float eps,
                      int fuse_gelu, hipStream_t) {
  if (int rc = dig_rules::layernorm_fwd(x_, gamma, beta, y_, mean, rstd, rows, D, eps, fuse_gelu)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
  bf16_t* y = (bf16_t*)y_;
#pragma omp parallel for
  for (int r = 0; r < rows; ++r) {
    float s = 0.f;
    for (int c = 0; c < D; ++c) s += bf2f(x[(size_t)r * D + c]);
    const float mu = s / D;
    float q = 0.f;
    for (int c = 0; c < D; ++c) { const float d = bf2f(x[(size_t)r * D + c]) - mu; q += d * d; }
    const float rs = 1.0f / std::sqrt(q / D + eps);
    for (int c = 0; c < D; ++c) {
      float v = (bf2f(x[(size_t)r * D + c]) - mu) * rs * gamma[c] + beta[c];
      if (fuse_gelu) v = gelu_f(v);
      y[(size_t)r * D + c] = f2bf(v);
    }
    mean[r] = mu;
    rstd[r] = rs;
  }
  return DIG_OK;
}


// the partial rows are the sums over the row slices part p owns (rows p, p + parts, ...); their total is what finalize adds
int dig_layernorm_bwd_partials(const void* dy_, const void* x_, const float* gamma, const float* beta, const float* mean, const float* rstd,
                               const void* dres_, void* dx_, float* workspace, int rows, int D, int fuse_gelu, hipStream_t) {
  if (int rc = dig_rules::layernorm_bwd_partials(dy_, x_, gamma, beta, mean, rstd, dres_, dx_, workspace, rows, D, fuse_gelu)) return rc;
  const bf16_t* dy = (const bf16_t*)dy_;
  const bf16_t* x = (const bf16_t*)x_;
  const bf16_t* dres = (const bf16_t*)dres_;
  bf16_t* dx = (bf16_t*)dx_;
  const int parts = dig_rules::layernorm_bwd_parts(rows);
  std::memset(workspace, 0, (size_t)parts * 3 * D * sizeof(float));
#pragma omp parallel for
  for (int p = 0; p < parts; ++p) {
    float* w = workspace + (size_t)p * 3 * D;
    std::vector<float> xh(D), d(D);
    for (int r = p; r < rows; r += parts) {
      float c1 = 0.f, c2 = 0.f;
      for (int c = 0; c < D; ++c) {
        xh[c] = (bf2f(x[(size_t)r * D + c]) - mean[r]) * rstd[r];
        float g = bf2f(dy[(size_t)r * D + c]);
        if (fuse_gelu) g *= dgelu_f(xh[c] * gamma[c] + beta[c]);
        w[c] += g * xh[c];
        w[D + c] += g;
        d[c] = g * gamma[c];
        c1 += d[c];
        c2 += d[c] * xh[c];
      }
      c1 /= D;
      c2 /= D;
      for (int c = 0; c < D; ++c) {
        float o = rstd[r] * (d[c] - c1 - xh[c] * c2);
        if (dres) { const float e = bf2f(dres[(size_t)r * D + c]); o += e; w[2 * D + c] += e; }
        dx[(size_t)r * D + c] = f2bf(o);
      }
    }
  }
  return DIG_OK;
}

int dig_layernorm_bwd_finalize(const float* workspace, int rows, int D, float* dgamma, float* dbeta, float* dcolsum, hipStream_t) {
  if (int rc = dig_rules::layernorm_bwd_finalize(workspace, rows, D, dgamma, dbeta, dcolsum)) return rc;
  const int parts = dig_rules::layernorm_bwd_parts(rows);
  for (int c = 0; c < D; ++c) {
    float a = 0.f, b = 0.f, e = 0.f;
    for (int p = 0; p < parts; ++p) {
      a += workspace[(size_t)p * 3 * D + c];
      b += workspace[(size_t)p * 3 * D + D + c];
      e += workspace[(size_t)p * 3 * D + 2 * D + c];
    }
    dgamma[c] += a;
    dbeta[c] += b;
    if (dcolsum) dcolsum[c] += e;
  }
  return DIG_OK;
}

int dig_layernorm_bwd_finalize_parts(const float* workspace, int parts, int D, float* dgamma, float* dbeta, float* dcolsum, hipStream_t) {
  if (int rc = dig_rules::layernorm_bwd_finalize_parts(workspace, parts, D, dgamma, dbeta, dcolsum)) return rc;
  for (int c = 0; c < D; ++c) {
    float a = 0.f, b = 0.f, e = 0.f;
    for (int p = 0; p < parts; ++p) {
      a += workspace[(size_t)p * 3 * D + c];
      b += workspace[(size_t)p * 3 * D + D + c];
      e += workspace[(size_t)p * 3 * D + 2 * D + c];
    }
    dgamma[c] += a;
    dbeta[c] += b;
    if (dcolsum) dcolsum[c] += e;
  }
  return DIG_OK;
}

int dig_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                      const void* dres, void* dx, float* dgamma, float* dbeta, float* dcolsum, float* workspace, int rows, int D,
                      int fuse_gelu, hipStream_t stream) {
  if (int rc = dig_rules::layernorm_bwd(dy, x, gamma, beta, mean, rstd, dres, dx, dgamma, dbeta, dcolsum, workspace, rows, D, fuse_gelu)) return rc;
  const int rc = dig_layernorm_bwd_partials(dy, x, gamma, beta, mean, rstd, dres, dx, workspace, rows, D, fuse_gelu, stream);
  if (rc != DIG_OK) return rc;
  return dig_layernorm_bwd_finalize(workspace, rows, D, dgamma, dbeta, dcolsum, stream);
}

// ------------------------------------------------------------------------------------------------------------------ BatchNorm
long long dig_bn_stats_workspace_bytes(int rows, int C) { return (long long)((rows + 63) / 64) * 2 * C * sizeof(float); }

int dig_bn_stats(const void* x_, float* sums, float* workspace, int rows, int C, hipStream_t) {
  if (int rc = dig_rules::bn_stats(x_, sums, workspace, rows, C)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < rows; ++r) { const float v = bf2f(x[(size_t)r * C + c]); a += v; b += v * v; }
    sums[c] = a;
    sums[C + c] = b;
  }
  return DIG_OK;
}

int dig_bn_fwd_apply(const void* x_, const float* sums, float n_total, float eps, const float* gamma, const float* beta, int relu, void* y_,
                     float* mean_out, float* rstd_out, int rows, int C, hipStream_t) {
  if (int rc = dig_rules::bn_fwd_apply_running(x_, sums, n_total, eps, gamma, beta, relu, y_, mean_out, rstd_out, 0.f, nullptr, nullptr, rows, C))
    return rc;
  const bf16_t* x = (const bf16_t*)x_;
  bf16_t* y = (bf16_t*)y_;
  const float inv_n = 1.0f / n_total;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    const float mu = sums[c] * inv_n;
    const float var = std::max(sums[C + c] * inv_n - mu * mu, 0.f);
    const float rs = 1.0f / std::sqrt(var + eps);
    mean_out[c] = mu;
    rstd_out[c] = rs;
    for (int r = 0; r < rows; ++r) {
      float o = (bf2f(x[(size_t)r * C + c]) - mu) * rs;
      if (gamma) o = o * gamma[c] + beta[c];
      if (relu) o = std::max(o, 0.f);
      y[(size_t)r * C + c] = f2bf(o);
    }
  }
  return DIG_OK;
}

int dig_bn_update_running(const float* sums, float n_total, float momentum, float* running_mean, float* running_var, int C, hipStream_t) {
  if (int rc = dig_rules::bn_update_running(sums, n_total, momentum, running_mean, running_var, C)) return rc;
  for (int c = 0; c < C; ++c) {
    const float mu = sums[c] / n_total;
    const float var = std::max(sums[C + c] / n_total - mu * mu, 0.f);
    running_mean[c] = running_mean[c] * (1.f - momentum) + mu * momentum;
    running_var[c] = running_var[c] * (1.f - momentum) + var * (n_total / (n_total - 1.f)) * momentum;
  }
  return DIG_OK;
}


int dig_bn_fwd_fused(const void* x_, float eps, const float* gamma, const float* beta, int relu, void* y_, float* mean_out, float* rstd_out,
                     float momentum, float* running_mean, float* running_var, int rows, int C, hipStream_t) {
  if (int rc = dig_rules::bn_fwd_fused(x_, eps, gamma, beta, relu, y_, mean_out, rstd_out, momentum, running_mean, running_var, rows, C)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
  bf16_t* y = (bf16_t*)y_;
  const float n = (float)rows, inv_n = 1.0f / n;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    float lane1[64], lane2[64];                                        // the device's row lanes: rows l, l + 64, ... summed per lane, lanes in order
    for (int l = 0; l < 64; ++l) {
      float a = 0.f, b = 0.f;
      for (int r = l; r < rows; r += 64) { const float v = bf2f(x[(size_t)r * C + c]); a += v; b += v * v; }
      lane1[l] = a; lane2[l] = b;
    }
    float s1 = 0.f, s2 = 0.f;
    for (int l = 0; l < 64; ++l) { s1 += lane1[l]; s2 += lane2[l]; }
    const float mu = s1 * inv_n, var = std::max(s2 * inv_n - mu * mu, 0.f), rs = 1.0f / std::sqrt(var + eps);
    mean_out[c] = mu; rstd_out[c] = rs;
    if (running_mean) {
      const float mr = s1 / n, vr = std::max(s2 / n - mr * mr, 0.f);
      running_mean[c] = running_mean[c] * (1.f - momentum) + mr * momentum;
      running_var[c] = running_var[c] * (1.f - momentum) + vr * (n / (n - 1.f)) * momentum;
    }
    for (int r = 0; r < rows; ++r) {
      float o = (bf2f(x[(size_t)r * C + c]) - mu) * rs;
      if (gamma) o = o * gamma[c] + beta[c];
      if (relu) o = std::max(o, 0.f);
      y[(size_t)r * C + c] = f2bf(o);
    }
  }
  return DIG_OK;
}

int dig_bn_bwd_fused(const void* dy_, const void* x_, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                     float* dbeta_acc, float* dgamma_acc, void* dx_, int rows, int C, hipStream_t) {
  if (int rc = dig_rules::bn_bwd_fused(dy_, x_, mean, rstd, gamma, beta, relu, dbeta_acc, dgamma_acc, dx_, rows, C)) return rc;
  const bf16_t* dy = (const bf16_t*)dy_;
  const bf16_t* x = (const bf16_t*)x_;
  bf16_t* dx = (bf16_t*)dx_;
  const float inv_n = 1.0f / (float)rows;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    const float g0 = gamma ? gamma[c] : 1.f, b0 = gamma ? beta[c] : 0.f;
    float lane1[64], lane2[64];
    for (int l = 0; l < 64; ++l) {
      float a = 0.f, b = 0.f;
      for (int r = l; r < rows; r += 64) {
        const float xh = (bf2f(x[(size_t)r * C + c]) - mean[c]) * rstd[c];
        float d = bf2f(dy[(size_t)r * C + c]);
        if (relu && !(g0 * xh + b0 > 0.f)) d = 0.f;
        a += d; b += d * xh;
      }
      lane1[l] = a; lane2[l] = b;
    }
    float s1 = 0.f, s2 = 0.f;
    for (int l = 0; l < 64; ++l) { s1 += lane1[l]; s2 += lane2[l]; }
    if (dbeta_acc) { dbeta_acc[c] += s1; dgamma_acc[c] += s2; }
    s1 *= inv_n; s2 *= inv_n;
    for (int r = 0; r < rows; ++r) {
      const float xh = (bf2f(x[(size_t)r * C + c]) - mean[c]) * rstd[c];
      float g = bf2f(dy[(size_t)r * C + c]);
      if (relu && !(g0 * xh + b0 > 0.f)) g = 0.f;
      dx[(size_t)r * C + c] = f2bf(g0 * rstd[c] * (g - s1 - xh * s2));
    }
  }
  return DIG_OK;
}

int dig_bn_fwd_apply_running(const void* x, const float* sums, float n_total, float eps, const float* gamma, const float* beta, int relu, void* y,
                             float* mean_out, float* rstd_out, float momentum, float* running_mean, float* running_var, int rows, int C,
                             hipStream_t st) {
  if (int rc = dig_rules::bn_fwd_apply_running(x, sums, n_total, eps, gamma, beta, relu, y, mean_out, rstd_out, momentum, running_mean, running_var,
                                               rows, C))
    return rc;
  const int rc = dig_bn_fwd_apply(x, sums, n_total, eps, gamma, beta, relu, y, mean_out, rstd_out, rows, C, st);
  if (rc || !running_mean) return rc;
  return dig_bn_update_running(sums, n_total, momentum, running_mean, running_var, C, st);
}

int dig_bn_bwd_stats(const void* dy_, const void* x_, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                     float* sums, float* workspace, int rows, int C, hipStream_t) {
  if (int rc = dig_rules::bn_bwd_stats_acc(dy_, x_, mean, rstd, gamma, beta, relu, sums, nullptr, nullptr, workspace, rows, C)) return rc;
  const bf16_t* dy = (const bf16_t*)dy_;
  const bf16_t* x = (const bf16_t*)x_;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    const float g0 = gamma ? gamma[c] : 1.f, b0 = gamma ? beta[c] : 0.f;
    float a = 0.f, b = 0.f;
    for (int r = 0; r < rows; ++r) {
      const float xh = (bf2f(x[(size_t)r * C + c]) - mean[c]) * rstd[c];
      float d = bf2f(dy[(size_t)r * C + c]);
      if (relu && !(g0 * xh + b0 > 0.f)) d = 0.f;
      a += d;
      b += d * xh;
    }
    sums[c] = a;
    sums[C + c] = b;
  }
  return DIG_OK;
}

int dig_bn_bwd_stats_acc(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                         float* sums, float* dbeta_acc, float* dgamma_acc, float* workspace, int rows, int C, hipStream_t st) {
  if (int rc = dig_rules::bn_bwd_stats_acc(dy, x, mean, rstd, gamma, beta, relu, sums, dbeta_acc, dgamma_acc, workspace, rows, C)) return rc;
  const int rc = dig_bn_bwd_stats(dy, x, mean, rstd, gamma, beta, relu, sums, workspace, rows, C, st);
  if (rc || !dbeta_acc) return rc;
  for (int c = 0; c < C; ++c) { dbeta_acc[c] += sums[c]; dgamma_acc[c] += sums[C + c]; }
  return DIG_OK;
}

int dig_bn_bwd_apply(const void* dy_, const void* x_, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                     const float* sums, float n_total, void* dx_, int rows, int C, hipStream_t) {
  if (int rc = dig_rules::bn_bwd_apply(dy_, x_, mean, rstd, gamma, beta, relu, sums, n_total, dx_, rows, C)) return rc;
  const bf16_t* dy = (const bf16_t*)dy_;
  const bf16_t* x = (const bf16_t*)x_;
  bf16_t* dx = (bf16_t*)dx_;
  const float inv_n = 1.0f / n_total;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    const float g0 = gamma ? gamma[c] : 1.f, b0 = gamma ? beta[c] : 0.f;
    const float s1 = sums[c] * inv_n, s2 = sums[C + c] * inv_n;
    for (int r = 0; r < rows; ++r) {
      const float xh = (bf2f(x[(size_t)r * C + c]) - mean[c]) * rstd[c];
      float g = bf2f(dy[(size_t)r * C + c]);
      if (relu && !(g0 * xh + b0 > 0.f)) g = 0.f;
      dx[(size_t)r * C + c] = f2bf(g0 * rstd[c] * (g - s1 - xh * s2));
    }
  }
  return DIG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ patch embedding
int dig_patch_embed_fwd(const float* img, const float* W, const float* bias, const unsigned char* mask, const float* mask_token,
                        const float* pos, void* out_, int n_img, int gh, int gw, int D, hipStream_t) {
  if (int rc = dig_rules::patch_embed_fwd(img, W, bias, mask, mask_token, pos, out_, n_img, gh, gw, D)) return rc;
  bf16_t* out = (bf16_t*)out_;
  const int ntok = gh * gw, Himg = gh * 4, Wimg = gw * 4;
#pragma omp parallel for
  for (int t = 0; t < n_img * ntok; ++t) {
    const int b = t / ntok, n = t % ntok, ph = n / gw, pw = n % gw;
    float patch[48];
    for (int k = 0; k < 48; ++k) {
      const int c = k >> 4, p1 = (k >> 2) & 3, p2 = k & 3;
      patch[k] = img[(((size_t)b * 3 + c) * Himg + ph * 4 + p1) * Wimg + pw * 4 + p2];
    }
    const bool m = mask && mask[t];
    for (int d = 0; d < D; ++d) {
      float acc = bias[d];
      for (int k = 0; k < 48; ++k) acc += patch[k] * W[d * 48 + k];
      out[(size_t)t * D + d] = f2bf((m ? mask_token[d] : acc) + pos[(size_t)n * D + d]);
    }
  }
  return DIG_OK;
}

int dig_patch_embed_bwd(const void* dy_, const float* img, const unsigned char* mask, float* dW, float* dbias, float* dmask_token, int n_img,
                        int gh, int gw, int D, hipStream_t) {
  if (int rc = dig_rules::patch_embed_bwd(dy_, img, mask, dW, dbias, dmask_token, n_img, gh, gw, D)) return rc;
  const bf16_t* dy = (const bf16_t*)dy_;
  const int ntok = gh * gw, Himg = gh * 4, Wimg = gw * 4;
#pragma omp parallel for
  for (int d = 0; d < D; ++d) {
    float acc[48], ab = 0.f, am = 0.f;
    for (int k = 0; k < 48; ++k) acc[k] = 0.f;
    for (int t = 0; t < n_img * ntok; ++t) {
      const float g = bf2f(dy[(size_t)t * D + d]);
      if (mask && mask[t]) { am += g; continue; }
      ab += g;
      const int b = t / ntok, n = t % ntok, ph = n / gw, pw = n % gw;
      for (int k = 0; k < 48; ++k) {
        const int c = k >> 4, p1 = (k >> 2) & 3, p2 = k & 3;
        acc[k] += g * img[(((size_t)b * 3 + c) * Himg + ph * 4 + p1) * Wimg + pw * 4 + p2];
      }
    }
    for (int k = 0; k < 48; ++k) dW[d * 48 + k] += acc[k];
    dbias[d] += ab;
    dmask_token[d] += am;
  }
  return DIG_OK;
}

int dig_patchify_bf16(const float* img, const unsigned char* mask, void* out_, int n_img, int gh, int gw, hipStream_t) {
  if (int rc = dig_rules::patchify_bf16(img, mask, out_, n_img, gh, gw)) return rc;
  bf16_t* out = (bf16_t*)out_;
  const int ntok = gh * gw, Himg = gh * 4, Wimg = gw * 4;
#pragma omp parallel for
  for (int t = 0; t < n_img * ntok; ++t) {
    const int b = t / ntok, n = t % ntok, ph = n / gw, pw = n % gw;
    const bool m = mask && mask[t];
    for (int k = 0; k < 64; ++k) {
      float v = 0.f;
      if (k < 48 && !m) {
        const int c = k >> 4, p1 = (k >> 2) & 3, p2 = k & 3;
        v = img[(((size_t)b * 3 + c) * Himg + ph * 4 + p1) * Wimg + pw * 4 + p2];
      }
      out[(size_t)t * 64 + k] = f2bf(v);
    }
  }
  return DIG_OK;
}

long long dig_colsum_workspace_bytes(int rows, int C) { return (long long)((rows + 63) / 64) * C * sizeof(float); }

int dig_colsum_masked(const void* x_, const unsigned char* mask, float* out_unmasked, float* out_masked, float* workspace, int rows, int C,
                      hipStream_t) {
  if (int rc = dig_rules::colsum_masked(x_, mask, out_unmasked, out_masked, workspace, rows, C)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < rows; ++r) (mask[r] ? b : a) += bf2f(x[(size_t)r * C + c]);
    out_unmasked[c] += a;
    out_masked[c] += b;
  }
  return DIG_OK;
}

// adaptive_avg_pool2d's bins: [floor(win gw / nwin), ceil((win + 1) gw / nwin)) (equal windows when nwin divides gw)
static inline void pool_window(int win, int gw, int nwin, int& c_lo, int& wlen) {
  c_lo = (win * gw) / nwin;
  wlen = ((win + 1) * gw + nwin - 1) / nwin - c_lo;
}

int dig_window_pool_fwd(const void* x_, void* out, int out_is_f32, int n_img, int gh, int gw, int nwin, int D, hipStream_t) {
  if (int rc = dig_rules::window_pool_fwd(x_, out, out_is_f32, n_img, gh, gw, nwin, D)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
#pragma omp parallel for
  for (int idx = 0; idx < n_img * nwin; ++idx) {
    const int img = idx / nwin, win = idx % nwin;
    int c_lo, wlen;
    pool_window(win, gw, nwin, c_lo, wlen);
    const float inv = 1.0f / (gh * wlen);
    for (int d = 0; d < D; ++d) {
      float a = 0.f;
      for (int r = 0; r < gh; ++r)
        for (int c = 0; c < wlen; ++c) a += bf2f(x[((size_t)img * gh * gw + r * gw + c_lo + c) * D + d]);
      if (out_is_f32) ((float*)out)[(size_t)idx * D + d] = a * inv;
      else ((bf16_t*)out)[(size_t)idx * D + d] = f2bf(a * inv);
    }
  }
  return DIG_OK;
}

int dig_window_pool_bwd(const void* dpool_, void* dx_, int n_img, int gh, int gw, int nwin, int D, int accumulate, hipStream_t) {
  if (int rc = dig_rules::window_pool_bwd(dpool_, dx_, n_img, gh, gw, nwin, D, accumulate)) return rc;
  const bf16_t* dpool = (const bf16_t*)dpool_;
  bf16_t* dx = (bf16_t*)dx_;
  const int ntok = gh * gw;
#pragma omp parallel for
  for (int t = 0; t < n_img * ntok; ++t) {
    const int img = t / ntok, n = t % ntok, col = n % gw, w0 = (col * nwin) / gw;
    for (int d = 0; d < D; ++d) {
      float a = 0.f;
      for (int win = std::max(0, w0 - 1); win <= std::min(nwin - 1, ((col + 1) * nwin + gw - 1) / gw - 1); ++win) {
        int c_lo, wlen;
        pool_window(win, gw, nwin, c_lo, wlen);
        if (col < c_lo || col >= c_lo + wlen) continue;
        a += bf2f(dpool[((size_t)img * nwin + win) * D + d]) * (1.0f / (gh * wlen));
      }
      if (accumulate) a += bf2f(dx[(size_t)t * D + d]);
      dx[(size_t)t * D + d] = f2bf(a);
    }
  }
  return DIG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ ConvPatchNet data movement
int dig_im2col3x3(const void* x_, void* col_, int n_img, int H, int W, int C, int ldc, hipStream_t) {
  if (int rc = dig_rules::im2col3x3(x_, col_, n_img, H, W, C, ldc)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
  bf16_t* col = (bf16_t*)col_;
  const long rows = (long)n_img * H * W;
#pragma omp parallel for
  for (long r = 0; r < rows; ++r) {
    const int xx = (int)(r % W), yy = (int)((r / W) % H);
    bf16_t* o = col + (size_t)r * ldc;
    for (int t = 0; t < 9; ++t) {
      const int y2 = yy + t / 3 - 1, x2 = xx + t % 3 - 1;
      const bool in = y2 >= 0 && y2 < H && x2 >= 0 && x2 < W;
      const bf16_t* s = x + ((long)r + (long)(t / 3 - 1) * W + (t % 3 - 1)) * (long)C;
      for (int c = 0; c < C; ++c) o[c * 9 + t] = in ? s[c] : (bf16_t)0;
    }
    for (int c = 9 * C; c < ldc; ++c) o[c] = 0;
  }
  return DIG_OK;
}

int dig_conv3x3_weight_flip(const void* w_, void* wt_, int c_out, int c_in, hipStream_t) {
  if (int rc = dig_rules::conv3x3_weight_flip(w_, wt_, c_out, c_in)) return rc;
  const bf16_t* w = (const bf16_t*)w_;
  bf16_t* wt = (bf16_t*)wt_;
  for (int co = 0; co < c_out; ++co)
    for (int ci = 0; ci < c_in; ++ci)
      for (int t = 0; t < 9; ++t) wt[((size_t)ci * c_out + co) * 9 + t] = w[((size_t)co * c_in + ci) * 9 + 8 - t];
  return DIG_OK;
}

int dig_maxpool2x2_fwd(const void* x_, void* y_, unsigned char* idx, int n_img, int H, int W, int C, hipStream_t) {
  if (int rc = dig_rules::maxpool2x2_fwd(x_, y_, idx, n_img, H, W, C)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
  bf16_t* y = (bf16_t*)y_;
  const int Ho = H / 2, Wo = W / 2;
#pragma omp parallel for
  for (long ro = 0; ro < (long)n_img * Ho * Wo; ++ro) {
    const int xo = (int)(ro % Wo), yo = (int)((ro / Wo) % Ho);
    const long b = ro / ((long)Wo * Ho);
    const bf16_t* p = x + ((b * H + 2 * yo) * W + 2 * xo) * (size_t)C;
    for (int c = 0; c < C; ++c) {
      bf16_t m = p[c];
      unsigned char am = 0;
      for (int t = 1; t < 4; ++t) {
        const bf16_t v = p[((size_t)(t >> 1) * W + (t & 1)) * C + c];
        const float fv = bf2f(v), fm = bf2f(m);
        if (fv > fm || fv != fv) { m = v; am = (unsigned char)t; }
      }
      y[(size_t)ro * C + c] = m;
      idx[(size_t)ro * C + c] = am;
    }
  }
  return DIG_OK;
}

int dig_maxpool2x2_bwd(const void* dy_, const unsigned char* idx, void* dx_, int n_img, int H, int W, int C, hipStream_t) {
  if (int rc = dig_rules::maxpool2x2_bwd(dy_, idx, dx_, n_img, H, W, C)) return rc;
  const bf16_t* dy = (const bf16_t*)dy_;
  bf16_t* dx = (bf16_t*)dx_;
  const int Ho = H / 2, Wo = W / 2;
#pragma omp parallel for
  for (long ro = 0; ro < (long)n_img * Ho * Wo; ++ro) {
    const int xo = (int)(ro % Wo), yo = (int)((ro / Wo) % Ho);
    const long b = ro / ((long)Wo * Ho);
    bf16_t* p = dx + ((b * H + 2 * yo) * W + 2 * xo) * (size_t)C;
    for (int c = 0; c < C; ++c)
      for (int t = 0; t < 4; ++t) p[((size_t)(t >> 1) * W + (t & 1)) * C + c] = idx[(size_t)ro * C + c] == t ? dy[(size_t)ro * C + c] : (bf16_t)0;
  }
  return DIG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ SimMIM plumbing
}  // extern "C"
template <typename T>
static void mask_views_u8_host(const T* mask, unsigned char* out, int B, int V, int N, int keep_views) {
  for (int v = 0; v < V; ++v)
    for (int b = 0; b < B; ++b)
      for (int n = 0; n < N; ++n) out[((size_t)v * B + b) * N + n] = (v < keep_views && mask[((size_t)b * V + v) * N + n] != (T)0) ? 1 : 0;
}
extern "C" {
int dig_mask_views_u8(const void* mask, int elem_kind, int B, int V, int N, int keep_views, unsigned char* out, hipStream_t) {
  if (int rc = dig_rules::mask_views_u8(mask, elem_kind, B, V, N, keep_views, out)) return rc;
  switch (elem_kind) {
    case 0: mask_views_u8_host((const unsigned char*)mask, out, B, V, N, keep_views); break;
    case 1: mask_views_u8_host((const float*)mask, out, B, V, N, keep_views); break;
    case 2: mask_views_u8_host((const double*)mask, out, B, V, N, keep_views); break;
    case 3: mask_views_u8_host((const int*)mask, out, B, V, N, keep_views); break;
    case 4: mask_views_u8_host((const long long*)mask, out, B, V, N, keep_views); break;
    default: break;                                                        // (the rule admits kinds 0..4 only)
  }
  return DIG_OK;
}
int dig_mask_to_index(const unsigned char* mask, int* idx, int* count, int B, int N, int max_per_sample, hipStream_t) {
  if (int rc = dig_rules::mask_to_index(mask, idx, count, B, N, max_per_sample)) return rc;
  for (int b = 0; b < B; ++b) {
    int k = 0;
    for (int n = 0; n < N; ++n)
      if (mask[(size_t)b * N + n]) {
        if (k < max_per_sample) idx[(size_t)b * max_per_sample + k] = b * N + n;
        ++k;
      }
    count[b] = k;
  }
  return DIG_OK;
}

int dig_gather_rows(const void* src_, const int* idx, void* dst_, int M, int M_pad, int D, hipStream_t) {
  if (int rc = dig_rules::gather_rows(src_, idx, dst_, M, M_pad, D)) return rc;
  const bf16_t* src = (const bf16_t*)src_;
  bf16_t* dst = (bf16_t*)dst_;
  for (int m = 0; m < M_pad; ++m) {
    if (m < M) std::memcpy(dst + (size_t)m * D, src + (size_t)idx[m] * D, D * 2);
    else std::memset(dst + (size_t)m * D, 0, D * 2);
  }
  return DIG_OK;
}

int dig_scatter_rows_add(const void* src_, const int* idx, void* dst_, int M, int D, hipStream_t) {
  if (int rc = dig_rules::scatter_rows_add(src_, idx, dst_, M, D)) return rc;
  const bf16_t* src = (const bf16_t*)src_;
  bf16_t* dst = (bf16_t*)dst_;
  for (int m = 0; m < M; ++m)
    for (int c = 0; c < D; ++c) dst[(size_t)idx[m] * D + c] = f2bf(bf2f(dst[(size_t)idx[m] * D + c]) + bf2f(src[(size_t)m * D + c]));
  return DIG_OK;
}

int dig_mim_target(const float* img, const int* idx, float* target, int M, int gh, int gw, int normalize, hipStream_t) {
  if (int rc = dig_rules::mim_target(img, idx, target, M, gh, gw, normalize)) return rc;
  const int ntok = gh * gw, Himg = gh * 4, Wimg = gw * 4;
  for (int m = 0; m < M; ++m) {
    const int t = idx[m], b = t / ntok, n = t % ntok, ph = n / gw, pw = n % gw;
    for (int c = 0; c < 3; ++c) {
      const float* base = img + (((size_t)b * 3 + c) * Himg + ph * 4) * Wimg + pw * 4;
      float v[16], mean = 0.f;
      for (int q = 0; q < 16; ++q) { v[q] = base[(q >> 2) * Wimg + (q & 3)] * 0.5f + 0.5f; mean += v[q]; }
      mean *= (1.0f / 16.0f);
      float var = 0.f;
      for (int q = 0; q < 16; ++q) var += (v[q] - mean) * (v[q] - mean);
      const float sd = std::sqrt(var * (1.0f / 15.0f)) + 1e-6f;
      for (int q = 0; q < 16; ++q) target[(size_t)m * 48 + q * 3 + c] = normalize ? (v[q] - mean) / sd : v[q];
    }
  }
  return DIG_OK;
}

int dig_mse_fwd_bwd(const float* pred, int ld_pred, const float* target, int M, int C, float gscale, float* loss, void* dpred_, int ld_dpred, hipStream_t);
int dig_mse_fwd_bwd_ws(const float* pred, int ld_pred, const float* target, int M, int C, float gscale, float* loss, void* dpred, int ld_dpred,
                       float*, hipStream_t st) {
  return dig_mse_fwd_bwd(pred, ld_pred, target, M, C, gscale, loss, dpred, ld_dpred, st);
}
int dig_mse_fwd_bwd(const float* pred, int ld_pred, const float* target, int M, int C, float gscale, float* loss, void* dpred_, int ld_dpred,
                    hipStream_t) {
  if (int rc = dig_rules::mse_fwd_bwd_ws(pred, ld_pred, target, M, C, gscale, loss, dpred_, ld_dpred, nullptr)) return rc;
  bf16_t* dpred = (bf16_t*)dpred_;
  const float inv = 1.0f / ((float)M * (float)C);
  double acc = 0.0;
  for (int m = 0; m < M; ++m)
    for (int c = 0; c < (dpred ? ld_dpred : C); ++c) {
      float g = 0.f;
      if (c < C) {
        const float df = pred[(size_t)m * ld_pred + c] - target[(size_t)m * C + c];
        acc += (double)df * df;
        g = 2.f * df * inv * gscale;
      }
      if (dpred) dpred[(size_t)m * ld_dpred + c] = f2bf(g);
    }
  if (loss) loss[0] += (float)(acc * inv);
  return DIG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ InfoNCE
int dig_l2norm_fwd(const float* x, float* y, float* inv_norm, int n, int C, float eps, hipStream_t) {
  if (int rc = dig_rules::l2norm_fwd(x, y, inv_norm, n, C, eps)) return rc;
  for (int r = 0; r < n; ++r) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += x[(size_t)r * C + c] * x[(size_t)r * C + c];
    const float inv = 1.0f / std::max(std::sqrt(s), eps);
    for (int c = 0; c < C; ++c) y[(size_t)r * C + c] = x[(size_t)r * C + c] * inv;
    inv_norm[r] = inv;
  }
  return DIG_OK;
}

int dig_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int n, int C, hipStream_t) {
  if (int rc = dig_rules::l2norm_bwd(dy, y, inv_norm, dx, n, C)) return rc;
  for (int r = 0; r < n; ++r) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += y[(size_t)r * C + c] * dy[(size_t)r * C + c];
    for (int c = 0; c < C; ++c) dx[(size_t)r * C + c] = (dy[(size_t)r * C + c] - y[(size_t)r * C + c] * s) * inv_norm[r];
  }
  return DIG_OK;
}

int dig_sgemm(const float* A, const float* B, float* C, int I, int J, int R, int lda, int ldb, int ldc, int trans_b, float alpha,
              int r_splits, hipStream_t) {
  if (int rc = dig_rules::sgemm(A, B, C, I, J, R, lda, ldb, ldc, trans_b, alpha, r_splits)) return rc;
  const int per = ((R + r_splits - 1) / r_splits + 63) / 64 * 64;
#pragma omp parallel for collapse(2)
  for (int s = 0; s < r_splits; ++s)
    for (int i = 0; i < I; ++i)
      for (int j = 0; j < J; ++j) {
        float acc = 0.f;
        for (int r = s * per; r < std::min(R, (s + 1) * per); ++r) acc += A[(size_t)i * lda + r] * (trans_b ? B[(size_t)r * ldb + j] : B[(size_t)j * ldb + r]);
        C[((size_t)s * I + i) * ldc + j] = alpha * acc;
      }
  return DIG_OK;
}

int dig_ce_rows(float* logits, int n, int m, int label_offset, float gscale, float* out3, hipStream_t);
int dig_ce_rows_ws(float* logits, int n, int m, int label_offset, float gscale, float* out3, float*, hipStream_t st) {
  return dig_ce_rows(logits, n, m, label_offset, gscale, out3, st);         // (the host build sums in row order anyway)
}
int dig_infonce_finish(const float* stats6, float loss_scale, float acc_scale, float* contra, float* accs4, hipStream_t) {
  if (int rc = dig_rules::infonce_finish(stats6, loss_scale, acc_scale, contra, accs4)) return rc;
  contra[0] = (stats6[0] + stats6[3]) * loss_scale;
  for (int k = 0; k < 4; ++k) accs4[k] = stats6[(k >> 1) * 3 + 1 + (k & 1)] * acc_scale;
  return DIG_OK;
}
int dig_step_meters(const float* loss, const float* contra, const float* pixel, const float* accs4, const int* counts, int n_counts,
                    const float* grad_norm, float* out10, hipStream_t) {
  if (int rc = dig_rules::step_meters(loss, contra, pixel, accs4, counts, n_counts, grad_norm, out10)) return rc;
  int lo = counts[0], hi = counts[0];
  for (int i = 1; i < n_counts; ++i) { lo = std::min(lo, counts[i]); hi = std::max(hi, counts[i]); }
  out10[0] = loss[0]; out10[1] = contra[0]; out10[2] = pixel[0];
  for (int k = 0; k < 4; ++k) out10[3 + k] = accs4[k];
  out10[7] = (float)lo; out10[8] = (float)hi; out10[9] = grad_norm ? grad_norm[0] : NAN;
  return DIG_OK;
}
int dig_ce_rows(float* logits, int n, int m, int label_offset, float gscale, float* out3, hipStream_t) {
  if (int rc = dig_rules::ce_rows_ws(logits, n, m, label_offset, gscale, out3, nullptr)) return rc;
  for (int i = 0; i < n; ++i) {
    float* row = logits + (size_t)i * m;
    const int label = i + label_offset;
    float mx = -3.0e38f;
    for (int j = 0; j < m; ++j) mx = std::max(mx, row[j]);
    const float zl = row[label];
    float s = 0.f;
    int gt = 0;
    for (int j = 0; j < m; ++j) { s += std::exp(row[j] - mx); gt += row[j] > zl; }
    const float lse = mx + std::log(s);
    for (int j = 0; j < m; ++j) row[j] = gscale * (std::exp(row[j] - mx) / s - (j == label ? 1.f : 0.f));
    out3[0] += lse - zl;
    if (gt < 1) out3[1] += 1.f;
    if (gt < 5) out3[2] += 1.f;
  }
  return DIG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ optimizer
static int adamw_core(float* p, const float* g, float* m, float* v, bf16_t* shadow, long long n, const unsigned char* group, float lr0,
                      float wd0, float lr1, float wd1, float beta1, float beta2, float eps, float inv_bc1, float inv_sqrt_bc2,
                      float grad_scale, const float* finite_gate) {
  if (finite_gate && !std::isfinite(finite_gate[0])) return DIG_OK;
#pragma omp parallel for
  for (long long i = 0; i < n; ++i) {
    const int grp = group[i >> 8] & 0x7f;                                // (bit 7: a weight of dig_adamw_step_tr's table -- same update)
    if (grp == 2) {                                                      // a parameter without a gradient: untouched
      if (shadow) shadow[i] = f2bf(p[i]);
      continue;
    }
    const float lr = grp ? lr1 : lr0, wd = grp ? wd1 : wd0;
    const float gk = g[i] * grad_scale;
    float P = p[i] * (1.0f - lr * wd);
    const float M = m[i] * beta1 + gk * (1.0f - beta1);
    const float V = v[i] * beta2 + gk * gk * (1.0f - beta2);
    P -= (lr * inv_bc1) * (M / (std::sqrt(V) * inv_sqrt_bc2 + eps));
    p[i] = P; m[i] = M; v[i] = V;
    if (shadow) shadow[i] = f2bf(P);
  }
  return DIG_OK;
}

int dig_adamw_bias_corrections(float beta1, float beta2, int step, float* out2) {
  if (int rc = dig_rules::adamw_bias_corrections(beta1, beta2, step, out2)) return rc;
  out2[0] = (float)(1.0 / (1.0 - std::pow((double)beta1, (double)step)));
  out2[1] = (float)(1.0 / std::sqrt(1.0 - std::pow((double)beta2, (double)step)));
  return DIG_OK;
}

struct AdamTrMat { long long off, dst_off; int rows, cols, tile0, pad; };

int dig_adamw_step_tr(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_flags, float lr0,
                      float wd0, float lr1, float wd1, float beta1, float beta2, float eps, int step, float grad_scale, const float* finite_gate,
                      const void* mats, int n_mats, int n_tiles, void* tr_out, hipStream_t) {
  if (int rc = dig_rules::adamw_step_tr(p, g, m, v, bf16_shadow, n, group_flags, lr0, wd0, lr1, wd1, beta1, beta2, eps, step, grad_scale,
                                        finite_gate, mats, n_mats, n_tiles, tr_out))
    return rc;
  if (finite_gate && !std::isfinite(finite_gate[0])) return DIG_OK;
  float bc[2];
  dig_adamw_bias_corrections(beta1, beta2, step, bc);
  const int rc = adamw_core(p, g, m, v, (bf16_t*)bf16_shadow, n, group_flags, lr0, wd0, lr1, wd1, beta1, beta2, eps, bc[0], bc[1], grad_scale, finite_gate);
  if (rc != DIG_OK) return rc;
  const AdamTrMat* mt = (const AdamTrMat*)mats;
  bf16_t* out = (bf16_t*)tr_out;
  for (int k = 0; k < n_mats; ++k)
    for (int r = 0; r < mt[k].rows; ++r)
      for (int c = 0; c < mt[k].cols; ++c) out[mt[k].dst_off + (long long)c * mt[k].rows + r] = f2bf(p[mt[k].off + (long long)r * mt[k].cols + c]);
  return DIG_OK;
}

int dig_adamw_step(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_flags, float lr0,
                   float wd0, float lr1, float wd1, float beta1, float beta2, float eps, int step, float grad_scale, const float* finite_gate,
                   hipStream_t) {
  if (int rc = dig_rules::adamw_step(p, g, m, v, bf16_shadow, n, group_flags, lr0, wd0, lr1, wd1, beta1, beta2, eps, step, grad_scale, finite_gate))
    return rc;
  float bc[2];
  dig_adamw_bias_corrections(beta1, beta2, step, bc);
  return adamw_core(p, g, m, v, (bf16_t*)bf16_shadow, n, group_flags, lr0, wd0, lr1, wd1, beta1, beta2, eps, bc[0], bc[1], grad_scale, finite_gate);
}

int dig_adamw_step_dev(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_flags,
                       const float* s6, float beta1, float beta2, float eps, float grad_scale, const float* finite_gate, hipStream_t) {
  if (int rc = dig_rules::adamw_step_dev(p, g, m, v, bf16_shadow, n, group_flags, s6, beta1, beta2, eps, grad_scale, finite_gate)) return rc;
  return adamw_core(p, g, m, v, (bf16_t*)bf16_shadow, n, group_flags, s6[0], s6[1], s6[2], s6[3], beta1, beta2, eps, s6[4], s6[5], grad_scale, finite_gate);
}

// any number of parameter groups (layer-wise lr decay): group_idx per 256-element granule indexes lr_tab / wd_tab; 255 = no gradient
int dig_adamw_step_groups(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_idx,
                          const float* lr_tab, const float* wd_tab, float beta1, float beta2, float eps, int step, float grad_scale,
                          const float* finite_gate, hipStream_t) {
  if (int rc = dig_rules::adamw_step_groups(p, g, m, v, bf16_shadow, n, group_idx, lr_tab, wd_tab, beta1, beta2, eps, step, grad_scale, finite_gate))
    return rc;
  if (finite_gate && !std::isfinite(finite_gate[0])) return DIG_OK;
  float bc[2];
  dig_adamw_bias_corrections(beta1, beta2, step, bc);
  bf16_t* shadow = (bf16_t*)bf16_shadow;
#pragma omp parallel for
  for (long long i = 0; i < n; ++i) {
    const int grp = group_idx[i >> 8];
    if (grp != 255) {
      const float lr = lr_tab[grp], wd = wd_tab[grp], gk = g[i] * grad_scale;
      float P = p[i] * (1.0f - lr * wd);
      const float M = m[i] * beta1 + gk * (1.0f - beta1);
      const float V = v[i] * beta2 + gk * gk * (1.0f - beta2);
      P -= (lr * bc[0]) * (M / (std::sqrt(V) * bc[1] + eps));
      p[i] = P; m[i] = M; v[i] = V;
    }
    if (shadow) shadow[i] = f2bf(p[i]);
  }
  return DIG_OK;
}

static int ema_core(float* pm, const float* p, bf16_t* shadow, long long n, float m, float om) {
#pragma omp parallel for
  for (long long i = 0; i < n; ++i) {
    pm[i] = pm[i] * m + p[i] * om;
    if (shadow) shadow[i] = f2bf(pm[i]);
  }
  return DIG_OK;
}
int dig_ema_update(float* pm, const float* p, void* bf16_shadow, long long n, float m, hipStream_t) {
  if (int rc = dig_rules::ema_update(pm, p, bf16_shadow, n, m)) return rc;
  return ema_core(pm, p, (bf16_t*)bf16_shadow, n, m, (float)(1.0 - (double)m));
}
int dig_ema_update_dev(float* pm, const float* p, void* bf16_shadow, long long n, const float* mm, hipStream_t) {
  if (int rc = dig_rules::ema_update_dev(pm, p, bf16_shadow, n, mm)) return rc;
  return ema_core(pm, p, (bf16_t*)bf16_shadow, n, mm[0], mm[1]);
}

int dig_sumsq(const float* x, long long n, float* workspace, float* out, hipStream_t) {
  if (int rc = dig_rules::sumsq(x, n, workspace, out)) return rc;
  double acc = 0.0;
  for (long long i = 0; i < n; ++i) acc += (double)x[i] * x[i];
  out[0] = (float)acc;
  return DIG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ helpers
int dig_colsum(const void* x_, float* out, float* workspace, int rows, int C, int ld, hipStream_t) {
  if (int rc = dig_rules::colsum(x_, out, workspace, rows, C, ld)) return rc;
  const bf16_t* x = (const bf16_t*)x_;
#pragma omp parallel for
  for (int c = 0; c < C; ++c) {
    float a = 0.f;
    for (int r = 0; r < rows; ++r) a += bf2f(x[(size_t)r * ld + c]);
    out[c] += a;
  }
  return DIG_OK;
}

int dig_colsum_partials(const float* partials, int n_parts, int C, float* out, hipStream_t) {
  if (int rc = dig_rules::colsum_partials(partials, n_parts, C, out)) return rc;
  for (int c = 0; c < C; ++c) {
    float a = 0.f;
    for (int b = 0; b < n_parts; ++b) a += partials[(size_t)b * C + c];
    out[c] += a;
  }
  return DIG_OK;
}

// ---- fused MLP chain (include/dig_hip.h; csrc/mlp_chain.hip): the same arithmetic as plain loops -- fp32 accumulation, the hidden
// values rounded to bf16 between the two layers, bias and residual added in fp32 before the final rounding
// drop (or null): out = resid + drop_path(dropout(fc2(.) + b2)), the mask rule of dig_gemm_bf16_dropout (element index r * D + j)
static int chain_fwd_cpu(const void* x_, const void* w1_, const float* b1, const void* w2_, const float* b2, const void* resid_, void* out_,
                         void* pre_out_, void* act_out_, int R, int D, int F, const dig_dropout_t* drop) {
  const bf16_t* x = (const bf16_t*)x_; const bf16_t* w1 = (const bf16_t*)w1_; const bf16_t* w2 = (const bf16_t*)w2_;
  const bf16_t* resid = (const bf16_t*)resid_;
  bf16_t* out = (bf16_t*)out_; bf16_t* pre_out = (bf16_t*)pre_out_; bf16_t* act_out = (bf16_t*)act_out_;
  std::vector<float> W1((size_t)F * D), W2((size_t)D * F);
  for (size_t i = 0; i < W1.size(); ++i) { W1[i] = bf2f(w1[i]); W2[i] = bf2f(w2[i]); }
#pragma omp parallel
  {
    std::vector<float> xr(D), h(F);
#pragma omp for
    for (int r = 0; r < R; ++r) {
      for (int k = 0; k < D; ++k) xr[k] = bf2f(x[(size_t)r * D + k]);
      for (int f = 0; f < F; ++f) {
        float a = b1 ? b1[f] : 0.f;
        const float* w = &W1[(size_t)f * D];
        for (int k = 0; k < D; ++k) a += w[k] * xr[k];
        if (pre_out) pre_out[(size_t)r * F + f] = f2bf(a);
        const bf16_t g = f2bf(gelu_f(a));
        if (act_out) act_out[(size_t)r * F + f] = g;
        h[f] = bf2f(g);
      }
      for (int j = 0; j < D; ++j) {
        float a = (b2 ? b2[j] : 0.f) + ((resid && !drop) ? bf2f(resid[(size_t)r * D + j]) : 0.f);
        const float* w = &W2[(size_t)j * F];
        for (int f = 0; f < F; ++f) a += w[f] * h[f];
        if (drop) a = drop_apply(a, *drop, r, j, D) + (resid ? bf2f(resid[(size_t)r * D + j]) : 0.f);
        out[(size_t)r * D + j] = f2bf(a);
      }
    }
  }
  return DIG_OK;
}

int dig_mlp_chain_fwd(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, const void* resid, void* out,
                      void* pre_out, void* act_out, int R, int D, int F, hipStream_t) {
  if (int rc = dig_rules::mlp_chain_fwd(x, w1, b1, w2, b2, resid, out, pre_out, act_out, R, D, F)) return rc;
  return chain_fwd_cpu(x, w1, b1, w2, b2, resid, out, pre_out, act_out, R, D, F, nullptr);
}

// rows of y = LN(x): fp32 statistics over the bf16 values, variance as E[x^2] - E[x]^2 (what the fused kernel computes)
static void ln_rows_cpu(const bf16_t* x, const float* g, const float* b, float eps, bf16_t* y, float* mean, float* rstd, int R, int D) {
#pragma omp parallel for
  for (int r = 0; r < R; ++r) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < D; ++k) { const float v = bf2f(x[(size_t)r * D + k]); s1 += v; s2 += v * v; }
    const float mu = s1 / D;
    const float rs = 1.0f / std::sqrt(std::max(s2 / D - mu * mu, 0.f) + eps);
    if (y) for (int k = 0; k < D; ++k) y[(size_t)r * D + k] = f2bf((bf2f(x[(size_t)r * D + k]) - mu) * (rs * g[k]) + b[k]);
    if (mean) { mean[r] = mu; rstd[r] = rs; }
  }
}

int dig_mlp_chain_fwd_ln_dropout(const void* x, const void* resid, const float* ln_g, const float* ln_b, float eps, void* ln_out, float* ln_mean,
                                 float* ln_rstd, const void* w1, const float* b1, const void* w2, const float* b2, void* out, void* pre_out,
                                 void* act_out, const float* nln_g, const float* nln_b, void* nln_out, float* nln_mean, float* nln_rstd, int R, int D,
                                 int F, const dig_dropout_t* drop, hipStream_t st) {
  if (int rc = dig_rules::mlp_chain_fwd_ln_dropout(x, resid, ln_g, ln_b, eps, ln_out, ln_mean, ln_rstd, w1, b1, w2, b2, out, pre_out, act_out, nln_g,
                                                   nln_b, nln_out, nln_mean, nln_rstd, R, D, F, drop))
    return rc;
  if (drop && !(drop->thr || drop->pthr)) drop = nullptr;
  std::vector<bf16_t> tmp;
  const bf16_t* ln = (const bf16_t*)x;
  if (ln_g) {
    bf16_t* lnw = (bf16_t*)ln_out;
    if (!lnw) { tmp.resize((size_t)R * D + 8); lnw = (bf16_t*)(((uintptr_t)tmp.data() + 15) & ~(uintptr_t)15); }
    ln_rows_cpu((const bf16_t*)x, ln_g, ln_b, eps, lnw, ln_mean, ln_rstd, R, D);
    ln = lnw;
  }
  (void)st;
  const int rc = chain_fwd_cpu(ln, w1, b1, w2, b2, resid, out, pre_out, act_out, R, D, F, drop);
  if (rc != DIG_OK) return rc;
  if (nln_g) ln_rows_cpu((const bf16_t*)out, nln_g, nln_b, eps, (bf16_t*)nln_out, nln_mean, nln_rstd, R, D);
  return DIG_OK;
}

int dig_mlp_chain_fwd_ln(const void* x, const void* resid, const float* ln_g, const float* ln_b, float eps, void* ln_out, float* ln_mean,
                         float* ln_rstd, const void* w1, const float* b1, const void* w2, const float* b2, void* out, void* pre_out, void* act_out,
                         const float* nln_g, const float* nln_b, void* nln_out, float* nln_mean, float* nln_rstd, int R, int D, int F,
                         hipStream_t st) {
  return dig_mlp_chain_fwd_ln_dropout(x, resid, ln_g, ln_b, eps, ln_out, ln_mean, ln_rstd, w1, b1, w2, b2, out, pre_out, act_out, nln_g, nln_b, nln_out,
                                      nln_mean, nln_rstd, R, D, F, nullptr, st);
}

int dig_mlp_chain_bwd(const void* dy_, const void* w2t_, const void* pre_, const void* w1t_, void* dpre_out_, void* dx_out_,
                      float* colsum_partials, int R, int D, int F, hipStream_t) {
  if (int rc = dig_rules::mlp_chain_bwd(dy_, w2t_, pre_, w1t_, dpre_out_, dx_out_, colsum_partials, R, D, F)) return rc;
  const bf16_t* dy = (const bf16_t*)dy_; const bf16_t* w2t = (const bf16_t*)w2t_; const bf16_t* w1t = (const bf16_t*)w1t_;
  const bf16_t* pre = (const bf16_t*)pre_;
  bf16_t* dpre = (bf16_t*)dpre_out_; bf16_t* dx = (bf16_t*)dx_out_;
  std::vector<float> W2T((size_t)F * D), W1T((size_t)D * F);
  for (size_t i = 0; i < W2T.size(); ++i) { W2T[i] = bf2f(w2t[i]); W1T[i] = bf2f(w1t[i]); }
#pragma omp parallel
  {
    std::vector<float> yr(D), h(F);
#pragma omp for
    for (int r = 0; r < R; ++r) {
      for (int k = 0; k < D; ++k) yr[k] = bf2f(dy[(size_t)r * D + k]);
      for (int f = 0; f < F; ++f) {
        float a = 0.f;
        const float* w = &W2T[(size_t)f * D];
        for (int k = 0; k < D; ++k) a += w[k] * yr[k];
        const bf16_t g = f2bf(a * dgelu_f(bf2f(pre[(size_t)r * F + f])));
        dpre[(size_t)r * F + f] = g;
        h[f] = bf2f(g);
      }
      for (int j = 0; j < D; ++j) {
        float a = 0.f;
        const float* w = &W1T[(size_t)j * F];
        for (int f = 0; f < F; ++f) a += w[f] * h[f];
        dx[(size_t)r * D + j] = f2bf(a);
      }
    }
  }
  if (colsum_partials) {                                  // partial row p = 32-row block p (the rounded values, as the device sums them)
    const int np = dig_rules::mlp_chain_colsum_rows(R);
#pragma omp parallel for
    for (int pr = 0; pr < np; ++pr)
      for (int f = 0; f < F; ++f) {
        float a = 0.f;
        for (int r = pr * 32; r < std::min(R, pr * 32 + 32); ++r) a += bf2f(dpre[(size_t)r * F + f]);
        colsum_partials[(size_t)pr * F + f] = a;
      }
  }
  return DIG_OK;
}

// dig_mlp_chain_bwd, then norm2's backward on its result: partial row p = 128-row block p
int dig_mlp_chain_bwd_ln(const void* dy_, const void* w2t, const void* pre, const void* w1t, void* dpre_out, const void* x_mid_,
                         const float* ln_g, const float* ln_mean, const float* ln_rstd, void* dx_mid_out, float* colsum_partials,
                         float* ln_partials, int R, int D, int F, hipStream_t stream) {
  if (int rc = dig_rules::mlp_chain_bwd_ln_proj(dy_, w2t, pre, w1t, dpre_out, x_mid_, ln_g, ln_mean, ln_rstd, dx_mid_out, colsum_partials,
                                                ln_partials, nullptr, nullptr, R, D, F))
    return rc;
  const int rc = dig_mlp_chain_bwd(dy_, w2t, pre, w1t, dpre_out, dx_mid_out, colsum_partials, R, D, F, stream);
  if (rc != DIG_OK) return rc;
  const bf16_t* dy = (const bf16_t*)dy_; const bf16_t* x = (const bf16_t*)x_mid_;
  bf16_t* dx = (bf16_t*)dx_mid_out;
  const int np = dig_rules::mlp_chain_ln_parts(R);
#pragma omp parallel for
  for (int pr = 0; pr < np; ++pr) {
    float* w = ln_partials + (size_t)pr * 3 * D;
    std::fill(w, w + 3 * D, 0.f);
    std::vector<float> xh(D), d(D);
    for (int r = pr * 128; r < std::min(R, pr * 128 + 128); ++r) {
      float c1 = 0.f, c2 = 0.f;
      for (int c = 0; c < D; ++c) {
        xh[c] = (bf2f(x[(size_t)r * D + c]) - ln_mean[r]) * ln_rstd[r];
        const float g = bf2f(dx[(size_t)r * D + c]);
        w[c] += g * xh[c];
        w[D + c] += g;
        d[c] = g * ln_g[c];
        c1 += d[c];
        c2 += d[c] * xh[c];
      }
      c1 /= D;
      c2 /= D;
      for (int c = 0; c < D; ++c) {
        const float e = bf2f(dy[(size_t)r * D + c]);
        w[2 * D + c] += e;
        dx[(size_t)r * D + c] = f2bf(e + ln_rstd[r] * (d[c] - c1 - xh[c] * c2));
      }
    }
  }
  return DIG_OK;
}

int dig_mlp_chain_bwd_ln_proj(const void* dy, const void* w2t, const void* pre, const void* w1t, void* dpre_out, const void* x_mid,
                              const float* ln_g, const float* ln_mean, const float* ln_rstd, void* dx_mid_out, float* colsum_partials,
                              float* ln_partials, const void* projt_, void* dctx_out_, int R, int D, int F, hipStream_t stream) {
  if (int rc = dig_rules::mlp_chain_bwd_ln_proj(dy, w2t, pre, w1t, dpre_out, x_mid, ln_g, ln_mean, ln_rstd, dx_mid_out, colsum_partials, ln_partials,
                                                projt_, dctx_out_, R, D, F))
    return rc;
  const int rc = dig_mlp_chain_bwd_ln(dy, w2t, pre, w1t, dpre_out, x_mid, ln_g, ln_mean, ln_rstd, dx_mid_out, colsum_partials, ln_partials, R, D, F,
                                      stream);
  if (rc != DIG_OK || !projt_) return rc;
  const bf16_t* dx = (const bf16_t*)dx_mid_out; const bf16_t* pt = (const bf16_t*)projt_;
  bf16_t* dc = (bf16_t*)dctx_out_;
  std::vector<float> W((size_t)D * D);
  for (size_t i = 0; i < W.size(); ++i) W[i] = bf2f(pt[i]);          // [in][out]
#pragma omp parallel
  {
    std::vector<float> xr(D);
#pragma omp for
    for (int r = 0; r < R; ++r) {
      for (int o = 0; o < D; ++o) xr[o] = bf2f(dx[(size_t)r * D + o]);
      for (int i = 0; i < D; ++i) {
        float a = 0.f;
        const float* w = &W[(size_t)i * D];
        for (int o = 0; o < D; ++o) a += w[o] * xr[o];
        dc[(size_t)r * D + i] = f2bf(a);
      }
    }
  }
  return DIG_OK;
}

int dig_transpose_bf16(const void* src_, void* dst_, int rows, int cols, hipStream_t) {
  if (int rc = dig_rules::transpose_bf16(src_, dst_, rows, cols)) return rc;
  const bf16_t* src = (const bf16_t*)src_; bf16_t* dst = (bf16_t*)dst_;
#pragma omp parallel for
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) dst[(size_t)c * rows + r] = src[(size_t)r * cols + c];
  return DIG_OK;
}

int dig_transpose_bf16_multi(const void* const* srcs, void* const* dsts, int count, int rows, int cols, hipStream_t st) {
  if (int rc = dig_rules::transpose_bf16_multi(srcs, dsts, count, rows, cols)) return rc;
  for (int k = 0; k < count; ++k) {
    const int rc = dig_transpose_bf16(srcs[k], dsts[k], rows, cols, st);
    if (rc) return rc;
  }
  return DIG_OK;
}

int dig_gelu_bwd(const void* dact_, const void* pre_, void* dpre_, long long n, hipStream_t) {
  if (int rc = dig_rules::gelu_bwd(dact_, pre_, dpre_, n)) return rc;
  const bf16_t* dact = (const bf16_t*)dact_;
  const bf16_t* pre = (const bf16_t*)pre_;
  bf16_t* dpre = (bf16_t*)dpre_;
#pragma omp parallel for
  for (long long i = 0; i < n; ++i) dpre[i] = f2bf(bf2f(dact[i]) * dgelu_f(bf2f(pre[i])));
  return DIG_OK;
}

int dig_add_bf16(const void* a_, const void* b_, void* out_, long long n, hipStream_t) {
  if (int rc = dig_rules::add_bf16(a_, b_, out_, n)) return rc;
  const bf16_t* a = (const bf16_t*)a_;
  const bf16_t* b = (const bf16_t*)b_;
  bf16_t* o = (bf16_t*)out_;
  for (long long i = 0; i < n; ++i) o[i] = f2bf(bf2f(a[i]) + bf2f(b[i]));
  return DIG_OK;
}

int dig_cast_f32_to_bf16(const float* x, void* y, long long n, hipStream_t) {
  if (int rc = dig_rules::cast_f32_to_bf16(x, y, n)) return rc;
  for (long long i = 0; i < n; ++i) ((bf16_t*)y)[i] = f2bf(x[i]);
  return DIG_OK;
}

int dig_cast_bf16_to_f32(const void* x, float* y, long long n, hipStream_t) {
  if (int rc = dig_rules::cast_bf16_to_f32(x, y, n)) return rc;
  for (long long i = 0; i < n; ++i) y[i] = bf2f(((const bf16_t*)x)[i]);
  return DIG_OK;
}

int dig_pad_cast_rows(const float* src, void* dst_, int M, int C, int M_pad, int ld, hipStream_t) {
  if (int rc = dig_rules::pad_cast_rows(src, dst_, M, C, M_pad, ld)) return rc;
  bf16_t* dst = (bf16_t*)dst_;
  for (int r = 0; r < M_pad; ++r)
    for (int c = 0; c < ld; ++c) dst[(size_t)r * ld + c] = (r < M && c < C) ? f2bf(src[(size_t)r * C + c]) : (bf16_t)0;
  return DIG_OK;
}

int dig_fill_f32(float* x, long long n, float value, hipStream_t) {
  if (int rc = dig_rules::fill_f32(x, n, value)) return rc;
  std::fill(x, x + n, value);
  return DIG_OK;
}

int dig_scale_f32(float* x, long long n, float s, hipStream_t) {
  if (int rc = dig_rules::scale_f32(x, n, s)) return rc;
  for (long long i = 0; i < n; ++i) x[i] *= s;
  return DIG_OK;
}

int dig_scale_by_device_scalar(float* x, long long n, const float* scalar, float extra, hipStream_t) {
  if (int rc = dig_rules::scale_by_device_scalar(x, n, scalar, extra)) return rc;
  const float s = scalar[0] * extra;
  for (long long i = 0; i < n; ++i) x[i] *= s;
  return DIG_OK;
}

int dig_axpy_f32(float* y, const float* x, long long n, float a, hipStream_t) {
  if (int rc = dig_rules::axpy_f32(y, x, n, a)) return rc;
  for (long long i = 0; i < n; ++i) y[i] += a * x[i];
  return DIG_OK;
}

int dig_dropout_apply(const void* in_, void* out_, long long rows, int cols, const dig_dropout_t* drop, hipStream_t) {
  if (int rc = dig_rules::dropout_apply(in_, out_, rows, cols, drop)) return rc;
  const bf16_t* in = (const bf16_t*)in_;
  bf16_t* out = (bf16_t*)out_;
#pragma omp parallel for
  for (long long i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) out[i * cols + j] = f2bf(drop_apply(bf2f(in[i * cols + j]), *drop, i, j, cols));
  return DIG_OK;
}

// ---- grouped weight gradients (csrc/wgrad.hip): same host-side planning and the same two-call protocol (partial slabs now, their
// sum folded into the gradients by the next call); the slab layout is this build's own ([tile][split][128][128 fn], row-major)
int dig_wgrad_group(const dig_wgrad_prob_t* probs, int n_probs, const dig_wgrad_prob_t* fold_probs, int n_fold, int R, int splits,
                    const unsigned* wg_map, int n_wg, float* slabs, const float* fold_slabs, int fold_splits, int fn, int wa, hipStream_t) {
  if (int rc = dig_rules::wgrad_group(probs, n_probs, fold_probs, n_fold, R, splits, wg_map, n_wg, slabs, fold_slabs, fold_splits, fn, wa)) return rc;
  const int TJ = 128 * fn, TI = 128 * wa;
  auto first_tiles = [&](const dig_wgrad_prob_t* q, int n) {              // first tile of every problem, then the table's tile count
    std::vector<int> tile0(1, 0);
    for (int k = 0; k < n; ++k) tile0.push_back(tile0.back() + ((q[k].I + TI - 1) / TI) * (q[k].J / TJ));
    return tile0;
  };
  const std::vector<int> t0 = first_tiles(probs, n_probs), f0 = first_tiles(fold_probs, n_fold);
  const size_t SLAB = (size_t)TI * TJ;
  // fold of the previous call's slabs (split order)
  for (int k = 0; k < n_fold; ++k) {
    const dig_wgrad_prob_t& q = fold_probs[k];
    const int tj_n = q.J / TJ;
    for (int T = f0[k]; T < f0[k + 1]; ++T) {
      const int lt = T - f0[k], ti = lt / tj_n, tj = lt % tj_n;
#pragma omp parallel for
      for (int il = 0; il < TI; ++il)
        for (int jl = 0; jl < TJ; ++jl) {
          const int i = ti * TI + il, j = tj * TJ + jl;
          if (i >= q.I) continue;
          float s = 0.f;
          for (int sp = 0; sp < fold_splits; ++sp) s += fold_slabs[((size_t)T * fold_splits + sp) * SLAB + (size_t)il * TJ + jl];
          if (q.trans_out) q.out[(size_t)j * q.ldo + i] += s; else q.out[(size_t)i * q.ldo + j] += s;
        }
    }
  }
  if (!n_probs) return DIG_OK;
  const int per = dig_rules::wgrad_group_rows_per_split(R, splits);
  for (int w = 0; w < n_wg; ++w) {
    const unsigned item = wg_map[w];
    if (item == 0xffffffffu) continue;
    const int tile = (int)(item & 0xffffu), split = (int)(item >> 16);
    int pi = 0;
    while (pi + 1 < n_probs && tile >= t0[pi + 1]) ++pi;
    if (tile >= t0[n_probs] || split >= splits) continue;                  // (an entry dig_wgrad_group_plan never writes: no slab is its)
    const dig_wgrad_prob_t& q = probs[pi];
    const bf16_t* A = (const bf16_t*)q.A;
    const bf16_t* B = (const bf16_t*)q.B;
    const int tj_n = q.J / TJ, lt = tile - t0[pi], ti = lt / tj_n, tj = lt % tj_n;
    const int rbeg = split * per, rend = std::min(R, rbeg + per);
    float* slab = slabs + ((size_t)tile * splits + split) * SLAB;
#pragma omp parallel for
    for (int il = 0; il < TI; ++il) {
      std::vector<float> acc(TJ, 0.f);
      if (ti * TI + il >= q.I) { std::memcpy(slab + (size_t)il * TJ, acc.data(), (size_t)TJ * 4); continue; }
      for (int r = rbeg; r < rend; ++r) {
        const float a = bf2f(A[(size_t)r * q.lda + ti * TI + il]);
        const bf16_t* brow = B + (size_t)r * q.ldb + tj * TJ;
        for (int jl = 0; jl < TJ; ++jl) acc[jl] += a * bf2f(brow[jl]);
      }
      std::memcpy(slab + (size_t)il * TJ, acc.data(), (size_t)TJ * 4);
    }
  }
  return DIG_OK;
}

// launch probe: nothing to time in this build
int dig_probe_start(void) { return DIG_OK; }
int dig_probe_stop(float*, int) { return 0; }

}  // extern "C"

// one call per encoder block: the same sequences as the HIP build (every call here is synchronous, so the hand-over to the side stream is empty)
#define DIG_BLOCK_HANDOVER(main, side) 0
#include "../dig_amd/csrc/abi_queries.inc"
#include "../dig_amd/csrc/encoder_block.inc"
