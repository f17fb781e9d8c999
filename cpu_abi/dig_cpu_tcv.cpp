// libdig_cpu.so, text-conditional cross-attention (`--text_cond_vis`): plain-C++ builds of dig_tcv_attn_fwd / dig_tcv_attn_bwd
// (include/dig_hip.h, csrc/text_cond_attn.hip).  Same contract as dig_cpu_rec.cpp: fp32 loops over host memory, bf16 rounding only where
// the HIP build stores bf16, `stream` ignored.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dig_cpu_common.h"

namespace {

inline float keep(const dig_dropout_t* d, int t, int k, int sh) {
  if (!d || !d->thr) return 1.f;
  return drop_hash(d->k0, d->k1, ((unsigned)t << 16) | (unsigned)k, (unsigned)sh) >= d->thr ? d->scale : 0.f;
}

struct Row {                                        // one query row: tanh(gamma), tanh(beta)
  std::vector<float> g, b;
  Row(const bf16_t* film, int d) : g(d), b(d) {
    for (int j = 0; j < d; ++j) { g[j] = std::tanh(bf2f(film[j])); b[j] = std::tanh(bf2f(film[d + j])); }
  }
};

// cond = mem + LN(g * vk + b) of one key row; zh = the normalised z; returns rstd
float cond_row(const Row& q, const bf16_t* vk, const bf16_t* mem, const float* lg, const float* lb, float eps, int d, float* zh, float* cond) {
  float s = 0.f;
  for (int j = 0; j < d; ++j) { zh[j] = q.g[j] * bf2f(vk[j]) + q.b[j]; s += zh[j]; }
  const float mean = s / (float)d;
  float v = 0.f;
  for (int j = 0; j < d; ++j) { const float e = zh[j] - mean; v += e * e; }
  const float rstd = 1.f / std::sqrt(v / (float)d + eps);
  for (int j = 0; j < d; ++j) {
    zh[j] = (zh[j] - mean) * rstd;
    cond[j] = bf2f(mem[j]) + zh[j] * lg[j] + lb[j];
  }
  return rstd;
}

}  // namespace

extern "C" {

int dig_tcv_attn_fwd(const void* film_, const void* u_, const void* vk_, const void* mem_, const float* lnc_g, const float* lnc_b, float eps,
                     void* c_, float* lse, float* wmean, int S, int Lq, int N, int heads, int d, int slots_per_mem, const dig_dropout_t* drop,
                     hipStream_t) {
  if (int rc = dig_rules::tcv_attn_fwd(film_, u_, vk_, mem_, lnc_g, lnc_b, eps, c_, lse, wmean, S, Lq, N, heads, d, slots_per_mem, drop)) return rc;
  const bf16_t* film = (const bf16_t*)film_; const bf16_t* u = (const bf16_t*)u_; const bf16_t* vk = (const bf16_t*)vk_;
  const bf16_t* mem = (const bf16_t*)mem_;
  bf16_t* c = (bf16_t*)c_;
  const int HD = heads * d;
#pragma omp parallel for
  for (int r = 0; r < S * Lq; ++r) {
    const int s = r / Lq, t = r - s * Lq;
    const size_t mrow = (size_t)(s / slots_per_mem) * N;
    const Row q(film + (size_t)r * 2 * d, d);
    std::vector<float> cond((size_t)N * d), zh(d), W((size_t)heads * N), acc(HD, 0.f);
    for (int k = 0; k < N; ++k) {
      cond_row(q, vk + (mrow + k) * d, mem + (mrow + k) * d, lnc_g, lnc_b, eps, d, zh.data(), &cond[(size_t)k * d]);
      for (int h = 0; h < heads; ++h) {
        float a = 0.f;
        for (int j = 0; j < d; ++j) a += bf2f(u[(size_t)r * HD + h * d + j]) * cond[(size_t)k * d + j];
        W[(size_t)h * N + k] = a;
      }
    }
    for (int h = 0; h < heads; ++h) {
      float m = W[(size_t)h * N];
      for (int k = 1; k < N; ++k) m = std::max(m, W[(size_t)h * N + k]);
      float sum = 0.f;
      for (int k = 0; k < N; ++k) { W[(size_t)h * N + k] = std::exp(W[(size_t)h * N + k] - m); sum += W[(size_t)h * N + k]; }
      for (int k = 0; k < N; ++k) W[(size_t)h * N + k] /= sum;
      lse[(size_t)r * heads + h] = m + std::log(sum);
    }
    for (int k = 0; k < N; ++k) {
      float a = 0.f;
      for (int h = 0; h < heads; ++h) a += W[(size_t)h * N + k];
      if (wmean) wmean[(size_t)r * N + k] = a / (float)heads;
      for (int h = 0; h < heads; ++h) {
        const float w = W[(size_t)h * N + k] * keep(drop, t, k, s * heads + h);
        for (int j = 0; j < d; ++j) acc[(size_t)h * d + j] += w * cond[(size_t)k * d + j];
      }
    }
    for (int e = 0; e < HD; ++e) c[(size_t)r * HD + e] = f2bf(acc[e]);
  }
  return DIG_OK;
}

int dig_tcv_attn_bwd(const void* film_, const void* u_, const void* vk_, const void* mem_, const float* lnc_g, const float* lnc_b, float eps,
                     const void* c_, const float* lse, const void* dc_, void* du_, void* dfilm_, void* dvk_, void* dmem_, float* dlnc_g,
                     float* dlnc_b, float* workspace, int S, int Lq, int N, int heads, int d, int slots_per_mem, const dig_dropout_t* drop,
                     hipStream_t) {
  if (int rc = dig_rules::tcv_attn_bwd(film_, u_, vk_, mem_, lnc_g, lnc_b, eps, c_, lse, dc_, du_, dfilm_, dvk_, dmem_, dlnc_g, dlnc_b, workspace, S,
                                       Lq, N, heads, d, slots_per_mem, drop))
    return rc;
  const bf16_t* film = (const bf16_t*)film_; const bf16_t* u = (const bf16_t*)u_; const bf16_t* vk = (const bf16_t*)vk_;
  const bf16_t* mem = (const bf16_t*)mem_; const bf16_t* dc = (const bf16_t*)dc_;
  bf16_t* du = (bf16_t*)du_; bf16_t* dfilm = (bf16_t*)dfilm_; bf16_t* dvk = (bf16_t*)dvk_; bf16_t* dmem = (bf16_t*)dmem_;
  const int HD = heads * d, R = S * Lq;
#pragma omp parallel for
  for (int s = 0; s < S; ++s) {                      // a sequence owns its memory (slots_per_mem = 1): dvk / dmem sum over its queries in order
    const size_t mrow = (size_t)s * N;
    std::vector<float> av((size_t)N * d, 0.f), am((size_t)N * d, 0.f), zh(d), cond(d), dcond(d), dz(d), dl(heads);
    for (int t = 0; t < Lq; ++t) {
      const size_t r = (size_t)s * Lq + t;
      const Row q(film + r * 2 * d, d);
      std::vector<float> acc_u(HD, 0.f), dga(d, 0.f), dbe(d, 0.f), delta(heads);
      float* part = workspace + r * 2 * d;
      for (int j = 0; j < 2 * d; ++j) part[j] = 0.f;
      for (int h = 0; h < heads; ++h) delta[h] = 0.f;
      for (int k = 0; k < N; ++k) {                  // delta = dc . c over the keys in fp32 (not from the rounded c: csrc/text_cond_attn.hip)
        cond_row(q, vk + (mrow + k) * d, mem + (mrow + k) * d, lnc_g, lnc_b, eps, d, zh.data(), cond.data());
        for (int h = 0; h < heads; ++h) {
          float lgt = 0.f, ph = 0.f;
          for (int j = 0; j < d; ++j) {
            lgt += bf2f(u[r * HD + h * d + j]) * cond[j];
            ph += bf2f(dc[r * HD + h * d + j]) * cond[j];
          }
          delta[h] += std::exp(lgt - lse[r * heads + h]) * keep(drop, t, k, s * heads + h) * ph;
        }
      }
      for (int k = 0; k < N; ++k) {
        const float rstd = cond_row(q, vk + (mrow + k) * d, mem + (mrow + k) * d, lnc_g, lnc_b, eps, d, zh.data(), cond.data());
        for (int j = 0; j < d; ++j) dcond[j] = 0.f;
        for (int h = 0; h < heads; ++h) {
          float lgt = 0.f, ph = 0.f;
          for (int j = 0; j < d; ++j) {
            lgt += bf2f(u[r * HD + h * d + j]) * cond[j];
            ph += bf2f(dc[r * HD + h * d + j]) * cond[j];
          }
          const float w = std::exp(lgt - lse[r * heads + h]), m = keep(drop, t, k, s * heads + h);
          dl[h] = w * (m * ph - delta[h]);
          for (int j = 0; j < d; ++j) {
            dcond[j] += w * m * bf2f(dc[r * HD + h * d + j]) + dl[h] * bf2f(u[r * HD + h * d + j]);
            acc_u[(size_t)h * d + j] += dl[h] * cond[j];
          }
        }
        float s1 = 0.f, s2 = 0.f;
        for (int j = 0; j < d; ++j) { const float a = dcond[j] * lnc_g[j]; s1 += a; s2 += a * zh[j]; }
        s1 /= (float)d; s2 /= (float)d;
        for (int j = 0; j < d; ++j) {
          dz[j] = rstd * (dcond[j] * lnc_g[j] - s1 - zh[j] * s2);
          part[j] += dcond[j] * zh[j];
          part[d + j] += dcond[j];
          dga[j] += dz[j] * bf2f(vk[(mrow + k) * d + j]);
          dbe[j] += dz[j];
          av[(size_t)k * d + j] += q.g[j] * dz[j];
          am[(size_t)k * d + j] += dcond[j];
        }
      }
      for (int e = 0; e < HD; ++e) du[r * HD + e] = f2bf(acc_u[e]);
      for (int j = 0; j < d; ++j) {
        dfilm[r * 2 * d + j] = f2bf(dga[j] * (1.f - q.g[j] * q.g[j]));
        dfilm[r * 2 * d + d + j] = f2bf(dbe[j] * (1.f - q.b[j] * q.b[j]));
      }
    }
    for (size_t e = 0; e < (size_t)N * d; ++e) { dvk[mrow * d + e] = f2bf(av[e]); dmem[mrow * d + e] = f2bf(am[e]); }
  }
  for (int j = 0; j < 2 * d; ++j) {                  // vis_cond_norm's gradients: the rows' shares in row order
    float a = 0.f;
    for (int r = 0; r < R; ++r) a += workspace[(size_t)r * 2 * d + j];
    (j < d ? dlnc_g[j] : dlnc_b[j - d]) += a;
  }
  return DIG_OK;
}

}  // extern "C"
