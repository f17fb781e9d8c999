// libdig_cpu.so, second part: plain-C++ builds of the entry points either side of the pre-training step (SURVEY.md 8(f) rows N1 / N3 / N4:
// input transform, K/V-cached decode + beam step + metrics, the fine-tune step's sequence attention / losses / embeddings, the GRU attention
// head).  Same contract as dig_cpu.cpp: names, argument lists, error codes and storage conventions of include/dig_hip.h, straightforward
// loops over host memory, `stream` ignored, every call synchronous; integer / byte work bit for bit, floating point to the tolerance of the
// operator tests.  Test infrastructure for a GPU-less container -- nothing under dig_amd/ loads it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "dig_cpu_common.h"

namespace {

constexpr float NEG_INF = -std::numeric_limits<float>::infinity();

// ---------------------------------------------------------------------------------------------------------------- input transform (N3)
constexpr int PRECISION_BITS = 32 - 8 - 2;

inline double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for every output index of one axis (csrc/input.hip coeffs_for, same operation order)
void axis_coeffs(int in_size, int out_size, int ksize, std::vector<int>& kk, std::vector<int>& bounds) {
  kk.assign((size_t)out_size * ksize, 0);
  bounds.assign((size_t)out_size * 2, 0);
  for (int xx = 0; xx < out_size; ++xx) {
    const double scale = (double)in_size / (double)out_size;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const double center = ((double)xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic_filter(((double)(x + xmin) - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
      double w = bicubic_filter(((double)(x + xmin) - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      kk[(size_t)xx * ksize + x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
}

inline int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

using dig_rules::ksize_for;   // (the LDS rule of the resize needs the tap count too)

inline unsigned philox_first(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

inline long long clamp_tok(long long t, int vocab) { return t < 0 ? 0 : (t >= vocab ? vocab - 1 : t); }

// log-sum-exp of a row (max-shifted)
inline void row_max_sum(const float* x, int C, float& m, float& s) {
  m = NEG_INF;
  for (int c = 0; c < C; ++c) m = std::max(m, x[c]);
  s = 0.f;
  for (int c = 0; c < C; ++c) s += std::exp(x[c] - m);
}

inline unsigned char canon_of(long long v, const unsigned char* canon, int n_classes) { return (v >= 0 && v < n_classes) ? canon[v] : 0; }
// Levenshtein distance with unit costs, one row of the table at a time
inline int levenshtein(const int* x, int xlen, const int* y, int ylen) {
  std::vector<int> row(ylen + 1);
  for (int j = 0; j <= ylen; ++j) row[j] = j;
  for (int i = 0; i < xlen; ++i) {
    int diag = row[0];
    row[0] = i + 1;
    for (int j = 1; j <= ylen; ++j) {
      const int old = row[j];
      row[j] = std::min(std::min(old, row[j - 1]) + 1, diag + (x[i] != y[j - 1] ? 1 : 0));
      diag = old;
    }
  }
  return row[ylen];
}

}  // namespace

extern "C" {

int dig_resize_bicubic_normalize_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                                    float* out, int out_h, int out_w, float mean, float std_, int max_h, int max_w, hipStream_t) {
  if (int rc = dig_rules::resize_bicubic_normalize_u8(packed, offsets, heights, widths, n_img, out, out_h, out_w, mean, std_, max_h, max_w))
    return rc;
  const int ksh = ksize_for(max_w, out_w), ksv = ksize_for(max_h, out_h);
#pragma omp parallel for
  for (int img = 0; img < n_img; ++img) {
    const int h = heights[img], w = widths[img];
    const unsigned char* src = packed + offsets[img];
    std::vector<int> kh, bh, kv, bv;
    axis_coeffs(w, out_w, ksh, kh, bh);
    axis_coeffs(h, out_h, ksv, kv, bv);
    const bool pass_h = (w != out_w), pass_v = (h != out_h);
    const size_t plane = (size_t)out_h * out_w;
    float* o = out + (size_t)img * 3 * plane;
    for (int p = 0; p < out_h * out_w; ++p) {
      const int yy = p / out_w, xx = p - yy * out_w;
      const int x0 = pass_h ? bh[2 * xx] : xx, nx = pass_h ? bh[2 * xx + 1] : 1;
      const int y0 = pass_v ? bv[2 * yy] : yy, ny = pass_v ? bv[2 * yy + 1] : 1;
      const int* kx = kh.data() + (size_t)xx * ksh;
      const int* ky = kv.data() + (size_t)yy * ksv;
      int a[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
      int r[3] = {0, 0, 0};
      for (int y = 0; y < ny; ++y) {
        const unsigned char* row = src + ((size_t)(y0 + y) * w + x0) * 3;
        int hv[3];
        if (pass_h) {
          int s[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
          for (int x = 0; x < nx; ++x)
            for (int c = 0; c < 3; ++c) s[c] += (int)row[3 * x + c] * kx[x];
          for (int c = 0; c < 3; ++c) hv[c] = clip8(s[c]);
        } else {
          for (int c = 0; c < 3; ++c) hv[c] = row[c];
        }
        for (int c = 0; c < 3; ++c) {
          if (pass_v) a[c] += hv[c] * ky[y];
          else r[c] = hv[c];
        }
      }
      for (int c = 0; c < 3; ++c) {
        if (pass_v) r[c] = clip8(a[c]);
        o[c * plane + p] = ((float)r[c] / 255.0f - mean) / std_;
      }
    }
  }
  return DIG_OK;
}

int dig_random_masks(unsigned char* mask, int n_rows, int n_patches, int num_mask, unsigned long long seed, unsigned step, hipStream_t) {
  if (int rc = dig_rules::random_masks(mask, n_rows, n_patches, num_mask, seed, step)) return rc;
  const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
#pragma omp parallel for
  for (int r = 0; r < n_rows; ++r) {
    std::vector<unsigned> keys(n_patches);
    for (int p = 0; p < n_patches; ++p) keys[p] = philox_first((unsigned)r, (unsigned)p, step, 0u, k0, k1);
    for (int p = 0; p < n_patches; ++p) {
      int rank = 0;
      for (int q = 0; q < n_patches; ++q) rank += (keys[q] < keys[p]) || (keys[q] == keys[p] && q < p);
      mask[(size_t)r * n_patches + p] = rank < num_mask ? 1 : 0;
    }
  }
  return DIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- decode (N4)
int dig_decode_embed(const long long* tokens, const float* emb, const float* pe_row, void* x_, int B, int d, int vocab, hipStream_t) {
  if (int rc = dig_rules::decode_embed(tokens, emb, pe_row, x_, B, d, vocab)) return rc;
  bf16_t* x = (bf16_t*)x_;
  for (int b = 0; b < B; ++b) {
    const long long t = clamp_tok(tokens[b], vocab);
    for (int c = 0; c < d; ++c) x[(size_t)b * d + c] = f2bf(emb[(size_t)t * d + c] + pe_row[c]);
  }
  return DIG_OK;
}

int dig_decode_self_attn(const void* qkv_cache, void* out_, int B, int T, int heads, int head_dim, int t, float scale, hipStream_t) {
  if (int rc = dig_rules::decode_self_attn(qkv_cache, out_, B, T, heads, head_dim, t, scale)) return rc;
  const bf16_t* qkv = (const bf16_t*)qkv_cache;
  bf16_t* out = (bf16_t*)out_;
  const int hk = heads * head_dim;
  const size_t row = (size_t)3 * hk;
#pragma omp parallel for collapse(2)
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < heads; ++h) {
      const bf16_t* base = qkv + (size_t)b * T * row + h * head_dim;
      std::vector<float> s(t + 1);
      float m = NEG_INF;
      for (int j = 0; j <= t; ++j) {
        float a = 0.f;
        for (int c = 0; c < head_dim; ++c) a += bf2f(base[(size_t)t * row + c]) * scale * bf2f(base[(size_t)j * row + hk + c]);
        s[j] = a;
        m = std::max(m, a);
      }
      float l = 0.f;
      for (int j = 0; j <= t; ++j) { s[j] = std::exp(s[j] - m); l += s[j]; }
      for (int c = 0; c < head_dim; ++c) {
        float a = 0.f;
        for (int j = 0; j <= t; ++j) a += s[j] * bf2f(base[(size_t)j * row + 2 * hk + c]);
        out[(size_t)b * hk + h * head_dim + c] = f2bf(a / l);
      }
    }
  return DIG_OK;
}

int dig_decode_cross_attn(const void* q_, const void* kv_mem, void* out_, float* weights, int B, int n_mem, int heads, int head_dim, float scale,
                          int slots_per_mem, hipStream_t) {
  if (int rc = dig_rules::decode_cross_attn(q_, kv_mem, out_, weights, B, n_mem, heads, head_dim, scale, slots_per_mem)) return rc;
  const bf16_t* q = (const bf16_t*)q_;
  const bf16_t* kv = (const bf16_t*)kv_mem;
  bf16_t* out = (bf16_t*)out_;
  const int hk = heads * head_dim;
#pragma omp parallel for collapse(2)
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < heads; ++h) {
      const bf16_t* kb = kv + (size_t)(b / slots_per_mem) * n_mem * 2 * hk + h * head_dim;
      std::vector<float> s(n_mem);
      float m = NEG_INF;
      for (int j = 0; j < n_mem; ++j) {
        float a = 0.f;
        for (int c = 0; c < head_dim; ++c) a += bf2f(q[(size_t)b * hk + h * head_dim + c]) * scale * bf2f(kb[(size_t)j * 2 * hk + c]);
        s[j] = a;
        m = std::max(m, a);
      }
      float l = 0.f;
      for (int j = 0; j < n_mem; ++j) { s[j] = std::exp(s[j] - m); l += s[j]; }
      const float inv = 1.f / l;
      if (weights)
        for (int j = 0; j < n_mem; ++j) weights[((size_t)b * heads + h) * n_mem + j] = s[j] * inv;
      for (int c = 0; c < head_dim; ++c) {
        float a = 0.f;
        for (int j = 0; j < n_mem; ++j) a += s[j] * bf2f(kb[(size_t)j * 2 * hk + hk + c]);
        out[(size_t)b * hk + h * head_dim + c] = f2bf(a * inv);
      }
    }
  return DIG_OK;
}

int dig_softmax_argmax(const float* logits, int ld, float* probs, long long* tokens, int B, int C, hipStream_t) {
  if (int rc = dig_rules::softmax_argmax(logits, ld, probs, tokens, B, C)) return rc;
  for (int b = 0; b < B; ++b) {
    const float* row = logits + (size_t)b * ld;
    float m = NEG_INF;
    int am = 0x7fffffff;
    for (int c = 0; c < C; ++c)
      if (row[c] > m) { m = row[c]; am = c; }                 // first index of the maximum (torch.max)
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += std::exp(row[c] - m);
    const float inv = 1.f / s;
    for (int c = 0; c < C; ++c) probs[(size_t)b * C + c] = std::exp(row[c] - m) * inv;
    tokens[b] = am == 0x7fffffff ? 0 : am;                    // no entry above -inf: index 0, as torch.max
  }
  return DIG_OK;
}

// The ranking of a beam-search step (beam_rank of csrc/decode.hip): per sample the candidate table, the top bw by (value, lowest index)
// -- or the forced candidates in their place -- and the step's symbol / predecessor / stored score / next running score.
static void beam_rank(const float* logits, int ld, float* seq_scores, int B, int bw, int C, int eos, long long* symbols, long long* predecessors,
                      float* stored_scores, const long long* forced) {
  const int n = bw * C;
  std::vector<float> cand(n);
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < bw; ++k) {
      const float* row = logits + (size_t)(b * bw + k) * ld;
      float m, s;
      row_max_sum(row, C, m, s);
      const float lse = m + std::log(s);
      for (int c = 0; c < C; ++c) cand[k * C + c] = seq_scores[b * bw + k] + (row[c] - lse);
    }
    for (int r = 0; r < bw; ++r) {
      float bv = NEG_INF;
      int bi = 0x7fffffff;
      if (forced) {
        bi = (int)clamp_tok(forced[b * bw + r], n);
        bv = cand[bi];
      } else {
        for (int i = 0; i < n; ++i)
          if (cand[i] > bv || (cand[i] == bv && i < bi)) { bv = cand[i]; bi = i; }
        if (bi == 0x7fffffff) bi = r;
        cand[bi] = NEG_INF;
      }
      const int sym = bi % C;
      symbols[b * bw + r] = sym;
      predecessors[b * bw + r] = bi / C + b * bw;
      stored_scores[b * bw + r] = bv;
      seq_scores[b * bw + r] = sym == eos ? NEG_INF : bv;
    }
  }
}

int dig_beam_step(const float* logits, int ld, float* seq_scores, int B, int beam_width, int C, int eos, long long* symbols,
                  long long* predecessors, float* stored_scores, hipStream_t) {
  if (int rc = dig_rules::beam_step(logits, ld, seq_scores, B, beam_width, C, eos, symbols, predecessors, stored_scores)) return rc;
  beam_rank(logits, ld, seq_scores, B, beam_width, C, eos, symbols, predecessors, stored_scores, nullptr);
  return DIG_OK;
}

// the ranking, then the gather of the recurrent state by predecessor and the next step's target embedding
int dig_attn_beam_advance(const float* logits, int ld, float* seq_scores, int B, int beam_width, int C, int eos, long long* symbols,
                          long long* predecessors, float* stored_scores, const long long* force_candidates, const float* s_in, const void* sbf_in_,
                          float* s_out, void* sbf_out_, int S, const float* table, int E, void* inp_, int ld_inp, hipStream_t) {
  if (int rc = dig_rules::attn_beam_advance(logits, ld, seq_scores, B, beam_width, C, eos, symbols, predecessors, stored_scores, force_candidates,
                                            s_in, sbf_in_, s_out, sbf_out_, S, table, E, inp_, ld_inp))
    return rc;
  const bf16_t* sbf_in = (const bf16_t*)sbf_in_;
  bf16_t* sbf_out = (bf16_t*)sbf_out_;
  bf16_t* inp = (bf16_t*)inp_;
  beam_rank(logits, ld, seq_scores, B, beam_width, C, eos, symbols, predecessors, stored_scores, force_candidates);
  for (size_t j = 0; j < (size_t)B * beam_width; ++j) {
    const size_t pred = (size_t)predecessors[j], sym = (size_t)symbols[j];
    for (int c = 0; c < S; ++c) { s_out[j * S + c] = s_in[pred * S + c]; sbf_out[j * S + c] = sbf_in[pred * S + c]; }
    for (int c = 0; c < E; ++c) inp[j * ld_inp + c] = f2bf(table[sym * E + c]);
  }
  return DIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- strings (csrc/metrics.hip)
int dig_string_match(const long long* pred, const long long* target, const unsigned char* canon, int n_classes, int eos, int B, int T,
                     unsigned char* match, hipStream_t) {
  if (int rc = dig_rules::string_match(pred, target, canon, n_classes, eos, B, T, match)) return rc;
  for (int b = 0; b < B; ++b) {
    // the kept characters of both rows (cut at eos, dropped classes removed), compared as strings
    std::vector<unsigned char> ps, ts;
    for (int i = 0; i < T && pred[(size_t)b * T + i] != eos; ++i) {
      const unsigned char c = canon_of(pred[(size_t)b * T + i], canon, n_classes);
      if (c) ps.push_back(c);
    }
    for (int i = 0; i < T && target[(size_t)b * T + i] != eos; ++i) {
      const unsigned char c = canon_of(target[(size_t)b * T + i], canon, n_classes);
      if (c) ts.push_back(c);
    }
    match[b] = ps == ts ? 1 : 0;
  }
  return DIG_OK;
}

int dig_char_fmeasure(const long long* pred, const long long* target, const unsigned char* canon, int n_classes, int eos, int B, int T,
                      double* f_per_sample, hipStream_t) {
  if (int rc = dig_rules::char_fmeasure(pred, target, canon, n_classes, eos, B, T, f_per_sample)) return rc;
  for (int b = 0; b < B; ++b) {
    unsigned long long ps = 0, ts = 0;
    for (int i = 0; i < T; ++i) {
      const long long v = pred[(size_t)b * T + i];
      if (v == eos) break;
      const unsigned char c = canon_of(v, canon, n_classes);
      if (c) ps |= 1ull << (c & 63);
    }
    for (int i = 0; i < T; ++i) {
      const long long v = target[(size_t)b * T + i];
      if (v == eos) break;
      const unsigned char c = canon_of(v, canon, n_classes);
      if (c) ts |= 1ull << (c & 63);
    }
    const double n = (double)__builtin_popcountll(ps & ts);
    const double p = n / ((double)__builtin_popcountll(ps) + 1e-5), r = n / ((double)__builtin_popcountll(ts) + 1e-5);
    f_per_sample[b] = 2 * p * r / (p + r + 1e-5);
  }
  return DIG_OK;
}

int dig_tokens_to_text(const long long* tokens, const unsigned char* canon, int n_classes, int eos, int B, int T, int* text, int* len,
                       hipStream_t) {
  if (int rc = dig_rules::tokens_to_text(tokens, canon, n_classes, eos, B, T, text, len)) return rc;
  for (int b = 0; b < B; ++b) {
    int n = 0;
    for (int i = 0; i < T && tokens[(size_t)b * T + i] != eos; ++i) {
      const int c = canon_of(tokens[(size_t)b * T + i], canon, n_classes);
      if (c) text[(size_t)b * T + n++] = c <= 10 ? '0' + (c - 1) : 'a' + (c - 11);
    }
    len[b] = n;
    for (int i = n; i < T; ++i) text[(size_t)b * T + i] = 0;
  }
  return DIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- labels (csrc/labels.hip)
int dig_encode_labels(const int* chars, const int* offsets, const int* class_of, int eos, int padding, int unknown, int max_len, int B,
                      long long* labels, long long* lens, hipStream_t) {
  if (int rc = dig_rules::encode_labels(chars, offsets, class_of, eos, padding, unknown, max_len, B, labels, lens)) return rc;
  if (B == 0) return DIG_OK;
  for (int b = 0; b < B; ++b) {
    const int begin = offsets[b], n = std::clamp(offsets[b + 1] - begin, 0, max_len - 1);
    long long* row = labels + (size_t)b * max_len;
    for (int t = 0; t < max_len; ++t) {
      if (t < n) {
        const int c = chars[begin + t];
        const int k = (c >= 0 && c < 128) ? class_of[c] : -1;
        row[t] = k >= 0 ? k : unknown;
      } else {
        row[t] = t == n ? eos : padding;
      }
    }
    lens[b] = n + 1;
  }
  return DIG_OK;
}

int dig_edit_distance(const int* a, const int* a_len, int lda, int a_rows, const int* a_index, const int* b, const int* b_len, int ldb,
                      int n, int* dist, hipStream_t) {
  if (int rc = dig_rules::edit_distance(a, a_len, lda, a_rows, a_index, b, b_len, ldb, n, dist)) return rc;
  for (int i = 0; i < n; ++i) {
    const int r = a_index ? a_index[i] : i;
    const bool have = r >= 0 && r < a_rows;
    dist[i] = levenshtein(a + (size_t)(have ? r : 0) * lda, have ? std::clamp(a_len[r], 0, lda) : 0, b + (size_t)i * ldb,
                          std::clamp(b_len[i], 0, ldb));
  }
  return DIG_OK;
}


int dig_lexicon_search(const int* query, const int* query_len, int ldq, int B, const int* words, const int* word_len, int ldw, int W,
                       const int* lex_begin, const int* lex_count, int max_count, int* best_index, int* best_dist, void* workspace,
                       long long workspace_bytes, hipStream_t) {
  if (int rc = dig_rules::lexicon_search(query, query_len, ldq, B, words, word_len, ldw, W, lex_begin, lex_count, max_count, best_index, best_dist,
                                         workspace, workspace_bytes))
    return rc;
  for (int q = 0; q < B; ++q) {
    const int begin = std::clamp(lex_begin[q], 0, W);
    const int count = std::clamp(lex_count[q], 0, std::min(W - begin, max_count));
    int bi = -1, bd = -1;
    for (int w = begin; w < begin + count; ++w) {
      const int d = levenshtein(words + (size_t)w * ldw, std::clamp(word_len[w], 0, ldw), query + (size_t)q * ldq,
                                std::clamp(query_len[q], 0, ldq));
      if (bi < 0 || d < bd) { bi = w; bd = d; }
    }
    best_index[q] = bi;
    best_dist[q] = bd;
  }
  return DIG_OK;
}

int dig_seq_confidence(const float* score, const int* text_len, int B, int T, double* conf, hipStream_t) {
  if (int rc = dig_rules::seq_confidence(score, text_len, B, T, conf)) return rc;
  for (int b = 0; b < B; ++b) {
    const int n = text_len[b] < 0 ? 0 : (text_len[b] >= T ? T : text_len[b] + 1);
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += std::log((double)score[(size_t)b * T + j]);
    conf[b] = std::exp(s);
  }
  return DIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- sequence losses (csrc/seq_loss.hip)
int dig_seq_cross_entropy(const float* input, const long long* target, const long long* length, int B, int T, int C, float* row_workspace,
                          float* loss, hipStream_t) {
  if (int rc = dig_rules::seq_cross_entropy(input, target, length, B, T, C, row_workspace, loss)) return rc;
  double total = 0.0;
  for (int row = 0; row < B * T; ++row) {
    const int b = row / T, t = row - b * T;
    float v = 0.f;
    if (t < length[b]) {
      const float* x = input + (size_t)row * C;
      float m, s;
      row_max_sum(x, C, m, s);
      const long long y = clamp_tok(target[row], C);
      v = -(x[y] - m - std::log(s));
    }
    row_workspace[row] = v;
    total += v;
  }
  loss[0] = (float)total * (1.0f / (float)B);
  return DIG_OK;
}

int dig_seq_cross_entropy_bwd(const float* logits, int ld, const long long* target, const long long* length, const float* gscalar, int B, int T,
                              int C, void* dlogits_, int ldd, hipStream_t) {
  if (int rc = dig_rules::seq_cross_entropy_bwd(logits, ld, target, length, gscalar, B, T, C, dlogits_, ldd)) return rc;
  bf16_t* dlogits = (bf16_t*)dlogits_;
  const float sc = (gscalar ? gscalar[0] : 1.f) * (1.0f / (float)B);
  for (int row = 0; row < B * T; ++row) {
    const int b = row / T, t = row - b * T;
    bf16_t* out = dlogits + (size_t)row * ldd;
    if (t >= length[b]) { for (int c = 0; c < ldd; ++c) out[c] = 0; continue; }
    const float* x = logits + (size_t)row * ld;
    float m, s;
    row_max_sum(x, C, m, s);
    const float inv = 1.f / s;
    const long long y = clamp_tok(target[row], C);
    for (int c = 0; c < ldd; ++c) out[c] = c < C ? f2bf(sc * (std::exp(x[c] - m) * inv - (c == y ? 1.f : 0.f))) : (bf16_t)0;
  }
  return DIG_OK;
}

int dig_seq_ls_cross_entropy(const float* input, const long long* target, const long long* length, int B, int T, int C, float smoothing,
                             float* row_workspace, float* loss, hipStream_t) {
  if (int rc = dig_rules::seq_ls_cross_entropy(input, target, length, B, T, C, smoothing, row_workspace, loss)) return rc;
  const int n = B * T;
  double a = 0.0, sj = 0.0, cnt = 0.0;
  for (int row = 0; row < n; ++row) {
    const int b = row / T, t = row - b * T;
    const float* x = input + (size_t)row * C;
    float m, s, sx = 0.f;
    row_max_sum(x, C, m, s);
    for (int c = 0; c < C; ++c) sx += x[c];
    const float lse = m + std::log(s);
    const long long y = clamp_tok(target[row], C);
    row_workspace[row] = t < length[b] ? lse - x[y] : 0.f;
    row_workspace[n + row] = lse - sx / (float)C;
    a += row_workspace[row];
    sj += row_workspace[n + row];
  }
  for (int b = 0; b < B; ++b) { const long long l = length[b]; cnt += (double)(l < 0 ? 0 : (l > T ? T : l)); }
  loss[0] = (float)(((double)(1.f - smoothing) * (double)n * a + (double)smoothing * cnt * sj) / (double)B);
  return DIG_OK;
}

int dig_seq_ls_cross_entropy_bwd(const float* logits, int ld, const long long* target, const long long* length, const float* gscalar, int B,
                                 int T, int C, float smoothing, void* dlogits_, int ldd, hipStream_t) {
  if (int rc = dig_rules::seq_ls_cross_entropy_bwd(logits, ld, target, length, gscalar, B, T, C, smoothing, dlogits_, ldd)) return rc;
  bf16_t* dlogits = (bf16_t*)dlogits_;
  float cnt = 0.f;
  for (int b = 0; b < B; ++b) { const long long l = length[b]; cnt += (float)(l < 0 ? 0 : (l > T ? T : l)); }
  const float confidence = 1.f - smoothing, sc = (gscalar ? gscalar[0] : 1.f) / (float)B, ws = smoothing * cnt;
  for (int row = 0; row < B * T; ++row) {
    const int b = row / T, t = row - b * T;
    const float* x = logits + (size_t)row * ld;
    float m, s;
    row_max_sum(x, C, m, s);
    const float inv = 1.f / s, wn = t < length[b] ? confidence * (float)(B * T) : 0.f;
    const long long y = clamp_tok(target[row], C);
    for (int c = 0; c < ldd; ++c) {
      float v = 0.f;
      if (c < C) {
        const float p = std::exp(x[c] - m) * inv;
        v = sc * (wn * (p - (c == y ? 1.f : 0.f)) + ws * (p - 1.f / (float)C));
      }
      dlogits[(size_t)row * ldd + c] = f2bf(v);
    }
  }
  return DIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- fine-tune step (N1): sequence attention
// per (sample, head): logits = (q . k) * scale, masked keys -> probability 0, lse of the unmasked logits kept; attention dropout multiplies
// the normalised probabilities (csrc/seq_attn.hip)
int dig_seq_attn_fwd_hd(const void* q_, int ldq, const void* k_, int ldk, const void* v_, int ldv, void* out_, int ldo, float* lse, int B,
                        int heads, int Lq, int Lk, float scale, int causal, const long long* lens, const dig_dropout_t* drop, int head_dim,
                        hipStream_t) {
  if (int rc = dig_rules::seq_attn_fwd_hd(q_, ldq, k_, ldk, v_, ldv, out_, ldo, lse, B, heads, Lq, Lk, scale, causal, lens, drop, head_dim))
    return rc;
  const bf16_t* q = (const bf16_t*)q_; const bf16_t* k = (const bf16_t*)k_; const bf16_t* v = (const bf16_t*)v_;
  bf16_t* out = (bf16_t*)out_;
  const bool dropping = drop && drop->thr;
#pragma omp parallel for collapse(2)
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < heads; ++h) {
      const long long len = lens ? lens[b] : (long long)Lk;
      std::vector<float> S((size_t)Lk);
      for (int i = 0; i < Lq; ++i) {
        const bf16_t* qr = q + ((size_t)b * Lq + i) * ldq + h * head_dim;
        float m = NEG_INF;
        for (int j = 0; j < Lk; ++j) {
          const bool ok = (!causal || j <= i) && (!lens || j < len);
          float a = NEG_INF;
          if (ok) {
            a = 0.f;
            const bf16_t* kr = k + ((size_t)b * Lk + j) * ldk + h * head_dim;
            for (int c = 0; c < head_dim; ++c) a += bf2f(qr[c]) * scale * bf2f(kr[c]);
          }
          S[j] = a;
          m = std::max(m, a);
        }
        float sum = 0.f;
        for (int j = 0; j < Lk; ++j) {
          const float e = (S[j] == NEG_INF) ? 0.f : std::exp(S[j] - m);
          sum += e;
          S[j] = dropping ? (drop_keep(drop->k0, drop->k1, ((unsigned)i << 16) | (unsigned)j, (unsigned)(b * heads + h), drop->thr) ? e * drop->scale : 0.f) : e;
        }
        const float inv = sum > 0.f ? 1.f / sum : 0.f;          // a fully masked row: out = 0, lse = -inf
        lse[((size_t)b * heads + h) * Lq + i] = sum > 0.f ? m + std::log(sum) : NEG_INF;
        for (int c = 0; c < head_dim; ++c) {
          float a = 0.f;
          for (int j = 0; j < Lk; ++j) a += S[j] * bf2f(v[((size_t)b * Lk + j) * ldv + h * head_dim + c]);
          out[((size_t)b * Lq + i) * ldo + h * head_dim + c] = f2bf(a * inv);
        }
      }
    }
  return DIG_OK;
}

int dig_seq_attn_fwd_dropout(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo, float* lse, int B,
                             int heads, int Lq, int Lk, float scale, int causal, const long long* lens, const dig_dropout_t* drop, hipStream_t st) {
  return dig_seq_attn_fwd_hd(q, ldq, k, ldk, v, ldv, out, ldo, lse, B, heads, Lq, Lk, scale, causal, lens, drop, 64, st);
}

int dig_seq_attn_fwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo, float* lse, int B, int heads,
                     int Lq, int Lk, float scale, int causal, const long long* lens, hipStream_t st) {
  return dig_seq_attn_fwd_dropout(q, ldq, k, ldk, v, ldv, out, ldo, lse, B, heads, Lq, Lk, scale, causal, lens, nullptr, st);
}

int dig_seq_attn_bwd_hd(const void* q_, int ldq, const void* k_, int ldk, const void* v_, int ldv, const void* dout_, int ldo, const float* lse,
                        void* dq_, int lddq, void* dk_, int lddk, void* dv_, int lddv, int B, int heads, int Lq, int Lk, float scale, int causal,
                        const long long* lens, const dig_dropout_t* drop, int head_dim, hipStream_t) {
  if (int rc = dig_rules::seq_attn_bwd_hd(q_, ldq, k_, ldk, v_, ldv, dout_, ldo, lse, dq_, lddq, dk_, lddk, dv_, lddv, B, heads, Lq, Lk, scale,
                                          causal, lens, drop, head_dim))
    return rc;
  const bf16_t* q = (const bf16_t*)q_; const bf16_t* k = (const bf16_t*)k_; const bf16_t* v = (const bf16_t*)v_;
  const bf16_t* dout = (const bf16_t*)dout_;
  bf16_t* dq = (bf16_t*)dq_; bf16_t* dk = (bf16_t*)dk_; bf16_t* dv = (bf16_t*)dv_;
  const bool dropping = drop && drop->thr;
#pragma omp parallel for collapse(2)
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < heads; ++h) {
      const long long len = lens ? lens[b] : (long long)Lk;
      std::vector<float> P((size_t)Lq * Lk), dS((size_t)Lq * Lk), F((size_t)Lq * Lk);
      for (int i = 0; i < Lq; ++i) {
        const bf16_t* qr = q + ((size_t)b * Lq + i) * ldq + h * head_dim;
        const bf16_t* gr = dout + ((size_t)b * Lq + i) * ldo + h * head_dim;
        const float l = lse[((size_t)b * heads + h) * Lq + i];
        float del = 0.f;
        for (int j = 0; j < Lk; ++j) {
          const bool ok = (!causal || j <= i) && (!lens || j < len);
          float pr = 0.f, dp = 0.f, f = 1.f;
          if (dropping) f = drop_keep(drop->k0, drop->k1, ((unsigned)i << 16) | (unsigned)j, (unsigned)(b * heads + h), drop->thr) ? drop->scale : 0.f;
          if (ok) {
            float sc = 0.f;
            const bf16_t* kr = k + ((size_t)b * Lk + j) * ldk + h * head_dim;
            const bf16_t* vr = v + ((size_t)b * Lk + j) * ldv + h * head_dim;
            for (int c = 0; c < head_dim; ++c) { sc += bf2f(qr[c]) * bf2f(kr[c]); dp += bf2f(gr[c]) * bf2f(vr[c]); }
            pr = std::exp(sc * scale - l);
            dp *= f;
          }
          P[(size_t)i * Lk + j] = pr; dS[(size_t)i * Lk + j] = dp; F[(size_t)i * Lk + j] = f;
          del += pr * dp;
        }
        for (int j = 0; j < Lk; ++j) dS[(size_t)i * Lk + j] = P[(size_t)i * Lk + j] * (dS[(size_t)i * Lk + j] - del);
      }
      for (int j = 0; j < Lk; ++j)
        for (int c = 0; c < head_dim; ++c) {
          float ak = 0.f, av = 0.f;
          for (int i = 0; i < Lq; ++i) {
            ak += dS[(size_t)i * Lk + j] * bf2f(q[((size_t)b * Lq + i) * ldq + h * head_dim + c]);
            av += P[(size_t)i * Lk + j] * F[(size_t)i * Lk + j] * bf2f(dout[((size_t)b * Lq + i) * ldo + h * head_dim + c]);
          }
          dk[((size_t)b * Lk + j) * lddk + h * head_dim + c] = f2bf(ak * scale);
          dv[((size_t)b * Lk + j) * lddv + h * head_dim + c] = f2bf(av);
        }
      for (int i = 0; i < Lq; ++i)
        for (int c = 0; c < head_dim; ++c) {
          float a = 0.f;
          for (int j = 0; j < Lk; ++j) a += dS[(size_t)i * Lk + j] * bf2f(k[((size_t)b * Lk + j) * ldk + h * head_dim + c]);
          dq[((size_t)b * Lq + i) * lddq + h * head_dim + c] = f2bf(a * scale);
        }
    }
  return DIG_OK;
}

int dig_seq_attn_bwd_dropout(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dout, int ldo, const float* lse,
                             void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, int B, int heads, int Lq, int Lk, float scale, int causal,
                             const long long* lens, const dig_dropout_t* drop, hipStream_t st) {
  return dig_seq_attn_bwd_hd(q, ldq, k, ldk, v, ldv, dout, ldo, lse, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, scale, causal, lens, drop, 64, st);
}

int dig_seq_attn_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dout, int ldo, const float* lse, void* dq,
                     int lddq, void* dk, int lddk, void* dv, int lddv, int B, int heads, int Lq, int Lk, float scale, int causal,
                     const long long* lens, hipStream_t st) {
  return dig_seq_attn_bwd_dropout(q, ldq, k, ldk, v, ldv, dout, ldo, lse, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, scale, causal, lens, nullptr, st);
}

int dig_seq_embed_fwd(const long long* tokens, const float* emb, const float* pos_table, void* x_, int B, int T, int d, int vocab, hipStream_t) {
  if (int rc = dig_rules::seq_embed_fwd(tokens, emb, pos_table, x_, B, T, d, vocab)) return rc;
  bf16_t* x = (bf16_t*)x_;
  for (int r = 0; r < B * T; ++r) {
    const long long t = clamp_tok(tokens[r], vocab);
    for (int c = 0; c < d; ++c) x[(size_t)r * d + c] = f2bf(emb[(size_t)t * d + c] + pos_table[(size_t)(r % T) * d + c]);
  }
  return DIG_OK;
}

int dig_seq_embed_bwd_lens(const long long* tokens, const void* dx_, float* demb, int n_tok, int d, int vocab, int T, const long long* lens,
                           hipStream_t) {
  if (int rc = dig_rules::seq_embed_bwd_lens(tokens, dx_, demb, n_tok, d, vocab, T, lens)) return rc;
  const bf16_t* dx = (const bf16_t*)dx_;
  for (int v = 0; v < vocab; ++v) {
    std::vector<int> list;                                             // matching rows, ascending: a fixed summation order
    for (int r = 0; r < n_tok; ++r)
      if (clamp_tok(tokens[r], vocab) == v && (!lens || (r % T) < lens[r / T])) list.push_back(r);
    const int n = (int)list.size();
    if (!n) continue;
    for (int c = 0; c < d; ++c) {
      float a0 = 0.f, a1 = 0.f;
      int k = 0;
      for (; k + 1 < n; k += 2) { a0 += bf2f(dx[(size_t)list[k] * d + c]); a1 += bf2f(dx[(size_t)list[k + 1] * d + c]); }
      if (k < n) a0 += bf2f(dx[(size_t)list[k] * d + c]);
      demb[(size_t)v * d + c] += a0 + a1;
    }
  }
  return DIG_OK;
}

int dig_seq_embed_bwd(const long long* tokens, const void* dx, float* demb, int n_tok, int d, int vocab, hipStream_t st) {
  return dig_seq_embed_bwd_lens(tokens, dx, demb, n_tok, d, vocab, 0, nullptr, st);
}

// ---------------------------------------------------------------------------------------------------------------- GRU attention head (N1)
// (csrc/gru_attn.hip; tanh / sigmoid in libm here, the device uses exp-based forms: fp32 round-off class)
int dig_addattn_fwd(const void* xproj_, const void* sproj_, const float* w, const void* x_, float* alpha, void* ctx_, int ldc, int B, int N, int A,
                    int X, hipStream_t) {
  if (int rc = dig_rules::addattn_fwd(xproj_, sproj_, w, x_, alpha, ctx_, ldc, B, N, A, X)) return rc;
  const bf16_t* xproj = (const bf16_t*)xproj_; const bf16_t* sproj = (const bf16_t*)sproj_; const bf16_t* x = (const bf16_t*)x_;
  bf16_t* ctx = (bf16_t*)ctx_;
#pragma omp parallel for
  for (int b = 0; b < B; ++b) {
    std::vector<float> v(N);
    float m = NEG_INF;
    for (int n = 0; n < N; ++n) {
      float acc = 0.f;
      for (int a = 0; a < A; ++a) acc += w[a] * std::tanh(bf2f(sproj[(size_t)b * A + a]) + bf2f(xproj[((size_t)b * N + n) * A + a]));
      v[n] = acc;
      m = std::max(m, acc);
    }
    float sum = 0.f;
    for (int n = 0; n < N; ++n) { v[n] = std::exp(v[n] - m); sum += v[n]; }
    const float inv = 1.f / sum;
    for (int n = 0; n < N; ++n) { v[n] *= inv; alpha[(size_t)b * N + n] = v[n]; }
    for (int c = 0; c < X; ++c) {
      float a = 0.f;
      for (int n = 0; n < N; ++n) a += v[n] * bf2f(x[((size_t)b * N + n) * X + c]);
      ctx[(size_t)b * ldc + c] = f2bf(a);
    }
  }
  return DIG_OK;
}

// dig_addattn_fwd's loops for the K slots of a sample (sproj row / alpha row / context row b*K + k, tokens of sample b)
int dig_addattn_fwd_slots(const void* xproj_, const void* sproj_, const float* w, const void* x_, float* alpha, void* ctx_, int ldc, int B, int N,
                          int A, int X, int slots, hipStream_t) {
  if (int rc = dig_rules::addattn_fwd_slots(xproj_, sproj_, w, x_, alpha, ctx_, ldc, B, N, A, X, slots)) return rc;
  const bf16_t* xproj = (const bf16_t*)xproj_; const bf16_t* sproj = (const bf16_t*)sproj_; const bf16_t* x = (const bf16_t*)x_;
  bf16_t* ctx = (bf16_t*)ctx_;
  const int K = slots;
#pragma omp parallel for
  for (int r = 0; r < B * K; ++r) {
    const int b = r / K;
    std::vector<float> v(N);
    float m = NEG_INF;
    for (int n = 0; n < N; ++n) {
      float acc = 0.f;
      for (int a = 0; a < A; ++a) acc += w[a] * std::tanh(bf2f(sproj[(size_t)r * A + a]) + bf2f(xproj[((size_t)b * N + n) * A + a]));
      v[n] = acc;
      m = std::max(m, acc);
    }
    float sum = 0.f;
    for (int n = 0; n < N; ++n) { v[n] = std::exp(v[n] - m); sum += v[n]; }
    const float inv = 1.f / sum;
    for (int n = 0; n < N; ++n) { v[n] *= inv; if (alpha) alpha[(size_t)r * N + n] = v[n]; }
    for (int c = 0; c < X; ++c) {
      float a = 0.f;
      for (int n = 0; n < N; ++n) a += v[n] * bf2f(x[((size_t)b * N + n) * X + c]);
      ctx[(size_t)r * ldc + c] = f2bf(a);
    }
  }
  return DIG_OK;
}

int dig_addattn_bwd(const void* xproj_, const void* sproj_, const float* w, const void* x_, const float* alpha, const void* dctx_, int ldd, float* dv,
                    void* dsproj_, float* dw_acc, int B, int N, int A, int X, hipStream_t) {
  if (int rc = dig_rules::addattn_bwd(xproj_, sproj_, w, x_, alpha, dctx_, ldd, dv, dsproj_, dw_acc, B, N, A, X)) return rc;
  const bf16_t* xproj = (const bf16_t*)xproj_; const bf16_t* sproj = (const bf16_t*)sproj_; const bf16_t* x = (const bf16_t*)x_;
  const bf16_t* dctx = (const bf16_t*)dctx_;
  bf16_t* dsproj = (bf16_t*)dsproj_;
#pragma omp parallel for
  for (int b = 0; b < B; ++b) {
    std::vector<float> g(N);
    float dot = 0.f;
    for (int n = 0; n < N; ++n) {
      float acc = 0.f;
      for (int c = 0; c < X; ++c) acc += bf2f(dctx[(size_t)b * ldd + c]) * bf2f(x[((size_t)b * N + n) * X + c]);
      g[n] = acc;
      dot += alpha[(size_t)b * N + n] * acc;
    }
    for (int n = 0; n < N; ++n) { g[n] = alpha[(size_t)b * N + n] * (g[n] - dot); dv[(size_t)b * N + n] = g[n]; }
    for (int a = 0; a < A; ++a) {
      float ga = 0.f, wa = 0.f;
      const float sp = bf2f(sproj[(size_t)b * A + a]);
      for (int n = 0; n < N; ++n) {
        const float t = std::tanh(sp + bf2f(xproj[((size_t)b * N + n) * A + a]));
        ga += g[n] * (1.f - t * t);
        wa += g[n] * t;
      }
      dsproj[(size_t)b * A + a] = f2bf(ga * w[a]);
      dw_acc[(size_t)b * A + a] += wa;
    }
  }
  return DIG_OK;
}

int dig_addattn_bwd_tokens(const void* xproj_, const void* sproj_all_, const float* w, const float* dv_all, const float* alpha_all,
                           const void* dctx_all_, int ldd, void* dxproj_, void* dx_, int T, int B, int N, int A, int X, hipStream_t) {
  if (int rc = dig_rules::addattn_bwd_tokens(xproj_, sproj_all_, w, dv_all, alpha_all, dctx_all_, ldd, dxproj_, dx_, T, B, N, A, X)) return rc;
  const bf16_t* xproj = (const bf16_t*)xproj_; const bf16_t* sproj_all = (const bf16_t*)sproj_all_; const bf16_t* dctx_all = (const bf16_t*)dctx_all_;
  bf16_t* dxproj = (bf16_t*)dxproj_; bf16_t* dx = (bf16_t*)dx_;
#pragma omp parallel for collapse(2)
  for (int b = 0; b < B; ++b)
    for (int n = 0; n < N; ++n) {
      for (int a = 0; a < A; ++a) {
        const float xv = bf2f(xproj[((size_t)b * N + n) * A + a]);
        float g = 0.f;
        for (int t = 0; t < T; ++t) {
          const float th = std::tanh(bf2f(sproj_all[((size_t)t * B + b) * A + a]) + xv);
          g += dv_all[((size_t)t * B + b) * N + n] * (1.f - th * th);
        }
        dxproj[((size_t)b * N + n) * A + a] = f2bf(g * w[a]);
      }
      for (int c = 0; c < X; ++c) {
        float g = 0.f;
        for (int t = 0; t < T; ++t) g += alpha_all[((size_t)t * B + b) * N + n] * bf2f(dctx_all[((size_t)t * B + b) * ldd + c]);
        dx[((size_t)b * N + n) * X + c] = f2bf(g);
      }
    }
  return DIG_OK;
}

int dig_gru_cell_fwd(const void* gi_, const void* gh_, const float* s_prev, float* s, void* s_bf16, float* gates, int B, int S, hipStream_t) {
  if (int rc = dig_rules::gru_cell_fwd(gi_, gh_, s_prev, s, s_bf16, gates, B, S)) return rc;
  const bf16_t* gi = (const bf16_t*)gi_; const bf16_t* gh = (const bf16_t*)gh_;
  bf16_t* sb = (bf16_t*)s_bf16;
  auto sig = [](float x) { return 1.f / (1.f + std::exp(-x)); };
  for (int i = 0; i < B * S; ++i) {
    const int b = i / S, k = i - b * S;
    const size_t g0 = (size_t)b * 3 * S + k;
    const float hn = bf2f(gh[g0 + 2 * S]);
    const float r = sig(bf2f(gi[g0]) + bf2f(gh[g0]));
    const float z = sig(bf2f(gi[g0 + S]) + bf2f(gh[g0 + S]));
    const float n = std::tanh(bf2f(gi[g0 + 2 * S]) + r * hn);
    const float sp = s_prev ? s_prev[i] : 0.f;
    const float v = (1.f - z) * n + z * sp;
    s[i] = v;
    sb[i] = f2bf(v);
    float* gt = gates + (size_t)b * 4 * S + k;
    gt[0] = r; gt[S] = z; gt[2 * S] = n; gt[3 * S] = hn;
  }
  return DIG_OK;
}

int dig_gru_cell_bwd(const float* ds_a, const float* ds_b, const float* ds_c, const float* ds_d, const float* gates, const float* s_prev, void* dgi_,
                     void* dgh_, float* ds_prev, int B, int S, hipStream_t) {
  if (int rc = dig_rules::gru_cell_bwd(ds_a, ds_b, ds_c, ds_d, gates, s_prev, dgi_, dgh_, ds_prev, B, S)) return rc;
  bf16_t* dgi = (bf16_t*)dgi_; bf16_t* dgh = (bf16_t*)dgh_;
  for (int i = 0; i < B * S; ++i) {
    const int b = i / S, k = i - b * S;
    float ds = ds_a[i];
    if (ds_b) ds += ds_b[i];
    if (ds_c) ds += ds_c[i];
    if (ds_d) ds += ds_d[i];
    const float* gt = gates + (size_t)b * 4 * S + k;
    const float r = gt[0], z = gt[S], n = gt[2 * S], hn = gt[3 * S];
    const float sp = s_prev ? s_prev[i] : 0.f;
    const float dn = ds * (1.f - z), dz = ds * (sp - n);
    const float dpre = dn * (1.f - n * n);
    const float dr = dpre * hn;
    const float gr = dr * r * (1.f - r), gz = dz * z * (1.f - z);
    const size_t g0 = (size_t)b * 3 * S + k;
    dgi[g0] = f2bf(gr); dgi[g0 + S] = f2bf(gz); dgi[g0 + 2 * S] = f2bf(dpre);
    dgh[g0] = f2bf(gr); dgh[g0 + S] = f2bf(gz); dgh[g0 + 2 * S] = f2bf(dpre * r);
    ds_prev[i] = ds * z;
  }
  return DIG_OK;
}

int dig_embed_rows(const long long* tokens, const float* table, void* out_, int ld, int rows, int cols, int vocab, hipStream_t) {
  if (int rc = dig_rules::embed_rows(tokens, table, out_, ld, rows, cols, vocab)) return rc;
  bf16_t* out = (bf16_t*)out_;
  for (int r = 0; r < rows; ++r) {
    const long long t = clamp_tok(tokens[r], vocab);
    for (int c = 0; c < cols; ++c) out[(size_t)r * ld + c] = f2bf(table[(size_t)t * cols + c]);
  }
  return DIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- CTC head (csrc/ctc.hip)
// The textbook recursions over the 2n + 1 states of the extended label sequence, in double and in log space (the device works in fp32
// re-centred every step: fp32 round-off class).

static double ctc_lse(double a, double b) {
  const double m = std::max(a, b);
  if (m == -std::numeric_limits<double>::infinity()) return m;
  return m + std::log(std::exp(a - m) + std::exp(b - m));
}

// Sample b: its extended sequence ext (2n + 1 states), the log-softmax lp [T][C] and alpha [T][S]; returns false for a sample that
// counts as nll = 0 (no alignment, or a label that is no class / the blank).
static bool ctc_forward(const float* x, int ld, const long long* tgt, long long tl, int ldt, int T, int C, int blank, std::vector<int>& ext,
                        std::vector<double>& lp, std::vector<double>& alpha, double& logp) {
  const double NINF = -std::numeric_limits<double>::infinity();
  const int n = (int)std::clamp(tl, 0LL, (long long)ldt);
  int rep = 0;
  for (int i = 0; i < n; ++i) {
    if (tgt[i] < 0 || tgt[i] >= C || tgt[i] == blank) return false;
    if (i && tgt[i] == tgt[i - 1]) ++rep;
  }
  if (n + rep > T) return false;
  const int S = 2 * n + 1;
  ext.assign(S, blank);
  for (int i = 0; i < n; ++i) ext[2 * i + 1] = (int)tgt[i];
  lp.assign((size_t)T * C, 0.0);
  for (int t = 0; t < T; ++t) {
    const float* row = x + (size_t)t * ld;
    double m = row[0], s = 0.0;
    for (int c = 1; c < C; ++c) m = std::max(m, (double)row[c]);
    for (int c = 0; c < C; ++c) s += std::exp((double)row[c] - m);
    const double l = m + std::log(s);
    for (int c = 0; c < C; ++c) lp[(size_t)t * C + c] = (double)row[c] - l;
  }
  alpha.assign((size_t)T * S, NINF);
  alpha[0] = lp[blank];
  if (n) alpha[1] = lp[ext[1]];
  for (int t = 1; t < T; ++t)
    for (int s = 0; s < S; ++s) {
      double a = alpha[(size_t)(t - 1) * S + s];
      if (s >= 1) a = ctc_lse(a, alpha[(size_t)(t - 1) * S + s - 1]);
      if (s >= 2 && (s & 1) && ext[s] != ext[s - 2]) a = ctc_lse(a, alpha[(size_t)(t - 1) * S + s - 2]);
      alpha[(size_t)t * S + s] = a + lp[(size_t)t * C + ext[s]];
    }
  logp = alpha[(size_t)(T - 1) * S + S - 1];
  if (n) logp = ctc_lse(logp, alpha[(size_t)(T - 1) * S + S - 2]);
  return logp > NINF && logp == logp;
}

int dig_ctc_loss(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset, int B, int T,
                 int C, int blank, float* nll, float* loss, hipStream_t) {
  if (int rc = dig_rules::ctc_loss(logits, ld, target, ldt, target_len, len_offset, B, T, C, blank, nll, loss)) return rc;
  if (B == 0) return DIG_OK;
  std::vector<int> ext;
  std::vector<double> lp, alpha;
  double total = 0.0;
  for (int b = 0; b < B; ++b) {
    double logp = 0.0;
    const bool ok = ctc_forward(logits + (size_t)b * T * ld, ld, target + (size_t)b * ldt, target_len[b] - (long long)len_offset, ldt, T, C, blank,
                                ext, lp, alpha, logp);
    nll[b] = ok ? (float)(-logp) : 0.f;
    total += (double)nll[b];
  }
  loss[0] = (float)(total / (double)B);
  return DIG_OK;
}

int dig_ctc_loss_bwd(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset,
                     const float* gscalar, int B, int T, int C, int blank, void* dlogits, int ldd, int dlogits_is_f32, hipStream_t) {
  if (int rc = dig_rules::ctc_loss_bwd(logits, ld, target, ldt, target_len, len_offset, gscalar, B, T, C, blank, dlogits, ldd, dlogits_is_f32)) return
      rc;
  if (B == 0) return DIG_OK;
  const double NINF = -std::numeric_limits<double>::infinity();
  const float sc = (gscalar ? gscalar[0] : 1.f) * (1.0f / (float)B);
  std::vector<int> ext;
  std::vector<double> lp, alpha, beta, occ;
  for (int b = 0; b < B; ++b) {
    float* d32 = (float*)dlogits + (size_t)b * T * ldd;
    bf16_t* d16 = (bf16_t*)dlogits + (size_t)b * T * ldd;
    double logp = 0.0;
    const bool ok = ctc_forward(logits + (size_t)b * T * ld, ld, target + (size_t)b * ldt, target_len[b] - (long long)len_offset, ldt, T, C, blank,
                                ext, lp, alpha, logp);
    const int S = (int)ext.size();
    if (ok) {
      beta.assign((size_t)T * S, NINF);
      beta[(size_t)(T - 1) * S + S - 1] = lp[(size_t)(T - 1) * C + blank];
      if (S > 1) beta[(size_t)(T - 1) * S + S - 2] = lp[(size_t)(T - 1) * C + ext[S - 2]];
      for (int t = T - 2; t >= 0; --t)
        for (int s = 0; s < S; ++s) {
          double a = beta[(size_t)(t + 1) * S + s];
          if (s + 1 < S) a = ctc_lse(a, beta[(size_t)(t + 1) * S + s + 1]);
          if (s + 2 < S && (s & 1) && ext[s] != ext[s + 2]) a = ctc_lse(a, beta[(size_t)(t + 1) * S + s + 2]);
          beta[(size_t)t * S + s] = a + lp[(size_t)t * C + ext[s]];
        }
    }
    for (int t = 0; t < T; ++t) {
      occ.assign(C, 0.0);
      if (ok)
        for (int s = 0; s < S; ++s) {
          const double v = alpha[(size_t)t * S + s] + beta[(size_t)t * S + s];
          if (v > NINF) occ[ext[s]] += std::exp(v - lp[(size_t)t * C + ext[s]] - logp);
        }
      for (int c = 0; c < ldd; ++c) {
        const float v = (ok && c < C) ? sc * (float)(std::exp(lp[(size_t)t * C + c]) - occ[c]) : 0.f;
        if (dlogits_is_f32) d32[(size_t)t * ldd + c] = v; else d16[(size_t)t * ldd + c] = f2bf(v);
      }
    }
  }
  return DIG_OK;
}

// Forced alignment, the rule of include/dig_hip.h as written: v [T][S] in double over the double log-softmax, one choice per cell (0 stay,
// 1 step, 2 skip: the number of states the back-trace moves down), a later predecessor taken only when strictly larger.
int dig_ctc_align(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset, int B, int T,
                  int C, int blank, int* start, int* end, float* char_logp, float* path_logp, int* frame_label, hipStream_t) {
  if (int rc = dig_rules::ctc_align(logits, ld, target, ldt, target_len, len_offset, B, T, C, blank, start, end, char_logp, path_logp, frame_label))
    return rc;
  const double NINF = -std::numeric_limits<double>::infinity();
  std::vector<int> ext, state(T);
  std::vector<double> lp, alpha, v;
  std::vector<unsigned char> choice;
  for (int b = 0; b < B; ++b) {
    int* st = start + (size_t)b * ldt;
    int* en = end + (size_t)b * ldt;
    float* cl = char_logp + (size_t)b * ldt;
    int* fr = frame_label ? frame_label + (size_t)b * T : nullptr;
    for (int k = 0; k < ldt; ++k) { st[k] = en[k] = -1; cl[k] = 0.f; }
    double logp = 0.0;
    bool ok = ctc_forward(logits + (size_t)b * T * ld, ld, target + (size_t)b * ldt, target_len[b] - (long long)len_offset, ldt, T, C, blank, ext,
                          lp, alpha, logp);
    const int S = (int)ext.size(), n = S / 2;
    int s = 0;
    if (ok) {
      v.assign((size_t)T * S, NINF);
      choice.assign((size_t)T * S, 0);
      v[0] = lp[blank];
      if (n) v[1] = lp[ext[1]];
      for (int t = 1; t < T; ++t)
        for (int q = 0; q < S; ++q) {
          const double* p = &v[(size_t)(t - 1) * S];
          double m = p[q];
          unsigned char c = 0;
          if (q >= 1 && p[q - 1] > m) { m = p[q - 1]; c = 1; }
          if (q >= 3 && (q & 1) && ext[q] != ext[q - 2] && p[q - 2] > m) { m = p[q - 2]; c = 2; }
          v[(size_t)t * S + q] = m + lp[(size_t)t * C + ext[q]];
          choice[(size_t)t * S + q] = c;
        }
      const double* last = &v[(size_t)(T - 1) * S];
      s = (n && last[S - 2] > last[S - 1]) ? S - 2 : S - 1;
      ok = last[s] > NINF;
      if (ok) path_logp[b] = (float)last[s];
    }
    if (!ok) {
      path_logp[b] = -std::numeric_limits<float>::infinity();
      for (int t = 0; fr && t < T; ++t) fr[t] = -2;
      continue;
    }
    for (int t = T - 1; t >= 0; --t) {
      state[t] = s;
      if (t) s -= choice[(size_t)t * S + s];
    }
    std::vector<double> sum(n, 0.0);
    for (int t = 0; t < T; ++t) {
      const int q = state[t], k = q >> 1;
      if (fr) fr[t] = (q & 1) ? k : -1;
      if (!(q & 1)) continue;
      if (st[k] < 0) st[k] = t;
      en[k] = t + 1;
      sum[k] += lp[(size_t)t * C + ext[q]];
    }
    for (int k = 0; k < n; ++k) cl[k] = (float)sum[k];
  }
  return DIG_OK;
}

int dig_ctc_greedy_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, long long* ids, float* score,
                          int* n, hipStream_t) {
  if (int rc = dig_rules::ctc_greedy_decode(logits, ld, B, T, C, blank, eos, padding, ids, score, n)) return rc;
  for (int b = 0; b < B; ++b) {
    long long* idr = ids + (size_t)b * (T + 1);
    float* scr = score + (size_t)b * (T + 1);
    int cnt = 0, prev = -1;
    for (int t = 0; t < T; ++t) {
      const float* row = logits + ((size_t)b * T + t) * ld;
      int am = 0;
      for (int c = 1; c < C; ++c)
        if (row[c] > row[am]) am = c;                                  // (the first maximum: the lowest id on a tie)
      float e = 0.f;
      for (int c = 0; c < C; ++c) e += std::exp(row[c] - row[am]);
      if (am != blank && am != eos && !(t > 0 && am == prev)) { idr[cnt] = am; scr[cnt] = 1.f / e; ++cnt; }
      prev = am;
    }
    for (int j = cnt; j <= T; ++j) { idr[j] = j == cnt ? eos : padding; scr[j] = 1.f; }
    n[b] = cnt;
  }
  return DIG_OK;
}

// Prefix beam search, the rule of include/dig_hip.h as written: a candidate table keyed by the prefix (an ordered map from the prefix's
// bytes to its row; rows in creation order), double recursions, a stable sort by tot for the selection.
int dig_ctc_beam_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, int beam_width, long long* ids,
                        float* score, float* logp, int* n, hipStream_t) {
  if (int rc = dig_rules::ctc_beam_decode(logits, ld, B, T, C, blank, eos, padding, beam_width, ids, score, logp, n)) return rc;
  const double NINF = -std::numeric_limits<double>::infinity();
  struct Hyp { std::string p; double lb, ln, tot; };
  std::vector<double> lp(C);
  for (int b = 0; b < B; ++b) {
    std::vector<Hyp> beam{{std::string(), 0.0, NINF, 0.0}};
    for (int t = 0; t < T; ++t) {
      const float* row = logits + ((size_t)b * T + t) * ld;
      double m = row[0], s = 0.0;
      for (int c = 1; c < C; ++c) m = std::max(m, (double)row[c]);
      for (int c = 0; c < C; ++c) s += std::exp((double)row[c] - m);
      const double l = m + std::log(s);
      for (int c = 0; c < C; ++c) lp[c] = (double)row[c] - l;
      std::vector<Hyp> cand;
      std::map<std::string, int> at;
      auto cell = [&](const std::string& p) -> Hyp& {
        auto it = at.find(p);
        if (it == at.end()) {
          it = at.emplace(p, (int)cand.size()).first;
          cand.push_back({p, NINF, NINF, NINF});
        }
        return cand[it->second];
      };
      for (const Hyp& h : beam) {
        const int last = h.p.empty() ? -1 : (int)(unsigned char)h.p.back();
        {
          Hyp& k = cell(h.p);
          k.lb = ctc_lse(k.lb, h.tot + lp[blank]);
          if (last >= 0) k.ln = ctc_lse(k.ln, h.ln + lp[last]);
        }
        for (int c = 0; c < C; ++c) {
          if (c == blank) continue;
          Hyp& k = cell(h.p + (char)(unsigned char)c);
          k.ln = ctc_lse(k.ln, (c == last ? h.lb : h.tot) + lp[c]);
        }
      }
      for (Hyp& k : cand) k.tot = ctc_lse(k.lb, k.ln);
      std::stable_sort(cand.begin(), cand.end(), [](const Hyp& a, const Hyp& b_) { return a.tot > b_.tot; });
      if ((int)cand.size() > beam_width) cand.resize(beam_width);
      beam.swap(cand);
    }
    long long* idr = ids + (size_t)b * (T + 1);
    float* scr = score + (size_t)b * (T + 1);
    int cnt = 0;
    for (unsigned char ch : beam[0].p)
      if ((int)ch != eos) idr[cnt++] = ch;
    for (int j = cnt; j <= T; ++j) idr[j] = j == cnt ? eos : padding;
    logp[b] = (float)beam[0].tot;
    for (int j = 0; j <= T; ++j) scr[j] = j == 0 ? (float)std::exp((double)logp[b]) : 1.f;
    n[b] = cnt;
  }
  return DIG_OK;
}

// Lexicon decode, the rule of include/dig_hip.h as written: per sample the frames' log-softmax once (double differences and sum,
// rounded to fp32), per word the device's recursion (fp32 in log space, re-centred every frame, the removed maxima summed in double),
// and a strict "greater" scan in range order for the first best word.
static float ctc_lse2f(float a, float b) {
  const float m = std::max(a, b);
  if (m == -std::numeric_limits<float>::infinity()) return m;
  return m + std::log(std::exp(a - m) + std::exp(b - m));
}
static float ctc_lse3f(float a, float b, float c) {
  const float m = std::max(std::max(a, b), c);
  if (m == -std::numeric_limits<float>::infinity()) return m;
  return m + std::log(std::exp(a - m) + std::exp(b - m) + std::exp(c - m));
}

// log p(word | the T x C log-softmax table lp), -inf for a word that cannot be scored
static float ctc_lex_word_score(const float* lp, int T, int C, int blank, const int* lab, int n) {
  const float NINF = -std::numeric_limits<float>::infinity();
  int rep = 0;
  for (int i = 0; i < n; ++i) {
    if (lab[i] < 0 || lab[i] >= C || lab[i] == blank) return NINF;
    if (i && lab[i] == lab[i - 1]) ++rep;
  }
  if (n + rep > T) return NINF;
  float ab[64], al[64], nb[64], nl[64];                                 // state 2i (the blank in front of label i; i = n: the last blank), 2i + 1
  for (int i = 0; i <= n; ++i) ab[i] = al[i] = NINF;
  ab[0] = lp[blank];
  if (n) al[0] = lp[lab[0]];
  double off = 0.0;
  for (int t = 0; t < T; ++t) {
    const float* row = lp + (size_t)t * C;
    if (t) {
      for (int i = 0; i <= n; ++i) {
        const float pl = i ? al[i - 1] : NINF;
        nb[i] = ctc_lse2f(ab[i], pl) + row[blank];
        nl[i] = i < n ? ctc_lse3f(al[i], ab[i], (i && lab[i] == lab[i - 1]) ? NINF : pl) + row[lab[i]] : NINF;
      }
      for (int i = 0; i <= n; ++i) { ab[i] = nb[i]; al[i] = nl[i]; }
    }
    float m = NINF;
    for (int i = 0; i <= n; ++i) m = std::max(m, std::max(ab[i], al[i]));
    for (int i = 0; i <= n; ++i) { ab[i] -= m; al[i] -= m; }
    off += (double)m;
  }
  const float tail = ctc_lse2f(ab[n], n ? al[n - 1] : NINF);
  const double logp = off + (double)tail;
  return (tail > NINF && logp == logp && logp > -1e300) ? (float)logp : NINF;
}

using dig_rules::ctc_lex_chunks;

int dig_ctc_lexicon_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, const int* words,
                           const int* word_len, int ldw, int W, const int* lex_begin, const int* lex_count, int max_count, int* best_index,
                           float* logp, long long* ids, float* score, int* n, float* scores, void* workspace, long long workspace_bytes,
                           hipStream_t) {
  if (int rc = dig_rules::ctc_lexicon_decode(logits, ld, B, T, C, blank, eos, padding, words, word_len, ldw, W, lex_begin, lex_count, max_count,
                                             best_index, logp, ids, score, n, scores, workspace, workspace_bytes))
    return rc;
  if (B == 0) return DIG_OK;
  const float NINF = -std::numeric_limits<float>::infinity();
  std::vector<float> lp((size_t)T * C);
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < T; ++t) {
      const float* row = logits + ((size_t)b * T + t) * ld;
      float m = row[0];
      for (int c = 1; c < C; ++c) m = std::max(m, row[c]);
      double e = 0.0;
      for (int c = 0; c < C; ++c) e += (double)std::exp((float)((double)row[c] - (double)m));
      const double ls = std::log(e);
      for (int c = 0; c < C; ++c) lp[(size_t)t * C + c] = (float)((double)row[c] - (double)m - ls);
    }
    const int begin = std::clamp(lex_begin[b], 0, W);
    const int count = std::clamp(lex_count[b], 0, std::min(W - begin, max_count));
    int best = -1;
    float bs = NINF;
    for (int j = 0; j < max_count; ++j) {
      float s = NINF;
      if (j < count) {
        const int w = begin + j;
        s = ctc_lex_word_score(lp.data(), T, C, blank, words + (size_t)w * ldw, std::clamp(word_len[w], 0, ldw));
        if (s > bs) { bs = s; best = w; }                               // (strict: the first of equal scores)
      }
      if (scores) scores[(size_t)b * max_count + j] = s;
    }
    const int len = best < 0 ? 0 : std::clamp(word_len[best], 0, std::min(ldw, T));
    long long* idr = ids + (size_t)b * (T + 1);
    float* scr = score + (size_t)b * (T + 1);
    for (int j = 0; j <= T; ++j) {
      idr[j] = j < len ? (long long)words[(size_t)best * ldw + j] : (j == len ? eos : padding);
      scr[j] = j == 0 ? (best < 0 ? 0.f : (float)std::exp((double)bs)) : 1.f;
    }
    best_index[b] = best;
    logp[b] = bs;
    n[b] = len;
  }
  return DIG_OK;
}

}  // extern "C"
