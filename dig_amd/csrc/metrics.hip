// Evaluation metrics (evaluation_metric/metrics.py of the reference): string accuracy and character F-measure of label rows, normalised
// strings as code points, Levenshtein distance of pairs, the lexicon search (nearest word of a range, first minimum) and the confidence
// of a prediction.  Integer VALU + LDS work; no matrix cores.
#include "common.h"

namespace {

constexpr int LEV_MAX = DIG_LEV_MAX_LEN;                 // longest string either side
constexpr int LEX_CHUNK = DIG_LEXICON_CHUNK;             // words per workgroup of the search = one wave, one word per lane

// Levenshtein distance (unit costs) of x[0..xlen) and y[0..ylen), one pair per lane.  The DP row runs over y: cell j = distance of the
// prefix of x read so far to y[0..j).  Cell 0 is the number of x characters read and stays in a register; cells 1..ylen live in LDS as
// 16-bit halves, two per dword (dword p = cells 2p+1 | 2p+2 << 16), lane-minor: row[p * 64 + lane], so a wave's ds_read_b32 /
// ds_write_b32 fall on distinct banks.  Values never exceed 128.  `row` needs ((cap + 1) / 2) * 64 dwords for ylen <= cap.
// When y is the same for the whole wave (the search) its reads are uniform and come through the scalar cache.
__device__ __forceinline__ int lev_lane(const int* __restrict__ x, int xlen, const int* __restrict__ y, int ylen, unsigned* __restrict__ row,
                                        int lane) {
  if (ylen == 0) return xlen;
  const int np = (ylen + 1) >> 1;
  for (int p = 0; p < np; ++p) row[p * 64 + lane] = (unsigned)(2 * p + 1) | ((unsigned)(2 * p + 2) << 16);
  for (int i = 0; i < xlen; ++i) {
    const int c = x[i];
    unsigned diag = (unsigned)i, left = (unsigned)i + 1u;
    for (int p = 0; p < np; ++p) {
      const unsigned v = row[p * 64 + lane];
      const unsigned o1 = v & 0xffffu, o2 = v >> 16;
      const int y1 = y[2 * p];
      const int y2 = (2 * p + 1 < ylen) ? y[2 * p + 1] : y1;                  // (the half past an odd ylen is never read back)
      const unsigned n1 = min(min(o1, left) + 1u, diag + (c != y1 ? 1u : 0u));
      const unsigned n2 = min(min(o2, n1) + 1u, o1 + (c != y2 ? 1u : 0u));
      row[p * 64 + lane] = n1 | (n2 << 16);
      diag = o2;
      left = n2;
    }
  }
  const unsigned v = row[((ylen - 1) >> 1) * 64 + lane];
  return (int)(((ylen - 1) & 1) ? (v >> 16) : (v & 0xffffu));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, o, 64), hi = __shfl_xor((unsigned)(k >> 32), o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    k = other < k ? other : k;
  }
  return k;
}

constexpr unsigned long long LEX_NONE = ~0ull;

// Accuracy (evaluation_metric/metrics.py:19-81): both label rows are cut at EOS, UNKNOWN and every class that is not a digit
// or letter are dropped, letters compare case-insensitively.  canon[c] = canonical code of class c (0 = dropped, EOS and
// UNKNOWN included).  One thread per sample; match[b] = 1 when the normalised strings are equal.
__global__ void string_match_kernel(const long long* __restrict__ pred, const long long* __restrict__ target,
                                    const unsigned char* __restrict__ canon, int n_classes, int eos, int B, int T,
                                    unsigned char* __restrict__ match) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long* p = pred + (size_t)b * T;
  const long long* t = target + (size_t)b * T;
  int i = 0, j = 0;
  bool ok = true;
  while (ok) {
    unsigned char a = 0, c = 0;
    while (i < T && p[i] != eos) {                                      // next kept character of the prediction
      const long long v = p[i++];
      a = (v >= 0 && v < n_classes) ? canon[v] : 0;
      if (a) break;
    }
    if (i < T && p[i] == eos && !a) i = T;
    while (j < T && t[j] != eos) {
      const long long v = t[j++];
      c = (v >= 0 && v < n_classes) ? canon[v] : 0;
      if (c) break;
    }
    if (j < T && t[j] == eos && !c) j = T;
    if (a != c) ok = false;
    if (!a && !c) break;                                                // both strings ended
  }
  match[b] = ok ? 1 : 0;
}

// recognition_f_measure (evaluation_metric/metrics.py:83-100): per sample, the SETS of kept characters of prediction and target
// (same cut / drop / case-fold rules as the accuracy; canon codes 1..63 -> one bit each), p = n/(|P|+1e-5), r = n/(|T|+1e-5),
// f = 2pr/(p+r+1e-5), all in double as the reference's Python floats.
__global__ void char_fmeasure_kernel(const long long* __restrict__ pred, const long long* __restrict__ target,
                                     const unsigned char* __restrict__ canon, int n_classes, int eos, int B, int T,
                                     double* __restrict__ f_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  unsigned long long ps = 0, ts = 0;
  for (int i = 0; i < T; ++i) {
    const long long v = pred[(size_t)b * T + i];
    if (v == eos) break;
    const unsigned char c = (v >= 0 && v < n_classes) ? canon[v] : 0;
    if (c) ps |= 1ull << (c & 63);
  }
  for (int i = 0; i < T; ++i) {
    const long long v = target[(size_t)b * T + i];
    if (v == eos) break;
    const unsigned char c = (v >= 0 && v < n_classes) ? canon[v] : 0;
    if (c) ts |= 1ull << (c & 63);
  }
  const double n = (double)__popcll(ps & ts);
  const double p = n / ((double)__popcll(ps) + 1e-5), r = n / ((double)__popcll(ts) + 1e-5);
  f_out[b] = 2 * p * r / (p + r + 1e-5);
}

// get_str_list + _normalize_text (metrics.py:14-64) of one tensor: one thread per row.
__global__ void tokens_to_text_kernel(const long long* __restrict__ tokens, const unsigned char* __restrict__ canon, int n_classes, int eos,
                                      int B, int T, int* __restrict__ text, int* __restrict__ len) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long* t = tokens + (size_t)b * T;
  int* o = text + (size_t)b * T;
  int n = 0;
  for (int i = 0; i < T; ++i) {
    const long long v = t[i];
    if (v == eos) break;
    const int c = (v >= 0 && v < n_classes) ? canon[v] : 0;
    if (c) o[n++] = c <= 10 ? '0' + (c - 1) : 'a' + (c - 11);
  }
  len[b] = n;
  for (int i = n; i < T; ++i) o[i] = 0;
}

// one pair per lane, one wave per workgroup; LDS: ((ldb + 1) / 2) * 64 dwords
__global__ __launch_bounds__(64) void edit_distance_kernel(const int* __restrict__ a, const int* __restrict__ a_len, int lda, int a_rows,
                                                           const int* __restrict__ a_index, const int* __restrict__ b,
                                                           const int* __restrict__ b_len, int ldb, int n, int* __restrict__ dist) {
  extern __shared__ unsigned lev_row[];
  const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
  if (i >= n) return;
  const int r = a_index ? a_index[i] : i;
  const bool have = r >= 0 && r < a_rows;                                       // a row outside `a` reads as the empty string
  const int alen = have ? clampi(a_len[r], 0, lda) : 0;
  const int blen = clampi(b_len[i], 0, ldb);
  dist[i] = lev_lane(a + (size_t)(have ? r : 0) * lda, alen, b + (size_t)i * ldb, blen, lev_row, lane);
}

// workgroup (chunk, query): lane l takes word lex_begin + chunk * 64 + l of the query's range and leaves the chunk's smallest
// (distance << 32 | pool index) in partial[query * n_chunks + chunk] (all ones: no word).  LDS: ((ldq + 1) / 2) * 64 dwords.
__global__ __launch_bounds__(64) void lexicon_search_kernel(const int* __restrict__ query, const int* __restrict__ query_len, int ldq,
                                                            const int* __restrict__ words, const int* __restrict__ word_len, int ldw, int W,
                                                            const int* __restrict__ lex_begin, const int* __restrict__ lex_count,
                                                            int max_count, int n_chunks, unsigned long long* __restrict__ partial) {
  extern __shared__ unsigned lev_row[];
  const int lane = threadIdx.x, q = blockIdx.y, chunk = blockIdx.x;
  const int begin = clampi(lex_begin[q], 0, W);
  const int count = clampi(lex_count[q], 0, min(W - begin, max_count));
  const int k = chunk * LEX_CHUNK + lane;
  unsigned long long key = LEX_NONE;
  if (k < count) {
    const int w = begin + k;
    const int qlen = clampi(query_len[q], 0, ldq);
    const int d = lev_lane(words + (size_t)w * ldw, clampi(word_len[w], 0, ldw), query + (size_t)q * ldq, qlen, lev_row, lane);
    key = ((unsigned long long)(unsigned)d << 32) | (unsigned)w;
  }
  key = wave_min_u64(key);
  if (lane == 0) partial[(size_t)q * n_chunks + chunk] = key;
}

// one wave per query: the smallest key over the query's chunks (a minimum over distinct keys: any order gives the same answer)
__global__ __launch_bounds__(64) void lexicon_fold_kernel(const unsigned long long* __restrict__ partial, int n_chunks, int* __restrict__ best_index,
                                                          int* __restrict__ best_dist) {
  const int lane = threadIdx.x, q = blockIdx.x;
  unsigned long long key = LEX_NONE;
  for (int c = lane; c < n_chunks; c += 64) {
    const unsigned long long o = partial[(size_t)q * n_chunks + c];
    key = o < key ? o : key;
  }
  key = wave_min_u64(key);
  if (lane == 0) {
    best_index[q] = key == LEX_NONE ? -1 : (int)(unsigned)key;
    best_dist[q] = key == LEX_NONE ? -1 : (int)(key >> 32);
  }
}

// RecPostProcess (metrics.py:195-200): one thread per row, double, index order
__global__ void seq_confidence_kernel(const float* __restrict__ score, const int* __restrict__ text_len, int B, int T, double* __restrict__ conf) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int tl = text_len[b];
  const int n = tl < 0 ? 0 : (tl >= T ? T : tl + 1);
  double s = 0.0;
  for (int j = 0; j < n; ++j) s += log((double)score[(size_t)b * T + j]);
  conf[b] = exp(s);
}

inline size_t lev_lds_bytes(int cap) { return (size_t)((cap + 1) / 2) * 64 * sizeof(unsigned); }

}  // namespace

// C-ABI: see include/dig_hip.h
extern "C" int dig_string_match(const long long* pred, const long long* target, const unsigned char* canon, int n_classes, int eos,
                                int B, int T, unsigned char* match, hipStream_t stream) {
  if (int rc = dig_rules::string_match(pred, target, canon, n_classes, eos, B, T, match)) return rc;
  hipLaunchKernelGGL(string_match_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, pred, target, canon, n_classes, eos, B, T, match);
  return dig_check_launch();
}

extern "C" int dig_char_fmeasure(const long long* pred, const long long* target, const unsigned char* canon, int n_classes, int eos,
                                 int B, int T, double* f_per_sample, hipStream_t stream) {
  if (int rc = dig_rules::char_fmeasure(pred, target, canon, n_classes, eos, B, T, f_per_sample)) return rc;
  hipLaunchKernelGGL(char_fmeasure_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, pred, target, canon, n_classes, eos, B, T, f_per_sample);
  return dig_check_launch();
}

extern "C" int dig_tokens_to_text(const long long* tokens, const unsigned char* canon, int n_classes, int eos, int B, int T, int* text,
                                  int* len, hipStream_t stream) {
  if (int rc = dig_rules::tokens_to_text(tokens, canon, n_classes, eos, B, T, text, len)) return rc;
  hipLaunchKernelGGL(tokens_to_text_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, tokens, canon, n_classes, eos, B, T, text, len);
  return dig_check_launch();
}

extern "C" int dig_edit_distance(const int* a, const int* a_len, int lda, int a_rows, const int* a_index, const int* b, const int* b_len,
                                 int ldb, int n, int* dist, hipStream_t stream) {
  if (int rc = dig_rules::edit_distance(a, a_len, lda, a_rows, a_index, b, b_len, ldb, n, dist)) return rc;
  hipLaunchKernelGGL(edit_distance_kernel, dim3((n + 63) / 64), dim3(64), lev_lds_bytes(ldb), stream, a, a_len, lda, a_rows, a_index, b, b_len,
                     ldb, n, dist);
  return dig_check_launch();
}


extern "C" int dig_lexicon_search(const int* query, const int* query_len, int ldq, int B, const int* words, const int* word_len, int ldw,
                                  int W, const int* lex_begin, const int* lex_count, int max_count, int* best_index, int* best_dist,
                                  void* workspace, long long workspace_bytes, hipStream_t stream) {
  if (int rc = dig_rules::lexicon_search(query, query_len, ldq, B, words, word_len, ldw, W, lex_begin, lex_count, max_count, best_index, best_dist,
                                         workspace, workspace_bytes))
    return rc;
  const int n_chunks = max_count == 0 ? 1 : (int)(((long long)max_count + LEX_CHUNK - 1) / LEX_CHUNK);
  unsigned long long* partial = (unsigned long long*)workspace;
  hipLaunchKernelGGL(lexicon_search_kernel, dim3(n_chunks, B), dim3(64), lev_lds_bytes(ldq), stream, query, query_len, ldq, words, word_len,
                     ldw, W, lex_begin, lex_count, max_count, n_chunks, partial);
  hipLaunchKernelGGL(lexicon_fold_kernel, dim3(B), dim3(64), 0, stream, partial, n_chunks, best_index, best_dist);
  return dig_check_launch();
}

extern "C" int dig_seq_confidence(const float* score, const int* text_len, int B, int T, double* conf, hipStream_t stream) {
  if (int rc = dig_rules::seq_confidence(score, text_len, B, T, conf)) return rc;
  hipLaunchKernelGGL(seq_confidence_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, score, text_len, B, T, conf);
  return dig_check_launch();
}
