// The argument rules of the C ABI (include/dig_hip.h), written once for both builds: libdig_hip.so (csrc/*.hip, the product) and the
// plain-C++ build of cpu_abi/ (the second opinion of the operator tests).  For every entry point that refuses calls of its own there is
// one dig_rules::NAME(arguments without the stream) here, returning DIG_OK or the refusal code (DIG_ERR_ARG / DIG_ERR_ALIGN /
// DIG_ERR_UNSUPPORTED), the rules applied in the order the HIP build has always applied them, so a call with two faults keeps its code.
// Every entry point of either build opens with `if (int rc = dig_rules::NAME(...)) return rc;` and holds no rule of its own; thin
// forwarding entry points (dig_gemm_bf16 -> dig_gemm_bf16_dropout, ...) inherit the rules of the entry point they forward to.
//
// A rule is a pure function of its arguments: it may read a dig_dropout_t, a dig_abi_run or a host descriptor table passed by pointer
// and never touches tensor memory.  Sizes a rule compares against a limit (rows per split, LDS bytes, instantiated kernel forms) come
// from helpers here that the launchers use too, in 64-bit arithmetic where an int product could overflow.  The host-only queries whose
// formula is the same in both builds are inline functions here as well; their extern "C" definitions are abi_queries.inc.
// Per build by nature (each describes its own build's partial-sum layout): dig_bn_stats_workspace_bytes, dig_colsum_workspace_bytes.
//
// Plain C++17, no HIP runtime call and no device code: g++ compiles this file unchanged (tests/abi_rules_main.cpp checks the magnitude
// rules that way under the address and undefined-behaviour sanitizers).  Limits that Python reads through _lib.const stay #defines of
// dig_hip.h; every other limit a rule names is a constant below, and the .hip files take their copies from here.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/dig_hip.h"

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
static inline bool aligned8(const void* p) { return (((uintptr_t)p) & 7u) == 0; }
// [a, a + bytes) and [b, b + bytes) share a byte
static inline bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

namespace dig_rules {

// ---- limits
constexpr int LDS_LIMIT = 160 * 1024;            // dynamic LDS of one workgroup (bytes)
constexpr unsigned long long OFFSET_LIMIT = 1ull << 32;   // byte / element offsets the kernels hold in 32 bits
constexpr int ATTN_TOKENS = 256, ATTN_HEAD_DIM = 64;      // encoder attention: tokens per image, head width
constexpr int ATTN_BWD_PROJ_MAX_DIM = 512;
constexpr int ATTN_BLOCK_DIM = 384, ATTN_BLOCK_HEADS = 6; // the one-launch attention block
constexpr int GEMM_BR = 64;                      // granule of the GEMM's reduction dim
constexpr int CHAIN_DIM = 384, CHAIN_FC = 64, CHAIN_ROWS = 128, CHAIN_SLOT = 16384;   // fused MLP: width, chunk, rows per workgroup, LDS slot
constexpr int CHAIN_MAX_F = 6144, CHAIN_LN_MAX_F = 2048;
constexpr int BN_FUSED_COLS = 32, BN_FUSED_MAX_ROWS = 4096, BN_FUSED_MIN_C = 256;
constexpr int PATCH_EMBED_MAX_D = 1024;
constexpr int RANDOM_MASKS_MAX_PATCHES = 16384;
constexpr int TRANSPOSE_MAX = 32;                // matrices of one dig_transpose_bf16_multi
constexpr int SEQ_ATTN_MAX_LQ = 32, SEQ_ATTN_MAX_LK = 512;
constexpr int SEQ_EMBED_BWD_LDS = 60 * 1024;     // token ids of one launch, in LDS
constexpr int DECODE_MAX_MEM = 8192;
constexpr int BEAM_STEP_MAX_WIDTH = 16, BEAM_ADVANCE_MAX_WIDTH = 8, BEAM_LDS = 60000;
constexpr int ADDATTN_MAX_A = 1024, ADDATTN_MAX_N = 512, ADDATTN_MAX_SLOTS = 8, ADDATTN_BWD_TOKENS_LDS = 150 * 1024;
constexpr int TCV_MAXN = 256, TCV_MAXQ = 32;
constexpr int CTC_MAX_T = 64, CTC_MAX_C = 256, CTC_MAX_LDT = 63, CTC_MAX_W = 32;
constexpr int GRID_Y_MAX = 65535;                // samples of a launch that puts them on gridDim.y

// a * b >= limit without forming a product that could wrap (a, b >= 0)
static inline bool prod_ge(unsigned long long a, unsigned long long b, unsigned long long limit) { return a && b >= (limit + a - 1) / a; }

// ---- host-only queries, one formula for both builds (extern "C" definitions: abi_queries.inc)
static inline long long gemm_rows_per_split(int R, int splits) {  // whole 64-row K tiles per split (64-bit: R near INT_MAX rounds up past it)
  const long long rtiles = ((long long)R + GEMM_BR - 1) / GEMM_BR;
  return ((rtiles + splits - 1) / splits) * GEMM_BR;
}
static inline int gemm_effective_splits(int R, int splits) {
  if (R <= 0 || splits < 1) return 0;
  const long long per = gemm_rows_per_split(R, splits);
  return (int)((R + per - 1) / per);
}
static inline int wgrad_group_supported(int I, int J, int R) {
  // (operands are addressed through 32-bit buffer offsets: R rows of at least I / J columns each must stay below 4 GiB -- the launcher
  //  checks the real leading dimensions again)
  return (I > 0 && J > 0 && R >= 64 && I % 128 == 0 && (J % 384 == 0 || J % 256 == 0) && R % 64 == 0 &&
          (unsigned long long)R * (unsigned)I * 2ull < OFFSET_LIMIT && (unsigned long long)R * (unsigned)J * 2ull < OFFSET_LIMIT) ? 1 : 0;
}
static inline int wgrad_group_fn(int J) { return J % 384 == 0 ? 3 : (J % 256 == 0 ? 2 : 0); }
// rows per R-split for a requested split count (whole groups of four 16-row stages), and the split count that results
static inline int wgrad_group_rows_per_split(int R, int splits) {
  if (R <= 0 || splits < 1 || R % 64) return 0;
  return (int)((((long long)R / 64 + splits - 1) / splits) * 64);
}
static inline int wgrad_group_effective_splits(int R, int splits) {
  const long long per = wgrad_group_rows_per_split(R, splits);
  return per ? (int)((R + per - 1) / per) : 0;
}
static inline long long wgrad_group_slab_bytes(int total_tiles, int splits, int fn, int wa) {
  return (long long)total_tiles * splits * 128 * wa * 128 * fn * 4;
}
// tiles of one problem: wa = 1: 128 x 128 fn (4 waves, two workgroups per CU);  wa = 2: 256 x 128 fn (8 waves, one workgroup per CU)
static inline int wgrad_group_tiles(int I, int J, int fn, int wa) {
  if (I <= 0 || J <= 0 || (fn != 2 && fn != 3) || (wa != 1 && wa != 2) || (I % 128) || (J % (128 * fn))) return 0;
  return (int)((((long long)I + 128 * wa - 1) / (128 * wa)) * (J / (128 * fn)));
}
// number of partial rows ([parts][3][D] fp32) the LayerNorm backward leaves in its workspace
static inline int layernorm_bwd_parts(int rows) {
  const long long p = ((long long)rows + 15) / 16;
  return (int)(p < 1 ? 1 : (p > 1024 ? 1024 : p));
}
static inline long long layernorm_bwd_workspace_bytes(int rows, int D) { return (long long)layernorm_bwd_parts(rows) * 3 * D * (long long)sizeof(float); }
static inline bool layernorm_dim_ok(int D) { return D == 64 || D == 128 || D == 192 || D == 256 || D == 384 || D == 512; }   // instantiated widths
// Few-row BatchNorm layers in one launch: 2 <= rows <= 4096, C >= 256 and a multiple of the 32-column slab
static inline int bn_fused_supported(int rows, int C) {
  return rows >= 2 && rows <= BN_FUSED_MAX_ROWS && C >= BN_FUSED_MIN_C && (C % BN_FUSED_COLS) == 0;
}
static inline int attn_block_supported(int heads, int embed_dim) { return (heads == ATTN_BLOCK_HEADS && embed_dim == ATTN_BLOCK_DIM) ? 1 : 0; }
static inline int mlp_chain_supported(int D, int F) { return D == CHAIN_DIM && F >= 2 * CHAIN_FC && F % (2 * CHAIN_FC) == 0 && F <= CHAIN_MAX_F; }
// partial rows dig_mlp_chain_bwd_ln writes into ln_partials ([rows][3][D] fp32): one per workgroup of 128 tokens
static inline int mlp_chain_ln_parts(int R) { return (int)(((long long)R + CHAIN_ROWS - 1) / CHAIN_ROWS); }
// partial rows dig_mlp_chain_bwd writes into colsum_partials ([rows][F] fp32)
static inline int mlp_chain_colsum_rows(int R) { return mlp_chain_ln_parts(R) * 4; }
// dynamic LDS of the fused MLP kernel.  mode 0: forward, 1: forward with the saved pre-activation, 2: backward; ln: the LayerNorm vectors
static inline long long mlp_chain_lds_bytes(int mode, bool ln, int F) {
  const long long vec = ((long long)F + CHAIN_DIM) * 4;
  return 7LL * CHAIN_SLOT + (mode == 0 ? vec : (mode == 1 ? CHAIN_SLOT + vec : 2LL * CHAIN_SLOT)) + (ln ? 4 * CHAIN_DIM * 4 : 0);
}
static inline long long lexicon_search_workspace_bytes(int B, int max_count) {
  if (B <= 0 || max_count < 0) return 0;
  const long long n_chunks = max_count == 0 ? 1 : ((long long)max_count + DIG_LEXICON_CHUNK - 1) / DIG_LEXICON_CHUNK;
  return (long long)B * n_chunks * (long long)sizeof(unsigned long long);
}
static inline long long ctc_lex_chunks(int max_count) { return ((long long)max_count + DIG_CTC_LEX_CHUNK - 1) / DIG_CTC_LEX_CHUNK; }
static inline long long ctc_lexicon_workspace_bytes(int B, int T, int C, int max_count) {
  if (B <= 0 || T <= 0 || C <= 0 || max_count < 0) return 0;
  const long long chunks = ctc_lex_chunks(max_count);
  const long long keys = (long long)B * (chunks < 1 ? 1 : chunks) * (long long)sizeof(unsigned long long);
  return keys + (long long)B * T * C * (long long)sizeof(float);
}
static inline long long sumsq_workspace_bytes(long long) { return 1024 * (long long)sizeof(float); }
// dig_mse_fwd_bwd_ws: the ticket word + one block sum per workgroup of its launch
constexpr int MSE_MAX_BLOCKS = 256;
static inline long long mse_workspace_bytes() { return (1 + MSE_MAX_BLOCKS) * (long long)sizeof(float); }
// dig_ce_rows_ws: the ticket word + the three sums of each row
static inline long long ce_rows_workspace_bytes(int n) { return n < 0 ? 0 : (1 + 3LL * n) * (long long)sizeof(float); }
// dig_tcv_attn_bwd: [S Lq][2d] each query row's share of (dlnc_g | dlnc_b), then [S Lq][heads] delta
static inline long long tcv_attn_bwd_workspace_bytes(int S, int Lq, int heads, int d) {
  if (S <= 0 || Lq <= 0 || Lq > TCV_MAXQ || heads <= 0 || d <= 0 || d > 512 || heads > d) return 0;   // (past these the entry point refuses; the product stays in 64 bits)
  return (long long)S * Lq * (2LL * d + heads) * (long long)sizeof(float);
}

// ---- sizes the launchers and the rules share
static inline long long sgemm_rows_per_split(int R, int r_splits) {  // whole 64-deep K steps per split
  return (((long long)R + r_splits - 1) / r_splits + 63) / 64 * 64;
}
static inline int sgemm_effective_splits(int R, int r_splits) {
  const long long per = sgemm_rows_per_split(R, r_splits);
  return (int)((R + per - 1) / per);
}
// taps per output index of one axis of the Pillow bicubic resize, for inputs up to in_size (64-bit: in_size / out_size is the caller's)
static inline long long resize_taps(int in_size, int out_size) {
  double fs = (double)in_size / out_size;
  if (fs < 1.0) fs = 1.0;
  long long c = (long long)(2.0 * fs);
  if ((double)c < 2.0 * fs) ++c;                                      // ceil
  return c * 2 + 1;
}
static inline int ksize_for(int in_size, int out_size) { return (int)resize_taps(in_size, out_size); }
// LDS bytes of the resize coefficient tables (dig_resize_bicubic_normalize_u8)
static inline size_t resize_lds_bytes(int out_h, int out_w, long long ksh, long long ksv) {
  return ((size_t)out_w * (size_t)(ksh + 2) + (size_t)out_h * (size_t)(ksv + 2)) * sizeof(int);
}
// dynamic LDS bytes of key-view stage B: the resize coefficient tables, four 8-byte contrast sums, the out_h x out_w x 3 image
static inline size_t stage_b_lds_bytes(int out_h, int out_w, long long ksh, long long ksv) {
  size_t ints = (size_t)out_w * (size_t)(ksh + 2) + (size_t)out_h * (size_t)(ksv + 2);
  ints += ints & 1;                                                                    // the sums start 8-byte aligned
  return ints * sizeof(int) + 4 * sizeof(unsigned long long) + 3 * (size_t)out_h * out_w;
}
// the ABINet tail: stage B without the pixel planes
static inline size_t abiaug_tail_lds_bytes(int out_h, int out_w, long long ksh, long long ksv) {
  return stage_b_lds_bytes(out_h, out_w, ksh, ksv) - 3 * (size_t)out_h * out_w;
}
static inline size_t addattn_bwd_tokens_lds_bytes(int T, int width) { return ((size_t)T * width + (size_t)T * 64) * 4; }
// LDS bytes of the sequence attention backward: Lk <= 384 / 430 / 512 at head dim 64 / 48 / 24 (head_dim and Lk within their limits)
static inline int seq_attn_bwd_lds_bytes(int head_dim, int Lk) { return 256 * head_dim + Lk * (256 + 2 * head_dim); }
static inline bool seq_head_dim_ok(int head_dim) { return head_dim == 24 || head_dim == 48 || head_dim == 64; }

// the packed [n_img, 256, 3 * embed_dim] bf16 qkv tensor is addressed through 32-bit byte offsets
static inline bool attn_qkv_bytes_over(int n_img, int embed_dim) {
  return prod_ge((unsigned long long)n_img * (unsigned long long)embed_dim, (unsigned long long)ATTN_TOKENS * 3 * 2, OFFSET_LIMIT);
}

// The GEMM forms (operand layouts, output kind, tile) that have a kernel instance without dropout -- the dispatch at the end of
// dig_gemm_bf16_dropout restated: every 128x128 form below, and the wide tiles (bk >= 200; a persistent tile runs as its
// one-tile-per-workgroup shape where the persistent kernel does not apply) for the starred ones as well.
static inline bool gemm_form_ok(int trans_a, int trans_b, int out_kind, int bk) {
  const bool ta = trans_a != 0, tb = trans_b != 0, wide = bk >= 200;
  if (!ta && !tb) return out_kind == 0 || out_kind == 1 || (out_kind == 2 && wide);   // (0, 0, 2)*
  if (!ta && tb) return out_kind == 0 || out_kind == 1 || (out_kind == 2 && wide);    // (0, 1, 2)*
  return ta && tb && out_kind == 2;                                                     // weight gradients: split-R slabs
}

static inline bool abi_run_ok(const dig_abi_run* r) {
  return r && r->geom_type >= 0 && r->geom_type <= 2 && r->noise_var >= 0 && r->mb_size >= 1 && r->mb_size <= DIG_ABI_MB_MAX &&
         r->rescale_factor >= 0 && r->rescale_factor <= 4;
}

// ---- rules shared by several entry points
static inline int mlp_chain_common(const void* x, const void* b1, const void* b2, const void* out, int R, int D, int F) {
  if (!x || !b1 || !b2 || !out || R <= 0) return DIG_ERR_ARG;
  if (D != CHAIN_DIM || F < 2 * CHAIN_FC || (F % (2 * CHAIN_FC))) return DIG_ERR_UNSUPPORTED;       // an even number of 64-wide chunks
  if (!aligned16(x) || !aligned16(b1) || !aligned16(b2) || !aligned16(out)) return DIG_ERR_ALIGN;
  if ((size_t)R * F * 2 >= OFFSET_LIMIT || (size_t)F * D * 2 >= (1ull << 31)) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
// the arguments of the ranking, as both beam entry points check them
static inline int beam_common(const float* logits, int ld, const float* seq_scores, int B, int beam_width, int max_width, int C,
                              const long long* symbols, const long long* predecessors, const float* stored_scores) {
  if (!logits || !seq_scores || !symbols || !predecessors || !stored_scores || B <= 0 || C <= 0 || ld < C) return DIG_ERR_ARG;
  if (beam_width < 1 || beam_width > max_width || (size_t)beam_width * C * sizeof(float) > BEAM_LDS) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int tcv_common(const void* film, const void* u, const void* vk, const void* mem, const float* lnc_g, const float* lnc_b, int S,
                             int Lq, int N, int heads, int d, int spm) {
  if (!film || !u || !vk || !mem || !lnc_g || !lnc_b || S <= 0 || Lq <= 0 || N <= 0 || spm <= 0 || S % spm) return DIG_ERR_ARG;
  if ((d != 128 && d != 384 && d != 512) || heads != d / 64 || N > TCV_MAXN || Lq > TCV_MAXQ) return DIG_ERR_UNSUPPORTED;
  if (!aligned16(film) || !aligned16(u) || !aligned16(vk) || !aligned16(mem)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int ctc_common(const void* logits, int ld, const void* target, int ldt, const void* target_len, int B, int T, int C, int blank) {
  if (!logits || !target || !target_len || B < 0 || T <= 0 || C <= 0 || ldt <= 0 || ld < C || blank < 0 || blank >= C) return DIG_ERR_ARG;
  if (T > CTC_MAX_T || C < 2 || C > CTC_MAX_C || ldt > CTC_MAX_LDT) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
// the output side of a weight-gradient problem table (host memory)
static inline int wgrad_outputs(const dig_wgrad_prob_t* q, int n, int fn) {
  for (int k = 0; k < n; ++k) {
    if (!q[k].out || q[k].I <= 0 || q[k].J <= 0 || (q[k].I % 128) || (q[k].J % (128 * fn))) return DIG_ERR_ARG;
    if ((q[k].ldo & 3) || !aligned16(q[k].out)) return DIG_ERR_ALIGN;
  }
  return DIG_OK;
}

// ---- gemm.hip
static inline int gemm_bf16_dropout(const void* A, const void* B, void* C, int I, int J, int R, int lda, int ldb, int ldc, int trans_a, int trans_b,
                                    int out_kind, const float* bias, const void* resid, int ldr, void* pre_act, int ldp, float alpha, int alpha_cols,
                                    int act, int splits, int a_rows, int b_rows, int bk, float* colsum_partials, const dig_dropout_t* drop) {
  if (!A || !B || !C || I <= 0 || J <= 0 || R <= 0 || splits < 1) return DIG_ERR_ARG;
  const bool dropping = drop && (drop->thr || drop->pthr);
  if (dropping) {
    // instantiated for the tiles the fine-tune step uses: 128x128 (bk 0 / 64 / 32) forward and dgrad, 256x256 / 256x192 (bk 244 / 264) forward
    if (out_kind != 0 || trans_a || !(bk == 0 || bk == 32 || bk == 64 || ((bk == 244 || bk == 264) && !trans_b))) return DIG_ERR_UNSUPPORTED;
    if ((size_t)I * (size_t)J >= OFFSET_LIMIT || (drop->pthr && drop->rows_per_sample <= 0)) return DIG_ERR_ARG;
  }
  if (bias && !aligned16(bias)) return DIG_ERR_ALIGN;
  if (out_kind < 0 || out_kind > 2 || act < 0 || act > 2 ||
      (bk != 0 && bk != 32 && bk != 64 && bk != 244 && bk != 264 && bk != 212 && bk != 221 && bk != 544 && bk != 564))
    return DIG_ERR_ARG;
  if (act == 2 && !resid) return DIG_ERR_ARG;                   // act 2: resid carries the saved pre-activation
  if (bk == 0) bk = 64;
  if (!aligned16(A) || !aligned16(B) || !aligned16(C) || (lda & 7) || (ldb & 7)) return DIG_ERR_ALIGN;
  if ((J & 7) || (ldc & 7) || (resid && ((ldr & 7) || !aligned16(resid))) || (pre_act && ((ldp & 7) || !aligned16(pre_act)))) return DIG_ERR_ALIGN;
  if (!trans_a && (R % GEMM_BR)) return DIG_ERR_ARG;   // direct operands need R % 64 == 0 (row-wrap would pollute)
  if (!trans_b && (R % GEMM_BR)) return DIG_ERR_ARG;
  if (out_kind == 2 && (bias || resid || act)) return DIG_ERR_ARG;
  if (out_kind != 2 && splits != 1) return DIG_ERR_ARG;
  if (out_kind == 2 && ldc != J) return DIG_ERR_ARG;            // partial slabs are dense [splits][I][J]
  if (colsum_partials && !(act == 2 && out_kind == 0 && trans_b && !trans_a && (bk < 100 || bk == 244)))
    return DIG_ERR_UNSUPPORTED;                                  // 128x128 kernel and the 64x64-per-wave wide tiles
  if (colsum_partials && !aligned16(colsum_partials)) return DIG_ERR_ALIGN;
  // a_rows / b_rows (0 = default) bound the rows that really exist in memory; the operands are addressed through 32-bit byte offsets
  const size_t ab = (size_t)(a_rows > 0 ? a_rows : (trans_a ? R : I)) * lda * 2;
  const size_t bb = (size_t)(b_rows > 0 ? b_rows : (trans_b ? R : J)) * ldb * 2;
  if (ab >= OFFSET_LIMIT || bb >= OFFSET_LIMIT) return DIG_ERR_ARG;
  if (gemm_effective_splits(R, splits) != splits) return DIG_ERR_ARG;   // use dig_gemm_effective_splits()
  if (!dropping && !gemm_form_ok(trans_a, trans_b, out_kind, bk)) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int reduce_partials_multi(const dig_reduce_seg_t* segs, int n_segs) {
  if (!segs || n_segs < 1 || n_segs > DIG_REDUCE_MAX_SEGS) return DIG_ERR_ARG;
  for (int k = 0; k < n_segs; ++k) {
    const dig_reduce_seg_t& g = segs[k];
    if (!g.partials || !g.out || g.splits < 1 || g.n <= 0 || (g.n & 3)) return DIG_ERR_ARG;
    if (!aligned16(g.partials) || !aligned16(g.out)) return DIG_ERR_ALIGN;
  }
  return DIG_OK;
}

// ---- wgrad.hip
static inline int wgrad_group(const dig_wgrad_prob_t* probs, int n_probs, const dig_wgrad_prob_t* fold_probs, int n_fold, int R, int splits,
                              const unsigned* wg_map, int n_wg, float* slabs, const float* fold_slabs, int fold_splits, int fn, int wa) {
  if (n_probs < 0 || n_probs > DIG_WGRAD_MAX_PROBS || n_fold < 0 || n_fold > DIG_WGRAD_MAX_PROBS || (n_probs == 0 && n_fold == 0)) return DIG_ERR_ARG;
  if ((fn != 2 && fn != 3) || (wa != 1 && wa != 2)) return DIG_ERR_UNSUPPORTED;
  if (n_wg < 1 || (n_probs > 0 && (!probs || !wg_map || !slabs || R < 64 || (R % 64) || splits < 1))) return DIG_ERR_ARG;
  if (n_fold > 0 && (!fold_probs || !fold_slabs || fold_splits < 1)) return DIG_ERR_ARG;
  if (int rc = wgrad_outputs(probs, n_probs, fn)) return rc;
  if (int rc = wgrad_outputs(fold_probs, n_fold, fn)) return rc;
  for (int k = 0; k < n_probs; ++k) {
    const dig_wgrad_prob_t& q = probs[k];
    if (!q.A || !q.B) return DIG_ERR_ARG;
    if (!aligned16(q.A) || !aligned16(q.B) || (q.lda & 7) || (q.ldb & 7) || q.lda < q.I || q.ldb < q.J) return DIG_ERR_ALIGN;
    if ((size_t)R * q.lda * 2 >= OFFSET_LIMIT || (size_t)R * q.ldb * 2 >= OFFSET_LIMIT) return DIG_ERR_UNSUPPORTED;
  }
  if (n_probs && wgrad_group_effective_splits(R, splits) != splits) return DIG_ERR_ARG;
  if (n_probs && !aligned16(slabs)) return DIG_ERR_ALIGN;
  if (n_fold && !aligned16(fold_slabs)) return DIG_ERR_ALIGN;
  return DIG_OK;
}

// ---- mlp_chain.hip
static inline int mlp_chain_fwd(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, const void* resid, void* out,
                                void* pre_out, void* act_out, int R, int D, int F) {
  if (int rc = mlp_chain_common(x, w1, w2, out, R, D, F)) return rc;
  if ((b1 && !aligned16(b1)) || (b2 && !aligned16(b2)) || (resid && !aligned16(resid)) || (pre_out && !aligned16(pre_out)) ||
      (act_out && !aligned16(act_out)))
    return DIG_ERR_ALIGN;
  if ((pre_out == nullptr) != (act_out == nullptr)) return DIG_ERR_ARG;             // both side outputs or none
  if (mlp_chain_lds_bytes(pre_out ? 1 : 0, false, F) > LDS_LIMIT) return DIG_ERR_UNSUPPORTED;   // b1 [F] sits in LDS
  return DIG_OK;
}
static inline int mlp_chain_fwd_ln_dropout(const void* x, const void* resid, const float* ln_g, const float* ln_b, float eps, void* ln_out,
                                           float* ln_mean, float* ln_rstd, const void* w1, const float* b1, const void* w2, const float* b2,
                                           void* out, void* pre_out, void* act_out, const float* nln_g, const float* nln_b, void* nln_out,
                                           float* nln_mean, float* nln_rstd, int R, int D, int F, const dig_dropout_t* drop) {
  if (int rc = mlp_chain_common(x, w1, w2, out, R, D, F)) return rc;
  if ((ln_g == nullptr) != (ln_b == nullptr) || (nln_g == nullptr) != (nln_b == nullptr) || (nln_g == nullptr) != (nln_out == nullptr)) return DIG_ERR_ARG;
  if ((ln_mean == nullptr) != (ln_rstd == nullptr) || (nln_mean == nullptr) != (nln_rstd == nullptr)) return DIG_ERR_ARG;
  if (!ln_g && (ln_out || ln_mean)) return DIG_ERR_ARG;                              // x is normalised already: nothing to report about it
  if (resid && !aligned16(resid)) return DIG_ERR_ALIGN;
  if ((pre_out == nullptr) != (act_out == nullptr)) return DIG_ERR_ARG;
  if (F > CHAIN_LN_MAX_F) return DIG_ERR_UNSUPPORTED;                               // (LDS: the LayerNorm vectors sit behind b1 / b2)
  if ((b1 && !aligned16(b1)) || (b2 && !aligned16(b2)) || (pre_out && !aligned16(pre_out)) || (act_out && !aligned16(act_out)) ||
      (ln_out && !aligned16(ln_out)) || (nln_out && !aligned16(nln_out)))
    return DIG_ERR_ALIGN;
  if (drop && (drop->thr || drop->pthr)) {
    if (drop->pthr && drop->rows_per_sample <= 0) return DIG_ERR_ARG;
    if ((size_t)R * D >= OFFSET_LIMIT) return DIG_ERR_UNSUPPORTED;                  // (element index of the mask hash: 32 bits)
  }
  return DIG_OK;
}
static inline int mlp_chain_bwd_ln_proj(const void* dy, const void* w2t, const void* pre, const void* w1t, void* dpre_out, const void* x_mid,
                                        const float* ln_g, const float* ln_mean, const float* ln_rstd, void* dx_mid_out, float* colsum_partials,
                                        float* ln_partials, const void* projt, void* dctx_out, int R, int D, int F) {
  if (int rc = mlp_chain_common(dy, w2t, w1t, dx_mid_out, R, D, F)) return rc;
  if (!pre || !dpre_out || !x_mid || !ln_g || !ln_mean || !ln_rstd || !ln_partials || ((projt == nullptr) != (dctx_out == nullptr))) return DIG_ERR_ARG;
  if (((size_t)R + CHAIN_ROWS) * D * 2 >= OFFSET_LIMIT) return DIG_ERR_UNSUPPORTED;   // (row offsets of the LayerNorm phase are 32-bit)
  if (!aligned16(pre) || !aligned16(dpre_out) || !aligned16(x_mid) || (colsum_partials && !aligned16(colsum_partials)) ||
      (projt && (!aligned16(projt) || !aligned16(dctx_out))))
    return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int mlp_chain_bwd(const void* dy, const void* w2t, const void* pre, const void* w1t, void* dpre_out, void* dx_out,
                                float* colsum_partials, int R, int D, int F) {
  if (int rc = mlp_chain_common(dy, w2t, w1t, dx_out, R, D, F)) return rc;
  if (!pre || !dpre_out) return DIG_ERR_ARG;
  if (!aligned16(pre) || !aligned16(dpre_out) || (colsum_partials && !aligned16(colsum_partials))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int transpose_bf16_multi(const void* const* srcs, void* const* dsts, int count, int rows, int cols) {
  if (!srcs || !dsts || count < 1 || count > TRANSPOSE_MAX || rows <= 0 || cols <= 0) return DIG_ERR_ARG;
  for (int k = 0; k < count; ++k)
    if (!srcs[k] || !dsts[k]) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- norm.hip
static inline int layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int rows, int D, float eps,
                                int fuse_gelu) {
  if (!x || !gamma || !beta || !y || !mean || !rstd || rows <= 0) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned16(y)) return DIG_ERR_ALIGN;
  if (!layernorm_dim_ok(D)) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int layernorm_bwd_partials(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                         const void* dres, void* dx, float* workspace, int rows, int D, int fuse_gelu) {
  if (!dy || !x || !gamma || !mean || !rstd || !dx || !workspace || rows <= 0) return DIG_ERR_ARG;
  if (fuse_gelu && !beta) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dx) || (dres && !aligned16(dres))) return DIG_ERR_ALIGN;
  if (!layernorm_dim_ok(D)) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}

// ---- elementwise.hip
static inline int mask_views_u8(const void* mask, int elem_kind, int B, int V, int N, int keep_views, unsigned char* out) {
  if (!mask || !out || B <= 0 || V <= 0 || N <= 0 || keep_views < 0) return DIG_ERR_ARG;
  if (elem_kind < 0 || elem_kind > 4) return DIG_ERR_UNSUPPORTED;     // 0: 1-byte (bool / uint8), 1: fp32, 2: fp64, 3: int32, 4: int64
  return DIG_OK;
}
static inline int colsum_partials_multi(const dig_colsum_seg_t* segs, int n_segs) {
  if (!segs || n_segs < 1 || n_segs > DIG_COLSUM_MAX_SEGS) return DIG_ERR_ARG;
  for (int k = 0; k < n_segs; ++k) {
    const dig_colsum_seg_t& g = segs[k];
    if (!g.partials || !g.out || g.n_parts <= 0 || g.C <= 0 || (g.C & 7) || g.stride < g.C || (g.stride & 3)) return DIG_ERR_ARG;
    if (!aligned16(g.partials)) return DIG_ERR_ALIGN;
  }
  return DIG_OK;
}

// ---- decode.hip
static inline int beam_step(const float* logits, int ld, float* seq_scores, int B, int beam_width, int C, int eos, long long* symbols,
                            long long* predecessors, float* stored_scores) {
  return beam_common(logits, ld, seq_scores, B, beam_width, BEAM_STEP_MAX_WIDTH, C, symbols, predecessors, stored_scores);
}
static inline int attn_beam_advance(const float* logits, int ld, float* seq_scores, int B, int beam_width, int C, int eos, long long* symbols,
                                    long long* predecessors, float* stored_scores, const long long* force_candidates, const float* s_in,
                                    const void* sbf_in, float* s_out, void* sbf_out, int S, const float* table, int E, void* inp, int ld_inp) {
  if (!s_in || !sbf_in || !s_out || !sbf_out || !table || !inp || S <= 0 || E <= 0 || ld_inp < E) return DIG_ERR_ARG;
  if (int rc = beam_common(logits, ld, seq_scores, B, beam_width, BEAM_ADVANCE_MAX_WIDTH, C, symbols, predecessors, stored_scores)) return rc;
  const size_t rows = (size_t)B * beam_width * S;
  if (ranges_overlap(s_in, s_out, rows * sizeof(float)) || ranges_overlap(sbf_in, sbf_out, rows * 2)) return DIG_ERR_ARG;   // fp32 and bf16 states
  return DIG_OK;
}

// ---- text_cond_attn.hip
static inline int tcv_attn_fwd(const void* film, const void* u, const void* vk, const void* mem, const float* lnc_g, const float* lnc_b, float eps,
                               void* c, float* lse, float* wmean, int S, int Lq, int N, int heads, int d, int slots_per_mem,
                               const dig_dropout_t* drop) {
  if (!c || !lse) return DIG_ERR_ARG;
  if (int rc = tcv_common(film, u, vk, mem, lnc_g, lnc_b, S, Lq, N, heads, d, slots_per_mem)) return rc;
  if (!aligned16(c)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int tcv_attn_bwd(const void* film, const void* u, const void* vk, const void* mem, const float* lnc_g, const float* lnc_b, float eps,
                               const void* c, const float* lse, const void* dc, void* du, void* dfilm, void* dvk, void* dmem, float* dlnc_g,
                               float* dlnc_b, float* workspace, int S, int Lq, int N, int heads, int d, int slots_per_mem,
                               const dig_dropout_t* drop) {
  if (!c || !lse || !dc || !du || !dfilm || !dvk || !dmem || !dlnc_g || !dlnc_b || !workspace) return DIG_ERR_ARG;
  if (int rc = tcv_common(film, u, vk, mem, lnc_g, lnc_b, S, Lq, N, heads, d, slots_per_mem)) return rc;
  if (slots_per_mem != 1) return DIG_ERR_UNSUPPORTED;
  if (!aligned16(c) || !aligned16(dc) || !aligned16(du) || !aligned16(dfilm) || !aligned16(dvk) || !aligned16(dmem)) return DIG_ERR_ALIGN;
  return DIG_OK;
}

// ---- ctc.hip
static inline int ctc_loss(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset, int B, int T,
                           int C, int blank, float* nll, float* loss) {
  if (!nll || !loss) return DIG_ERR_ARG;
  return ctc_common(logits, ld, target, ldt, target_len, B, T, C, blank);
}
static inline int ctc_loss_bwd(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset,
                               const float* gscalar, int B, int T, int C, int blank, void* dlogits, int ldd, int dlogits_is_f32) {
  if (!dlogits || ldd < C) return DIG_ERR_ARG;
  return ctc_common(logits, ld, target, ldt, target_len, B, T, C, blank);
}
static inline int ctc_align(const float* logits, int ld, const long long* target, int ldt, const long long* target_len, int len_offset, int B, int T,
                            int C, int blank, int* start, int* end, float* char_logp, float* path_logp, int* frame_label) {
  if (!start || !end || !char_logp || !path_logp) return DIG_ERR_ARG;                 // (frame_label: nullable)
  return ctc_common(logits, ld, target, ldt, target_len, B, T, C, blank);
}

// ---- abiaug.hip
static inline int abiaug_sample(dig_abi_params* params, long long* info, const int* heights, const int* widths, int n_img, const dig_abi_run* run,
                                unsigned long long seed, unsigned step) {
  if (!params || !info || !heights || !widths || n_img <= 0 || !abi_run_ok(run)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int abiaug_workspace_bytes(int geom, int det, int wh, int ww, const dig_abi_run* run) {
  if (!abi_run_ok(run) || wh <= 0 || ww <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int abiaug_warp_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                                 const dig_abi_params* params, const dig_abi_run* run, unsigned char* work, long long work_bytes, int max_wh,
                                 int max_ww) {
  if (!packed || !offsets || !heights || !widths || !params || !abi_run_ok(run) || n_img <= 0 || max_wh <= 0 || max_ww <= 0 ||
      work_bytes < 0 || (work_bytes > 0 && !work))
    return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int abiaug_deteriorate_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                                        const dig_abi_params* params, const dig_abi_run* run, unsigned char* work, long long work_bytes, int max_wh,
                                        int max_ww) {
  if (!packed || !offsets || !heights || !widths || !params || !abi_run_ok(run) || n_img <= 0 || max_wh <= 0 || max_ww <= 0 ||
      work_bytes < 0 || (work_bytes > 0 && !work))
    return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int abiaug_tail(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                              const dig_abi_params* params, const dig_abi_run* run, const unsigned char* work, long long work_bytes, float* out,
                              int out_h, int out_w, float mean, float std_, int max_wh, int max_ww) {
  if (!packed || !offsets || !heights || !widths || !params || !abi_run_ok(run) || !out || n_img <= 0 || out_h <= 0 || out_w <= 0 ||
      max_wh <= 0 || max_ww <= 0 || std_ == 0.f || work_bytes < 0 || (work_bytes > 0 && !work))
    return DIG_ERR_ARG;
  if (abiaug_tail_lds_bytes(out_h, out_w, resize_taps(max_ww, out_w), resize_taps(max_wh, out_h)) > LDS_LIMIT) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}

// ---- attention.hip
static inline int attn_fwd_dropout(const void* qkv, void* ctx, float* lse, int n_img, int heads, int embed_dim, const dig_dropout_t* drop,
                                   int q_rows) {
  if (!qkv || !ctx || !lse || n_img <= 0 || heads <= 0 || embed_dim != (long long)heads * ATTN_HEAD_DIM || q_rows < 1 || q_rows > ATTN_TOKENS) return DIG_ERR_ARG;
  if (!aligned16(qkv) || !aligned16(ctx)) return DIG_ERR_ALIGN;
  if (attn_qkv_bytes_over(n_img, embed_dim)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int attn_bwd_dropout(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int n_img, int heads,
                                   int embed_dim, float scale, float* q_colsum, float* v_colsum, const dig_dropout_t* drop, int q_rows) {
  if (!qkv || !ctx || !dctx || !lse || !dqkv || n_img <= 0 || heads <= 0 || embed_dim != (long long)heads * ATTN_HEAD_DIM || q_rows < 1 || q_rows > ATTN_TOKENS) return DIG_ERR_ARG;
  if ((q_rows + 31) / 32 < 8 && q_colsum) return DIG_ERR_UNSUPPORTED;         // the fused dQ column sums assume all eight query blocks
  if ((q_colsum == nullptr) != (v_colsum == nullptr)) return DIG_ERR_ARG;
  if (!aligned16(qkv) || !aligned16(ctx) || !aligned16(dctx) || !aligned16(dqkv)) return DIG_ERR_ALIGN;
  if (attn_qkv_bytes_over(n_img, embed_dim)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int attn_bwd_proj(const void* qkv, const void* ctx, const void* dy, const void* projt, const float* lse, void* dqkv, int n_img,
                                int heads, int embed_dim, float scale, float* q_colsum, float* v_colsum) {
  if (!qkv || !ctx || !dy || !projt || !lse || !dqkv || n_img <= 0 || heads <= 0) return DIG_ERR_ARG;
  if ((q_colsum == nullptr) != (v_colsum == nullptr)) return DIG_ERR_ARG;
  if (embed_dim != (long long)heads * ATTN_HEAD_DIM || (embed_dim & 127) || embed_dim > ATTN_BWD_PROJ_MAX_DIM) return DIG_ERR_UNSUPPORTED;
  if (!aligned16(qkv) || !aligned16(ctx) || !aligned16(dy) || !aligned16(projt) || !aligned16(dqkv)) return DIG_ERR_ALIGN;
  if (attn_qkv_bytes_over(n_img, embed_dim)) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- attn_block.hip
static inline int attn_block_fwd(const void* ln1, const void* x, const void* qkv_w, const float* qkv_b, const void* proj_w, const float* proj_b,
                                 void* qkv, void* ctx, float* lse, void* x_mid, int n_img, int heads, int embed_dim, float scale) {
  if (!ln1 || !x || !qkv_w || !proj_w || !ctx || !x_mid || n_img <= 0) return DIG_ERR_ARG;
  if ((qkv == nullptr) != (lse == nullptr)) return DIG_ERR_ARG;
  if (!attn_block_supported(heads, embed_dim)) return DIG_ERR_UNSUPPORTED;
  if (!aligned16(ln1) || !aligned16(x) || !aligned16(qkv_w) || !aligned16(proj_w) || !aligned16(ctx) || !aligned16(x_mid) || (qkv && !aligned16(qkv)))
    return DIG_ERR_ALIGN;
  if (attn_qkv_bytes_over(n_img, ATTN_BLOCK_DIM)) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- conv_patch.hip
static inline int im2col3x3(const void* x, void* col, int n_img, int H, int W, int C, int ldc) {
  if (!x || !col || n_img <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || ldc < 9LL * C || (ldc & 7)) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned16(col)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int conv3x3_weight_flip(const void* w, void* wt, int c_out, int c_in) {
  if (!w || !wt || c_out <= 0 || c_in <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int maxpool2x2_fwd(const void* x, void* y, unsigned char* idx, int n_img, int H, int W, int C) {
  if (!x || !y || !idx || n_img <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || C <= 0 || (C & 7)) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned16(y) || !aligned8(idx)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int maxpool2x2_bwd(const void* dy, const unsigned char* idx, void* dx, int n_img, int H, int W, int C) {
  if (!dy || !dx || !idx || n_img <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || C <= 0 || (C & 7)) return DIG_ERR_ARG;
  if (!aligned16(dy) || !aligned16(dx) || !aligned8(idx)) return DIG_ERR_ALIGN;
  return DIG_OK;
}

// ---- ctc.hip
static inline int ctc_greedy_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, long long* ids, float* score,
                                    int* n) {
  if (!logits || !ids || !score || !n || B < 0 || T <= 0 || C <= 0 || ld < C) return DIG_ERR_ARG;
  if (T > CTC_MAX_T || C < 2 || C > CTC_MAX_C) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int ctc_beam_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, int beam_width, long long* ids,
                                  float* score, float* logp, int* n) {
  if (!logits || !ids || !score || !logp || !n || B < 0 || T <= 0 || C <= 0 || ld < C || blank < 0 || blank >= C || beam_width <= 0) return DIG_ERR_ARG;
  if (T > CTC_MAX_T || C < 2 || C > CTC_MAX_C || beam_width > CTC_MAX_W) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int ctc_lexicon_decode(const float* logits, int ld, int B, int T, int C, int blank, int eos, int padding, const int* words,
                                     const int* word_len, int ldw, int W, const int* lex_begin, const int* lex_count, int max_count, int* best_index,
                                     float* logp, long long* ids, float* score, int* n, float* scores, void* workspace, long long workspace_bytes) {
  if (!logits || !words || !word_len || !lex_begin || !lex_count || !best_index || !logp || !ids || !score || !n || !workspace) return DIG_ERR_ARG;
  if (B < 0 || T <= 0 || C <= 0 || ldw <= 0 || ld < C || blank < 0 || blank >= C || W < 0 || max_count < 0) return DIG_ERR_ARG;
  if (T > CTC_MAX_T || C < 2 || C > CTC_MAX_C || ldw > CTC_MAX_LDT || B > GRID_Y_MAX) return DIG_ERR_UNSUPPORTED;
  if (B == 0) return DIG_OK;
  if (!aligned8(workspace)) return DIG_ERR_ALIGN;
  if (workspace_bytes < ctc_lexicon_workspace_bytes(B, T, C, max_count)) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- decode.hip
static inline int decode_embed(const long long* tokens, const float* emb, const float* pe_row, void* x, int B, int d, int vocab) {
  if (!tokens || !emb || !pe_row || !x || B <= 0 || d <= 0 || vocab <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int decode_self_attn(const void* qkv_cache, void* out, int B, int T, int heads, int head_dim, int t, float scale) {
  if (!qkv_cache || !out || B <= 0 || heads <= 0 || t < 0 || t >= T) return DIG_ERR_ARG;
  if (!seq_head_dim_ok(head_dim)) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int decode_cross_attn(const void* q, const void* kv_mem, void* out, float* weights, int B, int n_mem, int heads, int head_dim,
                                    float scale, int slots_per_mem) {
  if (!q || !kv_mem || !out || B <= 0 || n_mem <= 0 || heads <= 0 || slots_per_mem < 1 || B % slots_per_mem) return DIG_ERR_ARG;
  if (!seq_head_dim_ok(head_dim) || n_mem > DECODE_MAX_MEM) return DIG_ERR_UNSUPPORTED;
  if (!aligned16(kv_mem) || !aligned16(q)) return DIG_ERR_ALIGN;           // 16-byte reads of both
  return DIG_OK;
}
static inline int softmax_argmax(const float* logits, int ld, float* probs, long long* tokens, int B, int C) {
  if (!logits || !probs || !tokens || B <= 0 || C <= 0 || ld < C) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- elementwise.hip
static inline int patch_embed_fwd(const float* img, const float* W, const float* bias, const unsigned char* mask, const float* mask_token,
                                  const float* pos, void* out, int n_img, int gh, int gw, int D) {
  if (!img || !W || !bias || !mask_token || !pos || !out || n_img <= 0 || D <= 0 || D > PATCH_EMBED_MAX_D || (D & 63)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int patch_embed_bwd(const void* dy, const float* img, const unsigned char* mask, float* dW, float* dbias, float* dmask_token,
                                  int n_img, int gh, int gw, int D) {
  if (!dy || !img || !dW || !dbias || !dmask_token || n_img <= 0 || D <= 0 || D > PATCH_EMBED_MAX_D || (D & 63)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int window_pool_fwd(const void* x, void* out, int out_is_f32, int n_img, int gh, int gw, int nwin, int D) {
  if (!x || !out || n_img <= 0 || nwin <= 0 || gh <= 0 || gw <= 0 || (D & 1)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int window_pool_bwd(const void* dpool, void* dx, int n_img, int gh, int gw, int nwin, int D, int accumulate) {
  if (!dpool || !dx || n_img <= 0 || nwin <= 0 || gh <= 0 || gw <= 0 || (D & 1)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int mask_to_index(const unsigned char* mask, int* idx, int* count, int B, int N, int max_per_sample) {
  if (!mask || !idx || !count || B <= 0 || N <= 0 || max_per_sample <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int gather_rows(const void* src, const int* idx, void* dst, int M, int M_pad, int D) {
  if (!src || !idx || !dst || M <= 0 || M_pad < M || (D & 7)) return DIG_ERR_ARG;
  if (!aligned16(src) || !aligned16(dst)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int scatter_rows_add(const void* src, const int* idx, void* dst, int M, int D) {
  if (!src || !idx || !dst || M <= 0 || (D & 7)) return DIG_ERR_ARG;
  if (!aligned16(src) || !aligned16(dst)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int mim_target(const float* img, const int* idx, float* target, int M, int gh, int gw, int normalize) {
  if (!img || !idx || !target || M <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int mse_fwd_bwd_ws(const float* pred, int ld_pred, const float* target, int M, int C, float gscale, float* loss, void* dpred,
                                 int ld_dpred, float* workspace) {
  if (!pred || !target || M <= 0 || C <= 0 || ld_pred < C || (dpred && ld_dpred < C)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int add_bf16(const void* a, const void* b, void* out, long long n) {
  if (!a || !b || !out || n <= 0 || (n & 7)) return DIG_ERR_ARG;
  if (!aligned16(a) || !aligned16(b) || !aligned16(out)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int gelu_bwd(const void* dact, const void* pre, void* dpre, long long n) {
  if (!dact || !pre || !dpre || n <= 0 || (n & 7)) return DIG_ERR_ARG;
  if (!aligned16(dact) || !aligned16(pre) || !aligned16(dpre)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int colsum(const void* x, float* out, float* workspace, int rows, int C, int ld) {
  if (!x || !out || !workspace || rows <= 0 || C <= 0 || (C & 7) || (ld & 7)) return DIG_ERR_ARG;
  if (!aligned16(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int colsum_partials(const float* partials, int n_parts, int C, float* out) {
  if (!partials || !out || n_parts <= 0 || C <= 0 || (C & 7)) return DIG_ERR_ARG;
  if (!aligned16(partials)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int patchify_bf16(const float* img, const unsigned char* mask, void* out, int n_img, int gh, int gw) {
  if (!img || !out || n_img <= 0) return DIG_ERR_ARG;
  if (!aligned16(img) || !aligned16(out)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int colsum_masked(const void* x, const unsigned char* mask, float* out_unmasked, float* out_masked, float* workspace, int rows, int C) {
  if (!x || !mask || !out_unmasked || !out_masked || !workspace || rows <= 0 || C <= 0 || (C & 7)) return DIG_ERR_ARG;
  if (!aligned16(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int dropout_apply(const void* in, void* out, long long rows, int cols, const dig_dropout_t* drop) {
  if (!in || !out || !drop || rows <= 0 || cols <= 0 || (cols & 7) || rows >= (1ll << 32) || rows * cols >= (1ll << 32)) return DIG_ERR_ARG;
  if (drop->pthr && drop->rows_per_sample <= 0) return DIG_ERR_ARG;
  if (!aligned16(in) || !aligned16(out)) return DIG_ERR_ALIGN;
  return DIG_OK;
}

// ---- gemm.hip
static inline int reduce_partials_bf16(const float* partials, int splits, long long n, void* out) {
  if (!partials || !out || splits < 1 || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(partials) || !aligned8(out)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int reduce_partials(const float* partials, int splits, long long n, float* out, int accumulate) {
  if (!partials || !out || splits < 1 || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(partials) || !aligned16(out)) return DIG_ERR_ALIGN;
  return DIG_OK;
}

// ---- gru_attn.hip
static inline int addattn_fwd(const void* xproj, const void* sproj, const float* w, const void* x, float* alpha, void* ctx, int ldc, int B, int N,
                              int A, int X) {
  if (!xproj || !sproj || !w || !x || !alpha || !ctx || B <= 0 || N <= 0 || N > ADDATTN_MAX_N || A <= 0 || A > ADDATTN_MAX_A || (A & 7) || X <= 0 || (X & 1) || (ldc & 1))
    return DIG_ERR_ARG;
  if (!aligned16(xproj)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int addattn_fwd_slots(const void* xproj, const void* sproj, const float* w, const void* x, float* alpha, void* ctx, int ldc, int B,
                                    int N, int A, int X, int slots) {
  if (!xproj || !sproj || !w || !x || !ctx || B <= 0 || N <= 0 || A <= 0 || X <= 0 || (X & 1) || (ldc & 1)) return DIG_ERR_ARG;
  if (N > ADDATTN_MAX_N || A > ADDATTN_MAX_A || (A & 7) || slots < 1 || slots > ADDATTN_MAX_SLOTS) return DIG_ERR_UNSUPPORTED;
  if (!aligned16(xproj)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int addattn_bwd(const void* xproj, const void* sproj, const float* w, const void* x, const float* alpha, const void* dctx, int ldd,
                              float* dv, void* dsproj, float* dw_acc, int B, int N, int A, int X) {
  if (!xproj || !sproj || !w || !x || !alpha || !dctx || !dv || !dsproj || !dw_acc || B <= 0 || N <= 0 || N > ADDATTN_MAX_N || A <= 0 || A > ADDATTN_MAX_A || (A & 7) ||
      X <= 0 || X > ADDATTN_MAX_A || (X & 7))
    return DIG_ERR_ARG;
  if (!aligned16(xproj) || !aligned16(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int addattn_bwd_tokens(const void* xproj, const void* sproj_all, const float* w, const float* dv_all, const float* alpha_all,
                                     const void* dctx_all, int ldd, void* dxproj, void* dx, int T, int B, int N, int A, int X) {
  if (!xproj || !sproj_all || !w || !dv_all || !alpha_all || !dctx_all || !dxproj || !dx || T <= 0 || B <= 0 || N <= 0 || A <= 0 || (A & 1) || X <= 0 ||
      (X & 1))
    return DIG_ERR_ARG;
  if (addattn_bwd_tokens_lds_bytes(T, A) > ADDATTN_BWD_TOKENS_LDS || addattn_bwd_tokens_lds_bytes(T, X) > ADDATTN_BWD_TOKENS_LDS) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int gru_cell_fwd(const void* gi, const void* gh, const float* s_prev, float* s, void* s_bf16, float* gates, int B, int S) {
  if (!gi || !gh || !s || !s_bf16 || !gates || B <= 0 || S <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int gru_cell_bwd(const float* ds_a, const float* ds_b, const float* ds_c, const float* ds_d, const float* gates, const float* s_prev,
                               void* dgi, void* dgh, float* ds_prev, int B, int S) {
  if (!ds_a || !gates || !dgi || !dgh || !ds_prev || B <= 0 || S <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int embed_rows(const long long* tokens, const float* table, void* out, int ld, int rows, int cols, int vocab) {
  if (!tokens || !table || !out || rows <= 0 || cols <= 0 || ld < cols || vocab <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- input.hip
static inline int resize_bicubic_normalize_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths,
                                              int n_img, float* out, int out_h, int out_w, float mean, float std_, int max_h, int max_w) {
  if (!packed || !offsets || !heights || !widths || !out || n_img <= 0 || out_h <= 0 || out_w <= 0 || max_h <= 0 || max_w <= 0 || std_ == 0.f)
    return DIG_ERR_ARG;
  // crops beyond ~ (64 x out) per axis: shrink on the host first
  if (resize_lds_bytes(out_h, out_w, resize_taps(max_w, out_w), resize_taps(max_h, out_h)) > LDS_LIMIT) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int random_masks(unsigned char* mask, int n_rows, int n_patches, int num_mask, unsigned long long seed, unsigned step) {
  if (!mask || n_rows <= 0 || n_patches <= 0 || n_patches > RANDOM_MASKS_MAX_PATCHES || num_mask < 0 || num_mask > n_patches) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- keyview.hip
static inline int keyview_sample(dig_kv_params* params, const int* heights, const int* widths, int n_img, unsigned long long seed, unsigned step) {
  if (!params || !heights || !widths || n_img <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int keyview_workspace_bytes(long long packed_bytes, int n_img) {
  if (packed_bytes <= 0 || n_img <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int keyview_stage_a_u8(const unsigned char* packed, const long long* offsets, const int* heights, const int* widths, int n_img,
                                     const dig_kv_params* params, unsigned char* work, long long work_bytes, int max_h, int max_w) {
  if (!packed || !offsets || !heights || !widths || !params || !work || n_img <= 0 || max_h <= 0 || max_w <= 0 || work_bytes <= 0 ||
      work_bytes % 512 != 0 || (long long)max_h * max_w > work_bytes / 2 / 3)   // (3 bytes per pixel, half the workspace)
    return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int keyview_stage_b(const unsigned char* stage_a, const long long* offsets, const int* heights, const int* widths, int n_img,
                                  const dig_kv_params* params, float* out, int out_h, int out_w, float mean, float std_, int max_h, int max_w) {
  if (!stage_a || !offsets || !heights || !widths || !params || !out || n_img <= 0 || out_h <= 0 || out_w <= 0 || max_h <= 0 || max_w <= 0 ||
      std_ == 0.f)
    return DIG_ERR_ARG;
  if (stage_b_lds_bytes(out_h, out_w, resize_taps(max_w, out_w), resize_taps(max_h, out_h)) > LDS_LIMIT) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}

// ---- labels.hip
static inline int encode_labels(const int* chars, const int* offsets, const int* class_of, int eos, int padding, int unknown, int max_len, int B,
                                long long* labels, long long* lens) {
  if (!chars || !offsets || !class_of || !labels || !lens || max_len < 1 || B < 0) return DIG_ERR_ARG;
  if (B == 0) return DIG_OK;
  if ((long long)B * max_len > 0x7fffffffLL) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}

// ---- loss.hip
static inline int infonce_finish(const float* stats6, float loss_scale, float acc_scale, float* contra, float* accs4) {
  if (!stats6 || !contra || !accs4) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int step_meters(const float* loss, const float* contra, const float* pixel, const float* accs4, const int* counts, int n_counts,
                              const float* grad_norm, float* out10) {
  if (!loss || !contra || !pixel || !accs4 || !counts || n_counts <= 0 || !out10) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int l2norm_fwd(const float* x, float* y, float* inv_norm, int n, int C, float eps) {
  if (!x || !y || !inv_norm || n <= 0 || C <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int n, int C) {
  if (!dy || !y || !inv_norm || !dx || n <= 0 || C <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int sgemm(const float* A, const float* B, float* C, int I, int J, int R, int lda, int ldb, int ldc, int trans_b, float alpha,
                        int r_splits) {
  if (!A || !B || !C || I <= 0 || J <= 0 || R <= 0 || r_splits < 1) return DIG_ERR_ARG;
  if (sgemm_effective_splits(R, r_splits) != r_splits) return DIG_ERR_ARG;   // (callers pick r_splits with R % (64 * r_splits) == 0)
  return DIG_OK;
}
static inline int ce_rows_ws(float* logits, int n, int m, int label_offset, float gscale, float* out3, float* workspace) {
  if (!logits || !out3 || n <= 0 || m <= 0 || label_offset < 0 || (long long)label_offset + n > m) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- metrics.hip
static inline int string_match(const long long* pred, const long long* target, const unsigned char* canon, int n_classes, int eos, int B, int T,
                               unsigned char* match) {
  if (!pred || !target || !canon || !match || n_classes <= 0 || B <= 0 || T <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int char_fmeasure(const long long* pred, const long long* target, const unsigned char* canon, int n_classes, int eos, int B, int T,
                                double* f_per_sample) {
  if (!pred || !target || !canon || !f_per_sample || n_classes <= 0 || B <= 0 || T <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int tokens_to_text(const long long* tokens, const unsigned char* canon, int n_classes, int eos, int B, int T, int* text, int* len) {
  if (!tokens || !canon || !text || !len || n_classes <= 0 || B <= 0 || T <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int edit_distance(const int* a, const int* a_len, int lda, int a_rows, const int* a_index, const int* b, const int* b_len, int ldb,
                                int n, int* dist) {
  if (!a || !a_len || !b || !b_len || !dist || lda <= 0 || ldb <= 0 || n <= 0 || a_rows <= 0) return DIG_ERR_ARG;
  if (!a_index && a_rows < n) return DIG_ERR_ARG;
  if (lda > DIG_LEV_MAX_LEN || ldb > DIG_LEV_MAX_LEN) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}
static inline int lexicon_search(const int* query, const int* query_len, int ldq, int B, const int* words, const int* word_len, int ldw, int W,
                                 const int* lex_begin, const int* lex_count, int max_count, int* best_index, int* best_dist, void* workspace,
                                 long long workspace_bytes) {
  if (!query || !query_len || !words || !word_len || !lex_begin || !lex_count || !best_index || !best_dist || !workspace) return DIG_ERR_ARG;
  if (ldq <= 0 || ldw <= 0 || B <= 0 || W <= 0 || max_count < 0) return DIG_ERR_ARG;
  if (ldq > DIG_LEV_MAX_LEN || ldw > DIG_LEV_MAX_LEN || B > GRID_Y_MAX) return DIG_ERR_UNSUPPORTED;
  if (!aligned8(workspace)) return DIG_ERR_ALIGN;
  if (workspace_bytes < lexicon_search_workspace_bytes(B, max_count)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int seq_confidence(const float* score, const int* text_len, int B, int T, double* conf) {
  if (!score || !text_len || !conf || B <= 0 || T <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- mlp_chain.hip
static inline int transpose_bf16(const void* src, void* dst, int rows, int cols) {
  if (!src || !dst || rows <= 0 || cols <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- norm.hip
static inline int layernorm_bwd_finalize(const float* workspace, int rows, int D, float* dgamma, float* dbeta, float* dcolsum) {
  if (!workspace || !dgamma || !dbeta || rows <= 0 || D <= 0 || (D & 15)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int layernorm_bwd_finalize_parts(const float* workspace, int parts, int D, float* dgamma, float* dbeta, float* dcolsum) {
  if (!workspace || !dgamma || !dbeta || parts <= 0 || D <= 0 || (D & 15)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                const void* dres, void* dx, float* dgamma, float* dbeta, float* dcolsum, float* workspace, int rows, int D,
                                int fuse_gelu) {
  if (!dgamma || !dbeta || (dcolsum && !dres)) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int bn_stats(const void* x, float* sums, float* workspace, int rows, int C) {
  if (!x || !sums || !workspace || rows <= 0 || C <= 0 || (C & 7)) return DIG_ERR_ARG;
  if (!aligned16(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int bn_fwd_apply_running(const void* x, const float* sums, float n_total, float eps, const float* gamma, const float* beta, int relu,
                                       void* y, float* mean_out, float* rstd_out, float momentum, float* running_mean, float* running_var, int rows,
                                       int C) {
  if (!x || !sums || !y || !mean_out || !rstd_out || rows <= 0 || C <= 0 || (C & 7) || n_total <= 0.f) return DIG_ERR_ARG;
  if ((running_mean == nullptr) != (running_var == nullptr) || (running_mean && n_total <= 1.f)) return DIG_ERR_ARG;
  if ((gamma == nullptr) != (beta == nullptr)) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned16(y) || !aligned16(sums) || (gamma && (!aligned16(gamma) || !aligned16(beta)))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int bn_bwd_stats_acc(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                   int relu, float* sums, float* dbeta_acc, float* dgamma_acc, float* workspace, int rows, int C) {
  if (!dy || !x || !mean || !rstd || !sums || !workspace || rows <= 0 || C <= 0 || (C & 7)) return DIG_ERR_ARG;
  if ((dbeta_acc == nullptr) != (dgamma_acc == nullptr)) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(mean) || !aligned16(rstd) || (gamma && (!aligned16(gamma) || !aligned16(beta)))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int bn_bwd_apply(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                               const float* sums, float n_total, void* dx, int rows, int C) {
  if (!dy || !x || !mean || !rstd || !sums || !dx || rows <= 0 || C <= 0 || (C & 7) || n_total <= 0.f) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dx) || !aligned16(mean) || !aligned16(rstd) || !aligned16(sums) ||
      (gamma && (!aligned16(gamma) || !aligned16(beta)))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int bn_fwd_fused(const void* x, float eps, const float* gamma, const float* beta, int relu, void* y, float* mean_out, float* rstd_out,
                               float momentum, float* running_mean, float* running_var, int rows, int C) {
  if (!x || !y || !mean_out || !rstd_out || (gamma == nullptr) != (beta == nullptr) || (running_mean == nullptr) != (running_var == nullptr))
    return DIG_ERR_ARG;
  if (!bn_fused_supported(rows, C)) return DIG_ERR_UNSUPPORTED;
  // gamma / beta are read with 16-byte loads (load8f); the statistics and running vectors are held to the three-launch path's rule
  if (!aligned16(x) || !aligned16(y) || !aligned16(mean_out) || !aligned16(rstd_out) || (gamma && (!aligned16(gamma) || !aligned16(beta))) ||
      (running_mean && (!aligned16(running_mean) || !aligned16(running_var)))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int bn_bwd_fused(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                               float* dbeta_acc, float* dgamma_acc, void* dx, int rows, int C) {
  if (!dy || !x || !mean || !rstd || !dx || (gamma == nullptr) != (beta == nullptr) || (dbeta_acc == nullptr) != (dgamma_acc == nullptr))
    return DIG_ERR_ARG;
  if (!bn_fused_supported(rows, C)) return DIG_ERR_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dx) || !aligned16(mean) || !aligned16(rstd) || (gamma && (!aligned16(gamma) || !aligned16(beta))) ||
      (dbeta_acc && (!aligned16(dbeta_acc) || !aligned16(dgamma_acc)))) return DIG_ERR_ALIGN;   // mean / rstd / gamma / beta: 16-byte loads (load8f)
  return DIG_OK;
}
static inline int bn_update_running(const float* sums, float n_total, float momentum, float* running_mean, float* running_var, int C) {
  if (!sums || !running_mean || !running_var || C <= 0 || n_total <= 1.f) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- optim.hip
static inline int adamw_step(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_flags,
                             float lr0, float wd0, float lr1, float wd1, float beta1, float beta2, float eps, int step, float grad_scale,
                             const float* finite_gate) {
  if (!p || !g || !m || !v || !group_flags || n <= 0 || (n & 255) || step < 1) return DIG_ERR_ARG;
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || (bf16_shadow && !aligned8(bf16_shadow))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int adamw_step_tr(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_flags,
                                float lr0, float wd0, float lr1, float wd1, float beta1, float beta2, float eps, int step, float grad_scale,
                                const float* finite_gate, const void* mats, int n_mats, int n_tiles, void* tr_out) {
  if (!p || !g || !m || !v || !group_flags || n <= 0 || (n & 255) || step < 1 || !mats || n_mats < 1 || n_tiles < 1 || !tr_out) return DIG_ERR_ARG;
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || (bf16_shadow && !aligned8(bf16_shadow)) || !aligned8(tr_out))
    return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int adamw_bias_corrections(float beta1, float beta2, int step, float* out2) {
  if (!out2 || step < 1) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int adamw_step_dev(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_flags,
                                 const float* scalars6, float beta1, float beta2, float eps, float grad_scale, const float* finite_gate) {
  if (!p || !g || !m || !v || !group_flags || !scalars6 || n <= 0 || (n & 255)) return DIG_ERR_ARG;
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || (bf16_shadow && !aligned8(bf16_shadow))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int adamw_step_groups(float* p, const float* g, float* m, float* v, void* bf16_shadow, long long n, const unsigned char* group_idx,
                                    const float* lr_tab, const float* wd_tab, float beta1, float beta2, float eps, int step, float grad_scale,
                                    const float* finite_gate) {
  if (!p || !g || !m || !v || !group_idx || !lr_tab || !wd_tab || n <= 0 || (n & 255) || step < 1) return DIG_ERR_ARG;
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || (bf16_shadow && !aligned8(bf16_shadow))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int ema_update(float* pm, const float* p, void* bf16_shadow, long long n, float m) {
  if (!pm || !p || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(pm) || !aligned16(p) || (bf16_shadow && !aligned8(bf16_shadow))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int ema_update_dev(float* pm, const float* p, void* bf16_shadow, long long n, const float* m_and_one_minus_m) {
  if (!pm || !p || !m_and_one_minus_m || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(pm) || !aligned16(p) || (bf16_shadow && !aligned8(bf16_shadow))) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int sumsq(const float* x, long long n, float* workspace, float* out) {
  if (!x || !workspace || !out || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int cast_f32_to_bf16(const float* x, void* y, long long n) {
  if (!x || !y || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(x) || !aligned8(y)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int cast_bf16_to_f32(const void* x, float* y, long long n) {
  if (!x || !y || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(y) || !aligned8(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int scale_f32(float* x, long long n, float s) {
  if (!x || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int fill_f32(float* x, long long n, float value) {
  if (!x || n <= 0 || (n & 3)) return DIG_ERR_ARG;
  if (!aligned16(x)) return DIG_ERR_ALIGN;
  return DIG_OK;
}
static inline int scale_by_device_scalar(float* x, long long n, const float* scalar, float extra) {
  if (!x || !scalar || n <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int pad_cast_rows(const float* src, void* dst, int M, int C, int M_pad, int ld) {
  if (!src || !dst || M <= 0 || C <= 0 || M_pad < M || ld < C) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int axpy_f32(float* y, const float* x, long long n, float a) {
  if (!y || !x || n <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}

// ---- seq_attn.hip
static inline int seq_attn_fwd_hd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo, float* lse, int B,
                                  int heads, int Lq, int Lk, float scale, int causal, const long long* lens, const dig_dropout_t* drop,
                                  int head_dim) {
  if (!q || !k || !v || !out || !lse || B <= 0 || heads <= 0 || Lq <= 0 || Lq > SEQ_ATTN_MAX_LQ || Lk <= 0 || Lk > SEQ_ATTN_MAX_LK) return DIG_ERR_ARG;
  if (!seq_head_dim_ok(head_dim)) return DIG_ERR_UNSUPPORTED;
  if ((ldk & 7) || (ldv & 7) || !aligned16(k) || !aligned16(v)) return DIG_ERR_ALIGN;   // 16-byte row reads
  return DIG_OK;
}
static inline int seq_attn_bwd_hd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dout, int ldo,
                                  const float* lse, void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, int B, int heads, int Lq, int Lk,
                                  float scale, int causal, const long long* lens, const dig_dropout_t* drop, int head_dim) {
  if (!q || !k || !v || !dout || !lse || !dq || !dk || !dv || B <= 0 || heads <= 0 || Lq <= 0 || Lq > SEQ_ATTN_MAX_LQ || Lk <= 0 || Lk > SEQ_ATTN_MAX_LK) return DIG_ERR_ARG;
  if (!seq_head_dim_ok(head_dim)) return DIG_ERR_UNSUPPORTED;
  if (seq_attn_bwd_lds_bytes(head_dim, Lk) > DIG_SEQ_ATTN_BWD_LDS_LIMIT) return DIG_ERR_UNSUPPORTED;
  if ((ldk & 7) || (ldv & 7) || !aligned16(k) || !aligned16(v)) return DIG_ERR_ALIGN;   // 16-byte row reads
  if ((lddk & 7) || (lddv & 7) || !aligned16(dk) || !aligned16(dv)) return DIG_ERR_ALIGN;   // 16-byte dK / dV row stores, on both paths
  return DIG_OK;
}
static inline int seq_embed_fwd(const long long* tokens, const float* emb, const float* pos_table, void* x, int B, int T, int d, int vocab) {
  if (!tokens || !emb || !pos_table || !x || B <= 0 || T <= 0 || d <= 0 || vocab <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int seq_embed_bwd_lens(const long long* tokens, const void* dx, float* demb, int n_tok, int d, int vocab, int T,
                                     const long long* lens) {
  if (!tokens || !dx || !demb || n_tok <= 0 || d <= 0 || vocab <= 0) return DIG_ERR_ARG;
  if (lens && (T <= 0 || n_tok % T)) return DIG_ERR_ARG;
  if ((size_t)n_tok * sizeof(int) > SEQ_EMBED_BWD_LDS) return DIG_ERR_UNSUPPORTED;
  return DIG_OK;
}

// ---- seq_loss.hip
static inline int seq_cross_entropy(const float* input, const long long* target, const long long* length, int B, int T, int C, float* row_workspace,
                                    float* loss) {
  if (!input || !target || !length || !row_workspace || !loss || B <= 0 || T <= 0 || C <= 0) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int seq_cross_entropy_bwd(const float* logits, int ld, const long long* target, const long long* length, const float* gscalar, int B,
                                        int T, int C, void* dlogits, int ldd) {
  if (!logits || !target || !length || !dlogits || B <= 0 || T <= 0 || C <= 0 || ld < C || ldd < C) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int seq_ls_cross_entropy(const float* input, const long long* target, const long long* length, int B, int T, int C, float smoothing,
                                       float* row_workspace, float* loss) {
  if (!input || !target || !length || !row_workspace || !loss || B <= 0 || T <= 0 || C <= 0 || smoothing < 0.f || smoothing > 1.f) return DIG_ERR_ARG;
  return DIG_OK;
}
static inline int seq_ls_cross_entropy_bwd(const float* logits, int ld, const long long* target, const long long* length, const float* gscalar,
                                           int B, int T, int C, float smoothing, void* dlogits, int ldd) {
  if (!logits || !target || !length || !dlogits || B <= 0 || T <= 0 || C <= 0 || ld < C || ldd < C || smoothing < 0.f || smoothing > 1.f) return DIG_ERR_ARG;
  return DIG_OK;
}

}  // namespace dig_rules
