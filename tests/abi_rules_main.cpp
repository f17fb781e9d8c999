// The magnitude rules of dig_amd/csrc/abi_rules.h, checked without a library and without memory: every pointer below is a dummy that no
// rule dereferences (rules read only the small structs and tables passed by pointer, which are real).  Each rule is called just below, at
// and just above its limit and with INT_MAX-sized arguments; tests/test_abi_rules.py builds this file with the address and
// undefined-behaviour sanitizers, so a signed overflow inside a rule's size arithmetic ends the run.  The limits are worked out by hand
// from the documented sizes (comments), not read back from the header's helpers.
#include "../dig_amd/csrc/abi_rules.h"

#include <climits>
#include <cstdio>

namespace R = dig_rules;
static int failures = 0, checks = 0;
#define EXPECT(code, call)                                                                              \
  do {                                                                                                  \
    const int got_ = (call);                                                                            \
    ++checks;                                                                                           \
    if (got_ != (code)) { ++failures; std::printf("line %d: %s -> %d, expected %d\n", __LINE__, #call, got_, (int)(code)); } \
  } while (0)

template <class T>
static T* P(uintptr_t step = 0) { return reinterpret_cast<T*>(uintptr_t(0x100000) + step); }   // 16-byte aligned, never dereferenced
static const int OK = DIG_OK, ARG = DIG_ERR_ARG, ALIGN = DIG_ERR_ALIGN, UNSUP = DIG_ERR_UNSUPPORTED;
static const int IMAX = INT_MAX;

static void sequence_attention() {
  // lds_bwd = 256 hd + Lk (256 + 2 hd) <= 163840: Lk <= 384 (hd 64), 430 (hd 48: 12288 + 352 Lk), 512 = the ARG limit (hd 24)
  auto bwd = [](int hd, int Lk, int Lq = 32) {
    return R::seq_attn_bwd_hd(P<void>(), 64, P<void>(), 64, P<void>(), 64, P<void>(), 64, P<float>(), P<void>(), 64, P<void>(), 64, P<void>(), 64, 1, 1, Lq, Lk,
                              1.f, 0, nullptr, nullptr, hd);
  };
  EXPECT(OK, bwd(64, 383)); EXPECT(OK, bwd(64, 384)); EXPECT(UNSUP, bwd(64, 385)); EXPECT(UNSUP, bwd(64, 512));
  EXPECT(OK, bwd(48, 430)); EXPECT(UNSUP, bwd(48, 431));
  EXPECT(OK, bwd(24, 512)); EXPECT(ARG, bwd(24, 513)); EXPECT(ARG, bwd(64, IMAX));
  EXPECT(OK, bwd(64, 64, 32)); EXPECT(ARG, bwd(64, 64, 33)); EXPECT(ARG, bwd(64, 64, IMAX));
  EXPECT(UNSUP, bwd(32, 64)); EXPECT(UNSUP, bwd(IMAX, 64));
  auto fwd = [](int hd, int Lk, int Lq) {
    return R::seq_attn_fwd_hd(P<void>(), 64, P<void>(), 64, P<void>(), 64, P<void>(), 64, P<float>(), IMAX, IMAX, Lq, Lk, 1.f, 0, nullptr, nullptr, hd);
  };
  EXPECT(OK, fwd(64, 512, 32)); EXPECT(ARG, fwd(64, 513, 32)); EXPECT(ARG, fwd(64, 512, 33)); EXPECT(UNSUP, fwd(IMAX, 512, 32));
  // token ids of a launch in LDS: 4 n_tok <= 61440
  EXPECT(OK, R::seq_embed_bwd_lens(P<long long>(), P<void>(), P<float>(), 15360, 8, 8, 0, nullptr));
  EXPECT(UNSUP, R::seq_embed_bwd_lens(P<long long>(), P<void>(), P<float>(), 15361, 8, 8, 0, nullptr));
  EXPECT(UNSUP, R::seq_embed_bwd_lens(P<long long>(), P<void>(), P<float>(), IMAX, IMAX, IMAX, 0, nullptr));
  EXPECT(OK, R::decode_cross_attn(P<void>(), P<void>(), P<void>(), nullptr, 1, 8192, 1, 64, 1.f, 1));
  EXPECT(UNSUP, R::decode_cross_attn(P<void>(), P<void>(), P<void>(), nullptr, 1, 8193, 1, 64, 1.f, 1));
  EXPECT(UNSUP, R::decode_cross_attn(P<void>(), P<void>(), P<void>(), nullptr, IMAX, IMAX, IMAX, 64, 1.f, 1));
}

static void labels_and_beams() {
  // B * max_len <= 2^31 - 1
  auto enc = [](int B, int max_len) { return R::encode_labels(P<int>(), P<int>(), P<int>(), 1, 2, 3, max_len, B, P<long long>(), P<long long>()); };
  EXPECT(OK, enc(1, IMAX)); EXPECT(OK, enc(IMAX, 1)); EXPECT(UNSUP, enc(2, 1 << 30)); EXPECT(OK, enc(2, (1 << 30) - 1)); EXPECT(UNSUP, enc(IMAX, IMAX));
  EXPECT(OK, enc(0, IMAX)); EXPECT(ARG, enc(-1, 1));
  // candidate table in LDS: 4 beam_width C <= 60000
  auto step = [](int bw, int C) { return R::beam_step(P<float>(), C, P<float>(), 1, bw, C, 0, P<long long>(), P<long long>(), P<float>()); };
  EXPECT(OK, step(16, 937)); EXPECT(UNSUP, step(16, 938)); EXPECT(UNSUP, step(17, 8)); EXPECT(UNSUP, step(16, IMAX)); EXPECT(UNSUP, step(IMAX, IMAX));
  auto adv = [](int bw, int C, int B = 1, int S = 8) {
    return R::attn_beam_advance(P<float>(), C, P<float>(), B, bw, C, 0, P<long long>(), P<long long>(), P<float>(), nullptr, P<float>(), P<void>(),
                                P<float>(1 << 20), P<void>(1 << 20), S, P<float>(), 8, P<void>(), 8);
  };
  EXPECT(OK, adv(8, 1875)); EXPECT(UNSUP, adv(8, 1876)); EXPECT(UNSUP, adv(9, 8));
  EXPECT(ARG, adv(8, 8, 1024, 1024));          // 8 Mi state elements: the input and output states 1 MiB apart overlap
  EXPECT(ARG, adv(8, 8, IMAX, IMAX));
  EXPECT(OK, R::lexicon_search(P<int>(), P<int>(), 128, 65535, P<int>(), P<int>(), 128, 1, P<int>(), P<int>(), 64, P<int>(), P<int>(), P<void>(), 65535LL * 8));
  EXPECT(ARG, R::lexicon_search(P<int>(), P<int>(), 128, 65535, P<int>(), P<int>(), 128, 1, P<int>(), P<int>(), 65, P<int>(), P<int>(), P<void>(), 65535LL * 8));
  EXPECT(UNSUP, R::lexicon_search(P<int>(), P<int>(), 128, 65536, P<int>(), P<int>(), 128, 1, P<int>(), P<int>(), 64, P<int>(), P<int>(), P<void>(), LLONG_MAX));
  EXPECT(UNSUP, R::lexicon_search(P<int>(), P<int>(), 129, 1, P<int>(), P<int>(), 128, 1, P<int>(), P<int>(), 64, P<int>(), P<int>(), P<void>(), LLONG_MAX));
  EXPECT(UNSUP, R::lexicon_search(P<int>(), P<int>(), IMAX, IMAX, P<int>(), P<int>(), IMAX, IMAX, P<int>(), P<int>(), IMAX, P<int>(), P<int>(), P<void>(), LLONG_MAX));
  auto lex = [](int B, int T, int C, int ldw, long long bytes, int max_count = 64) {
    return R::ctc_lexicon_decode(P<float>(), C, B, T, C, 0, 1, 2, P<int>(), P<int>(), ldw, 1, P<int>(), P<int>(), max_count, P<int>(), P<float>(), P<long long>(),
                                 P<float>(), P<int>(), nullptr, P<void>(), bytes);
  };
  const long long full = 65535LL * 8 + 65535LL * 64 * 256 * 4;      // one chunk of keys per sample + the [B, T, C] fp32 log-probabilities
  EXPECT(OK, lex(65535, 64, 256, 63, full)); EXPECT(ARG, lex(65535, 64, 256, 63, full - 1)); EXPECT(UNSUP, lex(65536, 64, 256, 63, LLONG_MAX));
  EXPECT(UNSUP, lex(1, 65, 256, 63, LLONG_MAX)); EXPECT(UNSUP, lex(1, 64, 257, 63, LLONG_MAX)); EXPECT(UNSUP, lex(1, 64, 256, 64, LLONG_MAX));
  EXPECT(UNSUP, lex(IMAX, IMAX, IMAX, IMAX, LLONG_MAX, IMAX));
  EXPECT(OK, R::ctc_beam_decode(P<float>(), 256, 1, 64, 256, 0, 1, 2, 32, P<long long>(), P<float>(), P<float>(), P<int>()));
  EXPECT(UNSUP, R::ctc_beam_decode(P<float>(), 256, 1, 64, 256, 0, 1, 2, 33, P<long long>(), P<float>(), P<float>(), P<int>()));
  EXPECT(UNSUP, R::ctc_loss(P<float>(), 256, P<long long>(), 64, P<long long>(), 0, 1, 64, 256, 0, P<float>(), P<float>()));
  EXPECT(OK, R::ctc_loss(P<float>(), 256, P<long long>(), 63, P<long long>(), 0, 1, 64, 256, 0, P<float>(), P<float>()));
  EXPECT(UNSUP, R::edit_distance(P<int>(), P<int>(), 129, 1, nullptr, P<int>(), P<int>(), 128, 1, P<int>()));
  EXPECT(OK, R::edit_distance(P<int>(), P<int>(), 128, 1, nullptr, P<int>(), P<int>(), 128, 1, P<int>()));
}

static void encoder_attention() {
  // the packed qkv tensor: n_img * 256 * 3 * embed_dim * 2 bytes < 2^32; at embed_dim 384 that is n_img <= 7281 (589824 n_img)
  auto fwd = [](int n_img, int heads, int dim) { return R::attn_fwd_dropout(P<void>(), P<void>(), P<float>(), n_img, heads, dim, nullptr, 256); };
  EXPECT(OK, fwd(7281, 6, 384)); EXPECT(ARG, fwd(7282, 6, 384)); EXPECT(ARG, fwd(IMAX, 6, 384)); EXPECT(ARG, fwd(IMAX, IMAX, IMAX));
  EXPECT(ARG, fwd(IMAX, 1 << 24, 1 << 30));   // heads * 64 == embed_dim, n_img * embed_dim wraps 64 bits only after the product by 1536
  EXPECT(OK, fwd(43690, 1, 64)); EXPECT(ARG, fwd(43691, 1, 64));          // 98304 n_img
  auto bwd = [](int n_img) {
    return R::attn_bwd_dropout(P<void>(), P<void>(), P<void>(), P<float>(), P<void>(), n_img, 6, 384, 1.f, nullptr, nullptr, nullptr, 256);
  };
  EXPECT(OK, bwd(7281)); EXPECT(ARG, bwd(7282)); EXPECT(ARG, bwd(IMAX));
  auto proj = [](int n_img) { return R::attn_bwd_proj(P<void>(), P<void>(), P<void>(), P<void>(), P<float>(), P<void>(), n_img, 6, 384, 1.f, nullptr, nullptr); };
  EXPECT(OK, proj(7281)); EXPECT(ARG, proj(7282)); EXPECT(ARG, proj(IMAX));
  EXPECT(UNSUP, R::attn_bwd_proj(P<void>(), P<void>(), P<void>(), P<void>(), P<float>(), P<void>(), 1, 10, 640, 1.f, nullptr, nullptr));
  EXPECT(UNSUP, R::attn_bwd_proj(P<void>(), P<void>(), P<void>(), P<void>(), P<float>(), P<void>(), IMAX, IMAX, IMAX, 1.f, nullptr, nullptr));
  auto blk = [](int n_img) {
    return R::attn_block_fwd(P<void>(), P<void>(), P<void>(), nullptr, P<void>(), nullptr, P<void>(), P<void>(), P<float>(), P<void>(), n_img, 6, 384, 1.f);
  };
  EXPECT(OK, blk(7281)); EXPECT(ARG, blk(7282)); EXPECT(ARG, blk(IMAX));
}

static void gemm() {
  dig_dropout_t drop{};
  drop.thr = 1u << 31;
  drop.scale = 2.f;
  // with dropout the element index I * J is hashed in 32 bits
  auto g = [&](int I, int J, int R_, int lda, int ldb, int ta, int tb, int kind, int splits, const dig_dropout_t* d, int bk = 0, int a_rows = 0) {
    return R::gemm_bf16_dropout(P<void>(), P<void>(), P<void>(), I, J, R_, lda, ldb, J, ta, tb, kind, nullptr, nullptr, 0, nullptr, 0, 1.f, 0, 0, splits, a_rows, 0,
                                bk, nullptr, d);
  };
  EXPECT(OK, g(65535, 65536, 64, 64, 64, 0, 1, 0, 1, &drop)); EXPECT(ARG, g(65536, 65536, 64, 64, 64, 0, 1, 0, 1, &drop));
  EXPECT(OK, g(65536, 65536, 64, 64, 64, 0, 1, 0, 1, nullptr));
  // operands are addressed through 32-bit byte offsets: rows * ld * 2 < 2^32
  EXPECT(OK, g(1 << 20, 128, 64, 2040, 64, 0, 1, 0, 1, nullptr)); EXPECT(ARG, g(1 << 20, 128, 64, 2048, 64, 0, 1, 0, 1, nullptr));
  EXPECT(OK, g(1 << 20, 128, 64, 2048, 64, 0, 1, 0, 1, nullptr, 0, (1 << 20) - 1));      // a_rows bounds the rows that exist
  EXPECT(ARG, g(128, 1 << 20, 64, 64, 2048, 0, 0, 0, 1, nullptr));          // B [J, ldb] when it is not transposed
  // split slabs are whole 64-row K tiles: 716 rows in 8 splits are 6 slabs of 128
  EXPECT(ARG, g(128, 128, 716, 128, 128, 1, 1, 2, 8, nullptr)); EXPECT(OK, g(128, 128, 716, 128, 128, 1, 1, 2, 6, nullptr));
  EXPECT(OK, g(128, 128, IMAX, 0, 0, 1, 1, 2, 1, nullptr)); EXPECT(ARG, g(128, 128, IMAX, 8, 8, 1, 1, 2, 1, nullptr)); EXPECT(ALIGN, g(IMAX, IMAX, IMAX, IMAX, IMAX, 1, 1, 2, IMAX, nullptr));
  EXPECT(ARG, g(IMAX - 7, IMAX - 7, IMAX, IMAX - 7, IMAX - 7, 1, 1, 2, IMAX, nullptr));
  // forms without a kernel
  EXPECT(UNSUP, g(128, 128, 64, 128, 128, 1, 0, 0, 1, nullptr)); EXPECT(UNSUP, g(128, 128, 64, 128, 128, 1, 1, 0, 1, nullptr));
  EXPECT(UNSUP, g(128, 128, 64, 64, 128, 0, 0, 2, 1, nullptr, 64)); EXPECT(OK, g(128, 128, 64, 64, 128, 0, 0, 2, 1, nullptr, 244));
  EXPECT(OK, g(128, 128, 64, 64, 128, 0, 0, 2, 1, nullptr, 564)); EXPECT(UNSUP, g(128, 128, 64, 64, 64, 0, 1, 2, 1, nullptr, 32));
  EXPECT(OK, g(128, 128, 64, 64, 64, 0, 1, 1, 1, nullptr, 244));
  EXPECT(OK, R::sgemm(P<float>(), P<float>(), P<float>(), 8, 8, IMAX, 8, 8, 8, 0, 1.f, 1));
  EXPECT(ARG, R::sgemm(P<float>(), P<float>(), P<float>(), 8, 8, IMAX, 8, 8, 8, 0, 1.f, IMAX));
  EXPECT(OK, R::sgemm(P<float>(), P<float>(), P<float>(), 8, 8, 256, 8, 8, 8, 0, 1.f, 4)); EXPECT(ARG, R::sgemm(P<float>(), P<float>(), P<float>(), 8, 8, 256, 8, 8, 8, 0, 1.f, 3));
  // grouped weight gradient: R * ld * 2 < 2^32 for both operands (host table, read by the rule)
  dig_wgrad_prob_t q{};
  q.A = P<void>(); q.B = P<void>(); q.out = P<float>(); q.lda = 2040; q.ldb = 256; q.ldo = 256; q.I = 128; q.J = 256;
  auto wg = [&](int R_) { return R::wgrad_group(&q, 1, nullptr, 0, R_, 1, P<unsigned>(), 8, P<float>(), nullptr, 1, 2, 1); };
  EXPECT(OK, wg(1 << 20));
  q.lda = 2048; EXPECT(UNSUP, wg(1 << 20));
  q.lda = 128; q.ldb = 2048; EXPECT(UNSUP, wg(1 << 20));
  q.ldb = IMAX - 7; q.lda = IMAX - 7; EXPECT(UNSUP, wg(IMAX - 63));
  EXPECT(ARG, wg(IMAX));
}

static void fused_mlp() {
  dig_dropout_t drop{};
  drop.thr = 1u << 31;
  // D = 384.  Side outputs R * F * 2 < 2^32; the mask hash indexes R * D elements in 32 bits (with dropout only)
  auto ln = [&](int R_, int F, const dig_dropout_t* d) {
    return R::mlp_chain_fwd_ln_dropout(P<void>(), nullptr, nullptr, nullptr, 1e-6f, nullptr, nullptr, nullptr, P<void>(), nullptr, P<void>(), nullptr, P<void>(),
                                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, R_, 384, F, d);
  };
  EXPECT(OK, ln(16777215, 128, nullptr)); EXPECT(UNSUP, ln(16777216, 128, nullptr)); EXPECT(UNSUP, ln(IMAX, 128, nullptr));
  EXPECT(OK, ln(11184810, 128, &drop)); EXPECT(UNSUP, ln(11184811, 128, &drop)); EXPECT(OK, ln(11184811, 128, nullptr));
  EXPECT(OK, ln(1, 2048, nullptr)); EXPECT(UNSUP, ln(1, 2176, nullptr)); EXPECT(UNSUP, ln(1, IMAX, nullptr)); EXPECT(UNSUP, ln(IMAX, IMAX - 127, &drop));
  drop.pthr = 1; drop.rows_per_sample = 0;
  EXPECT(ARG, ln(1, 128, &drop));
  // b1 [F] fp32 in LDS: 7 * 16384 + 4 (F + 384) <= 163840 (F <= 11904), one more 16 KiB slot with the saved pre-activation (F <= 7808)
  auto fwd = [](int F, bool pre) {
    return R::mlp_chain_fwd(P<void>(), P<void>(), nullptr, P<void>(), nullptr, nullptr, P<void>(), pre ? P<void>() : nullptr, pre ? P<void>() : nullptr, 1, 384, F);
  };
  EXPECT(OK, fwd(11904, false)); EXPECT(UNSUP, fwd(12032, false)); EXPECT(OK, fwd(7808, true)); EXPECT(UNSUP, fwd(7936, true));
  EXPECT(UNSUP, fwd(IMAX - 127, false)); EXPECT(UNSUP, fwd(IMAX, true));
  // the LayerNorm phase of the backward: (R + 128) * D * 2 < 2^32
  auto bwd = [](int R_) {
    return R::mlp_chain_bwd_ln_proj(P<void>(), P<void>(), P<void>(), P<void>(), P<void>(), P<void>(), P<float>(), P<float>(), P<float>(), P<void>(), nullptr, P<float>(),
                                    nullptr, nullptr, R_, 384, 128);
  };
  EXPECT(OK, bwd(5592277)); EXPECT(UNSUP, bwd(5592278)); EXPECT(UNSUP, bwd(IMAX));
  EXPECT(UNSUP, R::mlp_chain_bwd(P<void>(), P<void>(), P<void>(), P<void>(), P<void>(), P<void>(), nullptr, IMAX, 384, IMAX - 127));
}

static void resizes() {
  // coefficient tables in LDS: out_w (ksh + 2) + out_h (ksv + 2) ints, ks = 2 ceil(2 max / out) + 1.  out 32 x 128, max_h 32 (ksv 5):
  // plain resize  <= 40960 ints: ksh <= 316, max_w <= 10048;   key-view stage B (+ 32 bytes of sums + the 12288-byte image): <= 37880 ints,
  // ksh <= 292, max_w <= 9280;   ABINet tail (+ 32 bytes): <= 40952 ints, max_ww <= 10048
  auto rs = [](int max_h, int max_w, int oh = 32, int ow = 128) {
    return R::resize_bicubic_normalize_u8(P<unsigned char>(), P<long long>(), P<int>(), P<int>(), 1, P<float>(), oh, ow, 0.5f, 0.5f, max_h, max_w);
  };
  EXPECT(OK, rs(32, 10048)); EXPECT(UNSUP, rs(32, 10049)); EXPECT(UNSUP, rs(IMAX, IMAX)); EXPECT(UNSUP, rs(IMAX, IMAX, 1, 1)); EXPECT(UNSUP, rs(32, 32, IMAX, IMAX));
  auto kb = [](int max_h, int max_w, int oh = 32, int ow = 128) {
    return R::keyview_stage_b(P<unsigned char>(), P<long long>(), P<int>(), P<int>(), 1, P<dig_kv_params>(), P<float>(), oh, ow, 0.5f, 0.5f, max_h, max_w);
  };
  EXPECT(OK, kb(32, 9280)); EXPECT(UNSUP, kb(32, 9281)); EXPECT(UNSUP, kb(IMAX, IMAX)); EXPECT(UNSUP, kb(IMAX, IMAX, 1, 1)); EXPECT(UNSUP, kb(32, 32, IMAX, IMAX));
  dig_abi_run run{};
  run.mb_size = 1;
  auto tail = [&](int max_wh, int max_ww) {
    return R::abiaug_tail(P<unsigned char>(), P<long long>(), P<int>(), P<int>(), 1, P<dig_abi_params>(), &run, nullptr, 0, P<float>(), 32, 128, 0.5f, 0.5f, max_wh,
                          max_ww);
  };
  EXPECT(OK, tail(32, 10048)); EXPECT(UNSUP, tail(32, 10049)); EXPECT(UNSUP, tail(IMAX, IMAX));
  run.mb_size = 0;
  EXPECT(ARG, tail(32, 32));
  // stage A keeps two 3-byte-per-pixel images in its workspace: max_h * max_w * 3 <= work_bytes / 2
  auto ka = [](int h, int w, long long bytes) {
    return R::keyview_stage_a_u8(P<unsigned char>(), P<long long>(), P<int>(), P<int>(), 1, P<dig_kv_params>(), P<unsigned char>(), bytes, h, w);
  };
  EXPECT(OK, ka(5, 17, 512)); EXPECT(ARG, ka(2, 43, 512)); EXPECT(ARG, ka(IMAX, IMAX, 512)); EXPECT(ARG, ka(IMAX, IMAX, LLONG_MAX - 511));
  EXPECT(OK, ka(1 << 15, 1 << 15, 6LL << 30));
}

static void the_rest() {
  // additive attention backward over T tokens: 4 T (width + 64) <= 153600 for both widths
  auto at = [](int T, int A, int X) {
    return R::addattn_bwd_tokens(P<void>(), P<void>(), P<float>(), P<float>(), P<float>(), P<void>(), 8, P<void>(), P<void>(), T, 1, 1, A, X);
  };
  EXPECT(OK, at(300, 64, 64)); EXPECT(UNSUP, at(301, 64, 64)); EXPECT(UNSUP, at(300, 64, 66)); EXPECT(UNSUP, at(IMAX, IMAX - 1, IMAX - 1));
  EXPECT(OK, R::addattn_fwd_slots(P<void>(), P<void>(), P<float>(), P<void>(), nullptr, P<void>(), 8, 1, 512, 1024, 8, 8));
  EXPECT(UNSUP, R::addattn_fwd_slots(P<void>(), P<void>(), P<float>(), P<void>(), nullptr, P<void>(), 8, 1, 513, 1024, 8, 8));
  EXPECT(UNSUP, R::addattn_fwd_slots(P<void>(), P<void>(), P<float>(), P<void>(), nullptr, P<void>(), 8, 1, 512, 1032, 8, 8));
  EXPECT(UNSUP, R::addattn_fwd_slots(P<void>(), P<void>(), P<float>(), P<void>(), nullptr, P<void>(), 8, 1, 512, 1024, 8, 9));
  // the dropout mask hashes rows * cols element indices in 32 bits
  dig_dropout_t drop{};
  EXPECT(OK, R::dropout_apply(P<void>(), P<void>(), (1LL << 29) - 1, 8, &drop)); EXPECT(ARG, R::dropout_apply(P<void>(), P<void>(), 1LL << 29, 8, &drop));
  EXPECT(ARG, R::dropout_apply(P<void>(), P<void>(), LLONG_MAX, IMAX - 7, &drop));
  EXPECT(OK, R::ce_rows_ws(P<float>(), IMAX, IMAX, 0, 1.f, P<float>(), nullptr)); EXPECT(ARG, R::ce_rows_ws(P<float>(), IMAX, IMAX, 1, 1.f, P<float>(), nullptr));
  EXPECT(ARG, R::ce_rows_ws(P<float>(), IMAX, IMAX, IMAX, 1.f, P<float>(), nullptr));
  EXPECT(ARG, R::im2col3x3(P<void>(), P<void>(), 1, 2, 2, IMAX - 7, IMAX - 7)); EXPECT(OK, R::im2col3x3(P<void>(), P<void>(), 1, 2, 2, 8, 72));
  EXPECT(OK, R::random_masks(P<unsigned char>(), 1, 16384, 1, 0, 0)); EXPECT(ARG, R::random_masks(P<unsigned char>(), 1, 16385, 1, 0, 0));
  EXPECT(OK, R::bn_fwd_fused(P<void>(), 1e-5f, nullptr, nullptr, 0, P<void>(), P<float>(), P<float>(), 0.1f, nullptr, nullptr, 4096, 256));
  EXPECT(UNSUP, R::bn_fwd_fused(P<void>(), 1e-5f, nullptr, nullptr, 0, P<void>(), P<float>(), P<float>(), 0.1f, nullptr, nullptr, 4097, 256));
  EXPECT(UNSUP, R::bn_fwd_fused(P<void>(), 1e-5f, nullptr, nullptr, 0, P<void>(), P<float>(), P<float>(), 0.1f, nullptr, nullptr, IMAX, IMAX));
  EXPECT(ARG, R::bn_bwd_apply(P<void>(), P<void>(), P<float>(), P<float>(), nullptr, nullptr, 0, P<float>(), 2.f, P<void>(), 2, 0));
  EXPECT(ARG, R::bn_bwd_apply(P<void>(), P<void>(), P<float>(), P<float>(), nullptr, nullptr, 0, P<float>(), 2.f, P<void>(), 2, -8));
  EXPECT(ARG, R::bn_bwd_apply(P<void>(), P<void>(), P<float>(), P<float>(), nullptr, nullptr, 0, P<float>(), 2.f, P<void>(), 2, INT_MIN));
  auto tcv = [](int N, int Lq) {
    return R::tcv_attn_fwd(P<void>(), P<void>(), P<void>(), P<void>(), P<float>(), P<float>(), 1e-5f, P<void>(), P<float>(), nullptr, 1, Lq, N, 6, 384, 1, nullptr);
  };
  EXPECT(OK, tcv(256, 32)); EXPECT(UNSUP, tcv(257, 32)); EXPECT(UNSUP, tcv(256, 33)); EXPECT(UNSUP, tcv(IMAX, IMAX));
  // the queries the rules lean on, at the ends of their range
  if (R::gemm_effective_splits(65536, 18) != 18 || R::gemm_effective_splits(716, 8) != 6 || R::gemm_effective_splits(IMAX, 1) != 1 ||
      R::layernorm_bwd_parts(IMAX) != 1024 || R::layernorm_bwd_parts(1) != 1 || R::mlp_chain_ln_parts(IMAX) != 16777216 ||
      R::wgrad_group_effective_splits(IMAX - 63, IMAX) != 33554431 || R::wgrad_group_tiles(IMAX - 127, 256, 2, 1) != 16777215 ||
      R::ksize_for(32, 32) != 5 || R::ksize_for(10048, 128) != 315 || R::ksize_for(10049, 128) != 317 ||
      R::mse_workspace_bytes() != 1028 || R::ce_rows_workspace_bytes(IMAX) != 4 + 12LL * IMAX || R::ce_rows_workspace_bytes(0) != 4 ||
      R::tcv_attn_bwd_workspace_bytes(IMAX, 32, 8, 512) != 4LL * IMAX * 32 * 1032 || R::tcv_attn_bwd_workspace_bytes(IMAX, IMAX, IMAX, IMAX) != 0) {
    ++failures;
    std::printf("a query disagrees with its documented value\n");
  }
}

int main() {
  sequence_attention();
  labels_and_beams();
  encoder_attention();
  gemm();
  fused_mlp();
  resizes();
  the_rest();
  if (failures) { std::printf("abi_rules_main: %d of %d checks FAILED\n", failures, checks); return 1; }
  std::printf("abi_rules_main: all checks passed (%d)\n", checks);
  return 0;
}
