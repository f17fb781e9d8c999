// Decode with a K/V cache: the per-step pieces of TFDecoder.forward_test (greedy) and of the two beam searches
// (models/decoder.py:224-252) that are not GEMMs / LayerNorms.  The reference re-runs the whole decoder over all 26 positions
// at every one of the 25 steps; position t only depends on tokens <= t, so the device path feeds one token per step, keeps
// the self-attention keys/values of each layer in HBM ([B, T, 3*H*dk] bf16: the fused q|k|v projection writes row t in place)
// and projects the cross-attention keys/values of the encoder memory once per layer.
//
//   dig_decode_embed       x[b,:] = trg_word_emb[token[b],:] + position_table[t,:]              (decoder.py:173-181)
//   dig_decode_self_attn   one query (row t) against cached rows 0..t, per (sample, head)        (transformer_layer.py:238-281)
//   dig_decode_cross_attn  one query against the Nm memory keys/values, per (sample, head); optional per-head weights
//   dig_softmax_argmax     probabilities + greedy token of a logit row                           (decoder.py:238-246)
//   dig_beam_step          one step of TFDecoder.beam_search: rank the candidates, keep the beam's books        (decoder.py:283-307)
//   dig_attn_beam_advance  the same ranking for the GRU attention head, + its state gather and next input rows  (attn_decoder.py:116-138)
// The string metrics are in metrics.hip, the sequence losses in seq_loss.hip.
// Head dimension d_k = d_v = 64 (`tf_decoder`, `small_tf_decoder`, `corres_base_tf_decoder`), 48 (`corres_small_tf_decoder`) or 24
// (`corres_tiny_tf_decoder`): a template parameter of the two attention kernels, heads are not padded.  All HBM-bound and tiny; one
// wave (self) or four waves (cross) per (sample, head), fp32 softmax.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "row_ops.h"

namespace {

__global__ __launch_bounds__(256) void embed_kernel(const long long* __restrict__ tok, const float* __restrict__ emb,
                                                    const float* __restrict__ pe_row, bf16_t* __restrict__ x, int B, int d, int vocab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * d) return;
  const int b = i / d, c = i - b * d;
  const long long t = clamp_class(tok[b], vocab);
  x[i] = f2bf(emb[(size_t)t * d + c] + pe_row[c]);
}

// qkv: [B, T, 3*hk] bf16 (q | k | v), row t holds this step's projections; out: [B, hk] bf16.  One wave, lane = channel: at head dim
// 24 / 48 the lanes >= DK read channel 0 (never past the head: the last head's v columns end the row), carry a zero query and write nothing.
template <int DK>
__global__ __launch_bounds__(64) void self_attn_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int T, int hk, int t,
                                                       float scale) {
  const int b = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  const bool live = DK == 64 || lane < DK;
  const size_t row = (size_t)3 * hk;
  const bf16_t* base = qkv + (size_t)b * T * row + h * DK + (live ? lane : 0);
  const float q = live ? bf2f(base[(size_t)t * row]) * scale : 0.f;
  float m = -INFINITY, l = 0.f, acc = 0.f;                             // online softmax over the t+1 cached positions
  for (int j = 0; j <= t; ++j) {
    const float s = wave_sum(q * bf2f(base[(size_t)j * row + hk]));
    const float mn = fmaxf(m, s);
    const float c = __expf(m - mn), p = __expf(s - mn);
    l = l * c + p;
    acc = acc * c + p * bf2f(base[(size_t)j * row + 2 * hk]);
    m = mn;
  }
  if (live) out[(size_t)b * hk + h * DK + lane] = f2bf(acc / l);
}

// q: [B, hk] bf16; kv: [B, Nm, 2*hk] bf16 (k | v); out: [B, hk] bf16; weights (optional): [B, H, Nm] fp32
// 256 threads = 32 key slots x 8 channel chunks: a lane loads 16 bytes (8 channels) of one key row, so 8 consecutive lanes
// cover a whole 128-byte row and every load instruction of a wave moves 8 full rows (coalesced; the first version gave each
// thread its own row and ran at 1.8 TB/s).  Scores: partial dot over the lane's 8 channels + 3 shuffles.  Values: each lane
// accumulates its 8 channels over its key slot's keys, then shuffles / LDS combine the 32 slots.  At head dim 24 / 48 a row has
// DK / 8 = 3 / 6 chunks: a key slot keeps its 8 lanes (the three shuffles stay inside the slot), the surplus lanes (chunk >= DK / 8) load
// nothing and add zero.
template <int DK>
__global__ __launch_bounds__(256) void cross_attn_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, bf16_t* __restrict__ out,
                                                         float* __restrict__ weights, int Nm, int hk, float scale, int slots_per_mem) {
  extern __shared__ float sm[];                                        // [Nm] scores / probabilities, then [4][DK] partial outputs
  __shared__ float red[8];
  const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, H = gridDim.y;
  const int chunk = tid & 7, slot = tid >> 3;                           // 8 channels [chunk*8, +8); keys slot, slot+32, ...
  const bool live = DK == 64 || chunk < DK / 8;
  float qv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qv[e] = 0.f;
  if (live) {
    const uint4 v = *reinterpret_cast<const uint4*>(q + (size_t)b * hk + h * DK + chunk * 8);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { qv[2 * e] = bf2f((bf16_t)(w[e] & 0xffff)) * scale; qv[2 * e + 1] = bf2f((bf16_t)(w[e] >> 16)) * scale; }
  }
  const bf16_t* kb = kv + (size_t)(b / slots_per_mem) * Nm * 2 * hk + h * DK + chunk * 8;   // beam search: `slots_per_mem` queries share a memory
  float lmax = -INFINITY;
  for (int j = slot; j < Nm; j += 32) {
    float s = 0.f;
    if (live) {
      const uint4 v = *reinterpret_cast<const uint4*>(kb + (size_t)j * 2 * hk);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) s += qv[2 * e] * bf2f((bf16_t)(w[e] & 0xffff)) + qv[2 * e + 1] * bf2f((bf16_t)(w[e] >> 16));
    }
    s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
    if (chunk == 0) sm[j] = s;
    lmax = fmaxf(lmax, s);
  }
  lmax = wave_max(lmax);
  if ((tid & 63) == 0) red[tid >> 6] = lmax;
  __syncthreads();
  const float gmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float lsum = 0.f;
  for (int j = tid; j < Nm; j += 256) {
    const float p = __expf(sm[j] - gmax);
    sm[j] = p;
    lsum += p;
  }
  lsum = wave_sum(lsum);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = lsum;
  __syncthreads();
  const float inv = 1.f / (red[4] + red[5] + red[6] + red[7]);
  if (weights)
    for (int j = tid; j < Nm; j += 256) weights[((size_t)b * H + h) * Nm + j] = sm[j] * inv;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int j = slot; live && j < Nm; j += 32) {
    const uint4 v = *reinterpret_cast<const uint4*>(kb + (size_t)j * 2 * hk + hk);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    const float p = sm[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) { acc[2 * e] += p * bf2f((bf16_t)(w[e] & 0xffff)); acc[2 * e + 1] += p * bf2f((bf16_t)(w[e] >> 16)); }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {                                         // combine the 8 key slots of this wave (lanes differ in bits 3..5)
    acc[e] += __shfl_xor(acc[e], 8, 64); acc[e] += __shfl_xor(acc[e], 16, 64); acc[e] += __shfl_xor(acc[e], 32, 64);
  }
  __syncthreads();                                                      // probabilities are no longer needed
  float* part = sm;
  if ((tid & 63) < 8 && live) {
#pragma unroll
    for (int e = 0; e < 8; ++e) part[(tid >> 6) * DK + chunk * 8 + e] = acc[e];
  }
  __syncthreads();
  if (tid < DK) out[(size_t)b * hk + h * DK + tid] = f2bf((part[tid] + part[DK + tid] + part[2 * DK + tid] + part[3 * DK + tid]) * inv);
}

// one wave per row: probs[b, :C] = softmax(logits[b, :C]); token[b] = first index of the maximum (torch.max semantics)
__global__ __launch_bounds__(64) void softmax_argmax_kernel(const float* __restrict__ logits, int ld, float* __restrict__ probs,
                                                            long long* __restrict__ token, int C) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* row = logits + (size_t)b * ld;
  float m;
  int am;
  row_argmax_first(row, C, lane, m, am);
  const float inv = 1.f / row_exp_sum(row, C, lane, m);
  for (int c = lane; c < C; c += 64) probs[(size_t)b * C + c] = __expf(row[c] - m) * inv;
  if (lane == 0) token[b] = am == 0x7fffffff ? 0 : am;                  // no entry above -inf: index 0, as torch.max
}

// The ranking of one beam-search step for one sample (TFDecoder.beam_search, decoder.py:283-307), the one copy both kernels below run:
// log-softmax of its `bw` slots' logits, + the slots' running scores, top-`bw` of the bw*C candidates (ties: the lower candidate index,
// i.e. torch.topk's result wherever it is defined), then the bookkeeping of that step: symbol = candidate % C, predecessor =
// candidate / C + b*bw, stored score, and the running score that the next step starts from (-inf once a slot has emitted EOS, :299-301).
// One 256-thread workgroup; bw <= 16.  cand: LDS [bw * C].  forced (nullable): candidate indices that stand in for the top-bw search.
// sym_s / pred_s (nullable, LDS [bw]): symbol and predecessor row of every slot, for what the caller does after the final barrier.
__device__ __forceinline__ void beam_rank(const float* __restrict__ logits, int ld, float* __restrict__ seq_scores, int bw, int C, int eos,
                                          long long* __restrict__ symbols, long long* __restrict__ preds, float* __restrict__ stored,
                                          const long long* __restrict__ forced, float* cand, int* sym_s, int* pred_s) {
  __shared__ float lse[16];
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = wave; k < bw; k += 4) {                                   // a wave per slot: log-sum-exp of the row
    float m, s;
    row_max_sum(logits + (size_t)(b * bw + k) * ld, C, lane, m, s);
    if (lane == 0) lse[k] = m + __logf(s);
  }
  __syncthreads();
  const int n = bw * C;
  for (int i = tid; i < n; i += 256) {
    const int k = i / C, c = i - k * C;
    cand[i] = seq_scores[b * bw + k] + (logits[(size_t)(b * bw + k) * ld + c] - lse[k]);
  }
  __syncthreads();
  for (int r = 0; r < bw; ++r) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (!forced) {
      for (int i = tid; i < n; i += 256) {
        const float v = cand[i];
        if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
      }
      wave_argmax_first(bv, bi);
      if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
      __syncthreads();
    }
    if (tid == 0) {
      if (forced) {
        bi = (int)clamp_class(forced[b * bw + r], n);
        bv = cand[bi];
      } else {
        for (int w = 1; w < 4; ++w)
          if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
        if (bi == 0x7fffffff) bi = r;                                      // every candidate is NaN / -inf and already taken: keep indices valid
        cand[bi] = -INFINITY;                                              // taken (a -inf candidate can be taken again: the reference's
      }                                                                    //  order among -inf ties is unspecified as well)
      const int sym = bi % C;
      symbols[b * bw + r] = sym;
      preds[b * bw + r] = bi / C + b * bw;
      stored[b * bw + r] = bv;
      seq_scores[b * bw + r] = sym == eos ? -INFINITY : bv;
      if (sym_s) { sym_s[r] = sym; pred_s[r] = bi / C + b * bw; }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void beam_step_kernel(const float* __restrict__ logits, int ld, float* __restrict__ seq_scores, int bw, int C,
                                                        int eos, long long* __restrict__ symbols, long long* __restrict__ preds,
                                                        float* __restrict__ stored) {
  extern __shared__ float cand[];                                       // [bw * C]
  beam_rank(logits, ld, seq_scores, bw, C, eos, symbols, preds, stored, nullptr, cand, nullptr, nullptr);
}

// What closes a step of AttentionRecognitionHead.beam_search (attn_decoder.py:116-138) for one sample, in one launch: the ranking, then
// what the GRU head's next step needs and the transformer decoder's does not -- the recurrent state of slot j becomes the state of its
// predecessor (fp32 and bf16 copies, gathered into buffers distinct from their sources), and the embedding of the symbol slot j emitted
// goes into columns [0, E) of its GRU input row.  bw <= 8.
__global__ __launch_bounds__(256) void attn_beam_advance_kernel(const float* __restrict__ logits, int ld, float* __restrict__ seq_scores, int bw, int C,
                                                                int eos, long long* __restrict__ symbols, long long* __restrict__ preds,
                                                                float* __restrict__ stored, const long long* __restrict__ forced,
                                                                const float* __restrict__ s_in, const bf16_t* __restrict__ sbf_in,
                                                                float* __restrict__ s_out, bf16_t* __restrict__ sbf_out, int S,
                                                                const float* __restrict__ table, int E, bf16_t* __restrict__ inp, int ld_inp) {
  extern __shared__ float cand[];                                       // [bw * C]
  __shared__ int sym_s[8], pred_s[8];
  const int b = blockIdx.x, tid = threadIdx.x;
  beam_rank(logits, ld, seq_scores, bw, C, eos, symbols, preds, stored, forced, cand, sym_s, pred_s);
  // pred_s[j] - b*bw < bw and sym_s[j] < C: the sources below are rows of this sample's slots and of the table's first C rows
  const size_t row0 = (size_t)b * bw;
  for (int i = tid; i < bw * S; i += 256) {
    const int j = i / S, c = i - j * S;
    const size_t src = (size_t)pred_s[j] * S + c, dst = (row0 + j) * S + c;
    s_out[dst] = s_in[src];
    sbf_out[dst] = sbf_in[src];
  }
  for (int i = tid; i < bw * E; i += 256) {
    const int j = i / E, c = i - j * E;
    inp[(row0 + j) * ld_inp + c] = f2bf(table[(size_t)sym_s[j] * E + c]);
  }
}

}  // namespace

// C-ABI: see include/dig_hip.h
extern "C" int dig_decode_embed(const long long* tokens, const float* emb, const float* pe_row, void* x, int B, int d, int vocab,
                                hipStream_t stream) {
  if (int rc = dig_rules::decode_embed(tokens, emb, pe_row, x, B, d, vocab)) return rc;
  hipLaunchKernelGGL(embed_kernel, dim3((B * d + 255) / 256), dim3(256), 0, stream, tokens, emb, pe_row, (bf16_t*)x, B, d, vocab);
  return dig_check_launch();
}

extern "C" int dig_decode_self_attn(const void* qkv_cache, void* out, int B, int T, int heads, int head_dim, int t, float scale,
                                    hipStream_t stream) {
  if (int rc = dig_rules::decode_self_attn(qkv_cache, out, B, T, heads, head_dim, t, scale)) return rc;
  const bf16_t* in = (const bf16_t*)qkv_cache;
  const int hk = heads * head_dim;
  if (head_dim == 64) hipLaunchKernelGGL(self_attn_kernel<64>, dim3(B, heads), dim3(64), 0, stream, in, (bf16_t*)out, T, hk, t, scale);
  else if (head_dim == 48) hipLaunchKernelGGL(self_attn_kernel<48>, dim3(B, heads), dim3(64), 0, stream, in, (bf16_t*)out, T, hk, t, scale);
  else if (head_dim == 24) hipLaunchKernelGGL(self_attn_kernel<24>, dim3(B, heads), dim3(64), 0, stream, in, (bf16_t*)out, T, hk, t, scale);
  else return DIG_ERR_UNSUPPORTED;   // unreachable: abi_rules.h
  return dig_check_launch();
}

extern "C" int dig_decode_cross_attn(const void* q, const void* kv_mem, void* out, float* weights, int B, int n_mem, int heads,
                                     int head_dim, float scale, int slots_per_mem, hipStream_t stream) {
  if (int rc = dig_rules::decode_cross_attn(q, kv_mem, out, weights, B, n_mem, heads, head_dim, scale, slots_per_mem)) return rc;
  const size_t lds = (size_t)std::max(n_mem, 4 * head_dim) * sizeof(float);
  const bf16_t* qp = (const bf16_t*)q;
  const bf16_t* kv = (const bf16_t*)kv_mem;
  const int hk = heads * head_dim;
  if (head_dim == 64) hipLaunchKernelGGL(cross_attn_kernel<64>, dim3(B, heads), dim3(256), lds, stream, qp, kv, (bf16_t*)out, weights, n_mem, hk, scale, slots_per_mem);
  else if (head_dim == 48) hipLaunchKernelGGL(cross_attn_kernel<48>, dim3(B, heads), dim3(256), lds, stream, qp, kv, (bf16_t*)out, weights, n_mem, hk, scale, slots_per_mem);
  else hipLaunchKernelGGL(cross_attn_kernel<24>, dim3(B, heads), dim3(256), lds, stream, qp, kv, (bf16_t*)out, weights, n_mem, hk, scale, slots_per_mem);
  return dig_check_launch();
}

extern "C" int dig_softmax_argmax(const float* logits, int ld, float* probs, long long* tokens, int B, int C, hipStream_t stream) {
  if (int rc = dig_rules::softmax_argmax(logits, ld, probs, tokens, B, C)) return rc;
  hipLaunchKernelGGL(softmax_argmax_kernel, dim3(B), dim3(64), 0, stream, logits, ld, probs, tokens, C);
  return dig_check_launch();
}

extern "C" int dig_beam_step(const float* logits, int ld, float* seq_scores, int B, int beam_width, int C, int eos, long long* symbols,
                             long long* predecessors, float* stored_scores, hipStream_t stream) {
  if (int rc = dig_rules::beam_step(logits, ld, seq_scores, B, beam_width, C, eos, symbols, predecessors, stored_scores)) return rc;
  hipLaunchKernelGGL(beam_step_kernel, dim3(B), dim3(256), (size_t)beam_width * C * sizeof(float), stream, logits, ld, seq_scores, beam_width, C,
                     eos, symbols, predecessors, stored_scores);
  return dig_check_launch();
}

extern "C" int dig_attn_beam_advance(const float* logits, int ld, float* seq_scores, int B, int beam_width, int C, int eos, long long* symbols,
                                     long long* predecessors, float* stored_scores, const long long* force_candidates, const float* s_in,
                                     const void* sbf_in, float* s_out, void* sbf_out, int S, const float* table, int E, void* inp, int ld_inp,
                                     hipStream_t stream) {
  if (int rc = dig_rules::attn_beam_advance(logits, ld, seq_scores, B, beam_width, C, eos, symbols, predecessors, stored_scores, force_candidates,
                                            s_in, sbf_in, s_out, sbf_out, S, table, E, inp, ld_inp))
    return rc;
  hipLaunchKernelGGL(attn_beam_advance_kernel, dim3(B), dim3(256), (size_t)beam_width * C * sizeof(float), stream, logits, ld, seq_scores, beam_width, C,
                     eos, symbols, predecessors, stored_scores, force_candidates, s_in, (const bf16_t*)sbf_in, s_out, (bf16_t*)sbf_out, S, table, E,
                     (bf16_t*)inp, ld_inp);
  return dig_check_launch();
}
