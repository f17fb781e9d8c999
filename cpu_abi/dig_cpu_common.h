// What every file of libdig_cpu.so shares: the ABI itself (include/dig_hip.h -- its types, limits and error codes; every entry point
// defined here is compiled against its declaration, so a definition whose argument list drifts from the header does not build), the
// argument rules of the ABI (dig_amd/csrc/abi_rules.h -- the very text the HIP build compiles: every entry point here opens with its
// dig_rules:: call and holds no refusal of its own, so a refusal test that passes on this build speaks for the product) and the storage
// helpers of the HIP build's common.h in plain C++.  The arithmetic behind the rules stays this build's own: it is the second opinion.
#pragma once
#include <cstdint>
#include <cstring>

#include "../include/dig_hip.h"
#include "../dig_amd/csrc/abi_rules.h"   // aligned16 / ranges_overlap, the limits, dig_rules::NAME for every entry point

typedef uint16_t bf16_t;

inline float bf2f(bf16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline bf16_t f2bf(float f) {                       // round to nearest even, as v_cvt_pk_bf16_f32
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}
inline unsigned drop_hash(unsigned k0, unsigned k1, unsigned a, unsigned b) {
  unsigned x = a ^ k0;
  x ^= x >> 16; x *= 0x7feb352du;
  x += k1 + b * 0x9e3779b9u;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
inline bool drop_keep(unsigned k0, unsigned k1, unsigned a, unsigned b, unsigned thr) { return drop_hash(k0, k1, a, b) >= thr; }
