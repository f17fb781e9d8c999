// What every file of libdig_cpu.so shares: the ABI itself (include/dig_hip.h -- its types, limits and error codes; every entry point
// defined here is compiled against its declaration, so a definition whose argument list drifts from the header does not build) and the
// storage helpers of the HIP build's common.h in plain C++.
#pragma once
#include <cstdint>
#include <cstring>

#include "../include/dig_hip.h"

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
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
inline bool ranges_overlap(const void* a, const void* b, size_t bytes) {      // [a, a + bytes) and [b, b + bytes) share a byte
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
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
