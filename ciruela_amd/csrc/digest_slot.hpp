// A 32-byte digest in registers and its home slot in an open-addressing
// table: what the digest joins on the device share (join.hip, repeats.hip).
// Device code only.
//
// The home slot folds all 32 bytes of a digest under the caller's seed
// (digests come from other parties' indexes: digests crafted to share a prefix
// must not share a home slot, and a caller that joins untrusted digests passes
// a seed they cannot predict):
//   x = seed; for the four little-endian u64 words w of the digest, in order:
//   x = (x ^ w) * 0x9E3779B97F4A7C15, x ^= x >> 32;  home = x & (slots - 1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cir {
namespace dev {

struct Digest {
  uint4 lo, hi;
};

__device__ __forceinline__ Digest load_digest(const uint8_t* __restrict__ base, uint64_t i) {
  const uint4* p = reinterpret_cast<const uint4*>(base + 32 * i);
  Digest d;
  d.lo = p[0];
  d.hi = p[1];
  return d;
}

__device__ __forceinline__ bool same_digest(const Digest& a, const Digest& b) {
  const uint32_t diff = (a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) |
                        (a.lo.w ^ b.lo.w) | (a.hi.x ^ b.hi.x) | (a.hi.y ^ b.hi.y) |
                        (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w);
  return diff == 0;
}

__device__ __forceinline__ uint64_t mix_word(uint64_t x, uint32_t lo, uint32_t hi) {
  x = (x ^ ((uint64_t)lo | ((uint64_t)hi << 32))) * 0x9E3779B97F4A7C15ull;
  return x ^ (x >> 32);
}

__device__ __forceinline__ uint64_t home_slot(const Digest& d, uint64_t seed, uint64_t mask) {
  uint64_t x = seed;
  x = mix_word(x, d.lo.x, d.lo.y);
  x = mix_word(x, d.lo.z, d.lo.w);
  x = mix_word(x, d.hi.x, d.hi.y);
  x = mix_word(x, d.hi.z, d.hi.w);
  return x & mask;
}

}  // namespace dev
}  // namespace cir
