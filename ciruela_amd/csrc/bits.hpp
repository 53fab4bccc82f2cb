// Bit runs between bitmaps of 64-bit words (bit i of a bitmap = bit (i & 63)
// of word i >> 6).  cir_check_blocks copies each run of a batch's verdicts
// (kernels.hpp launch_block_bits) into the image's bitmap; a run starts on a
// word boundary on neither side.  Host only, no dependencies: tools/
// bits_fuzz.cpp checks it against a bit-by-bit loop.
#pragma once
#include <stdint.h>

namespace cir {

// The k bits (1 <= k <= 64) of src from bit sbit on, in the low bits of the
// result.  Reads only words that hold one of those bits.
inline uint64_t get_bits(const uint64_t* src, uint64_t sbit, unsigned k) {
  const uint64_t w = sbit >> 6;
  const unsigned sh = (unsigned)(sbit & 63);
  uint64_t v = src[w] >> sh;
  if (sh + k > 64) v |= src[w + 1] << (64 - sh);  // (sh > 0 here)
  return k == 64 ? v : v & ((1ull << k) - 1);
}

// dst[dbit .. dbit + count) = src[sbit .. sbit + count); every other bit of
// dst stays as it is, and no word of either side that holds none of the
// run's bits is touched.  The two bitmaps must not overlap.
inline void copy_bits(uint64_t* dst, uint64_t dbit, const uint64_t* src, uint64_t sbit,
                      uint64_t count) {
  while (count > 0) {
    const unsigned dsh = (unsigned)(dbit & 63);
    const unsigned k = (unsigned)(count < 64u - dsh ? count : 64u - dsh);
    const uint64_t mask = (k == 64 ? ~0ull : (1ull << k) - 1) << dsh;
    uint64_t& w = dst[dbit >> 6];
    w = (w & ~mask) | (get_bits(src, sbit, k) << dsh);
    dbit += k;
    sbit += k;
    count -= k;
  }
}

// How many of the bits [bit, bit + count) are set.
inline uint64_t count_bits(const uint64_t* src, uint64_t bit, uint64_t count) {
  uint64_t n = 0;
  while (count > 0) {
    const unsigned k = (unsigned)(count < 64 ? count : 64);
    n += (uint64_t)__builtin_popcountll(get_bits(src, bit, k));
    bit += k;
    count -= k;
  }
  return n;
}

// How many bits from `bit` on, at most count, equal `value` in a row.
inline uint64_t run_bits(const uint64_t* src, uint64_t bit, uint64_t count, bool value) {
  uint64_t n = 0;
  while (n < count) {
    const unsigned k = (unsigned)(count - n < 64 ? count - n : 64);
    uint64_t v = get_bits(src, bit + n, k);
    if (value) v = ~v;  // (the first bit that differs is the lowest set one)
    if (k < 64) v &= (1ull << k) - 1;
    if (v) return n + (uint64_t)__builtin_ctzll(v);
    n += k;
  }
  return count;
}

// Clear the bits [bit, bit + count).
inline void clear_bits(uint64_t* dst, uint64_t bit, uint64_t count) {
  while (count > 0) {
    const unsigned sh = (unsigned)(bit & 63);
    const unsigned k = (unsigned)(count < 64u - sh ? count : 64u - sh);
    dst[bit >> 6] &= ~((k == 64 ? ~0ull : (1ull << k) - 1) << sh);
    bit += k;
    count -= k;
  }
}

}  // namespace cir
