// Seeded fuzz of ciruela_amd/csrc/bits.hpp (the bit-run copy of
// cir_check_blocks) against a bit-by-bit loop.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/bits_fuzz.cpp -o build/bits_fuzz
// and run it; tests/test_check_blocks_cpu.py does.  Source and destination
// are heap buffers of exactly the words a run touches, so a read or a write
// one word outside it is an AddressSanitizer report.
//
// usage: bits_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bits.hpp"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

static bool bit(const std::vector<uint64_t>& v, uint64_t i) { return v[i >> 6] >> (i & 63) & 1; }

static int one(uint64_t sbit, uint64_t dbit, uint64_t count) {
  // exactly the words [first, last] of the run on either side, shifted so
  // that the buffers start at the run's first word
  const uint64_t s0 = sbit & 63, d0 = dbit & 63;
  std::vector<uint64_t> src(count ? (s0 + count + 63) / 64 : 0);
  std::vector<uint64_t> dst(count ? (d0 + count + 63) / 64 : 0);
  for (uint64_t& w : src) w = rnd();
  for (uint64_t& w : dst) w = rnd();
  const std::vector<uint64_t> before = dst;
  cir::copy_bits(dst.data(), d0, src.data(), s0, count);
  for (uint64_t i = 0; i < dst.size() * 64; ++i) {
    const bool in = i >= d0 && i < d0 + count;
    const bool want = in ? bit(src, s0 + (i - d0)) : bit(before, i);
    if (bit(dst, i) != want) {
      fprintf(stderr, "copy_bits(sbit %llu, dbit %llu, count %llu): bit %llu is %d\n",
              (unsigned long long)s0, (unsigned long long)d0, (unsigned long long)count,
              (unsigned long long)i, (int)bit(dst, i));
      return 1;
    }
  }
  uint64_t ones = 0;
  for (uint64_t i = 0; i < count; ++i) ones += bit(src, s0 + i);
  if (cir::count_bits(src.data(), s0, count) != ones) {
    fprintf(stderr, "count_bits(bit %llu, count %llu) is wrong\n", (unsigned long long)s0,
            (unsigned long long)count);
    return 1;
  }
  std::vector<uint64_t> cleared = before;
  cir::clear_bits(cleared.data(), d0, count);
  for (uint64_t i = 0; i < cleared.size() * 64; ++i)
    if (bit(cleared, i) != (i >= d0 && i < d0 + count ? false : bit(before, i))) {
      fprintf(stderr, "clear_bits(bit %llu, count %llu): bit %llu\n", (unsigned long long)d0,
              (unsigned long long)count, (unsigned long long)i);
      return 1;
    }
  return 0;
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20240607;
  uint64_t ran = 0;
  // every offset pair at the counts where a path changes: none, one bit, up
  // to and across a word, and runs that span three words on either side
  static const uint64_t kCounts[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193};
  for (uint64_t c : kCounts)
    for (uint64_t s = 0; s < 64; s += (s < 3 || s > 60) ? 1 : 7)
      for (uint64_t d = 0; d < 64; d += (d < 3 || d > 60) ? 1 : 5) {
        if (one(s, d, c)) return 1;
        ++ran;
      }
  for (uint64_t i = 0; i < cases; ++i) {
    const uint64_t c = rnd() % 8 == 0 ? rnd() % 5000 : rnd() % 200;
    if (one(rnd() % 64, rnd() % 64, c)) return 1;
    ++ran;
  }
  // runs that start far into a bitmap (word index > 0 on both sides)
  for (uint64_t i = 0; i < 200; ++i) {
    const uint64_t sb = rnd() % 1000, db = rnd() % 1000, c = rnd() % 300;
    std::vector<uint64_t> src((sb + c + 63) / 64 + 1), dst((db + c + 63) / 64 + 1);
    for (uint64_t& w : src) w = rnd();
    for (uint64_t& w : dst) w = rnd();
    const std::vector<uint64_t> before = dst;
    cir::copy_bits(dst.data(), db, src.data(), sb, c);
    for (uint64_t k = 0; k < dst.size() * 64; ++k) {
      const bool in = k >= db && k < db + c;
      if (bit(dst, k) != (in ? bit(src, sb + (k - db)) : bit(before, k))) {
        fprintf(stderr, "copy_bits(sbit %llu, dbit %llu, count %llu): bit %llu\n",
                (unsigned long long)sb, (unsigned long long)db, (unsigned long long)c,
                (unsigned long long)k);
        return 1;
      }
    }
    ++ran;
  }
  printf("bits_fuzz: %llu cases ok\n", (unsigned long long)ran);
  return 0;
}
