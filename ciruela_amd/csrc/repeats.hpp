// The rule of cir_block_repeats / cir_match_repeats_dev, written once: which
// blocks of one index carry a digest that an earlier or already present block
// of the same index carries, so that they are copied inside the image instead
// of fetched.  Header-only and free of HIP (the way extents.hpp and
// sources.hpp hold theirs): the kernels (repeats.hip), the host path
// (repeats.cpp) and the fuzz (tools/repeats_fuzz.cpp) all use this text.
//
// Blocks g < n are the index's file-entry blocks in index order, blocks
// ascending (the global numbering of cir_check_blocks).  Two optional bitmaps,
// bit g & 63 of word g >> 6, ceil(n / 64) words, bits at and past n ignored:
//   wanted   want == NULL, or want's bit g is set: still to be obtained;
//   present  not wanted, present != NULL and present's bit g is set: in the
//            new directory, or there before any copy below is made;
//   a block that is neither takes no part: never a source, never a destination.
// A bit set in both bitmaps means wanted.
//
// Every block that takes part has a key: g when present, 2^31 + g when wanted.
// The leader of a digest is the participating block with the smallest key
// among those that have that digest over all 32 bytes: a present holder beats
// any wanted one, and among equals the first in index order wins (the flavour
// of scan_links' break, src/daemon/metadata/hardlink_sources.rs:143).  A
// wanted block g whose digest's leader is L != g is a repeat: it is copied
// from block L of the same image.  A wanted block that is its own leader is
// fetched.
//
// match[g] = kNone when g is not wanted or is its own leader, else the leader
// as an ordinal of a pool of 2n: L when the leader is present, n + L when it
// is a wanted block.  With the need run table twice as the pool's (the first
// copy with x = 0; the second with every `first` raised by n and x = 1; n_pool
// = 2n) extents.hpp's unchanged rule gives the rest: the length check (unequal
// lengths: dropped, stays in the fetch bitmap, no second candidate), the
// extents (src = 0: a present source, 1: a fetched one; src_file a file
// ordinal of the same index) and the fetch bitmap.  A leader is never a repeat,
// so no block is both a source and a destination.
//
// n <= kMaxBlocks = 2^30 - 1 keeps 2n within the extent rule's 2^31 - 1 and
// 2^31 + g clear of kNone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CIR_REP_HD __host__ __device__ inline
#else
#define CIR_REP_HD inline
#endif

namespace cir {
namespace repeats {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kWantedBit = 0x80000000u;
constexpr uint64_t kMaxBlocks = 0x3FFFFFFFull;

CIR_REP_HD bool bit(const uint64_t* map, uint64_t g) { return map[g >> 6] >> (g & 63) & 1; }

// Block g's key, or kNone when it takes no part (g < n <= kMaxBlocks).
CIR_REP_HD uint32_t key_of(const uint64_t* want, const uint64_t* present, uint64_t g) {
  if (!want || bit(want, g)) return kWantedBit | (uint32_t)g;
  if (present && bit(present, g)) return (uint32_t)g;
  return kNone;
}
CIR_REP_HD bool key_wanted(uint32_t key) { return key != kNone && (key & kWantedBit); }
CIR_REP_HD uint32_t key_block(uint32_t key) { return key & ~kWantedBit; }

// match[] of the block with key `mine` whose digest's leader has key `leader`.
CIR_REP_HD uint32_t match_of(uint32_t mine, uint32_t leader, uint64_t n) {
  if (!key_wanted(mine) || leader == mine || leader == kNone) return kNone;
  return (leader & kWantedBit) ? (uint32_t)n + key_block(leader) : leader;
}

}  // namespace repeats
}  // namespace cir

#if !defined(__HIPCC__)
// The host side: the join with a hash map in which the smaller key wins, and
// the doubled run table.
#include "sources.hpp"

namespace cir {
namespace repeats {

struct Counts {
  uint64_t wanted = 0, present = 0, repeats = 0;
};

// How many blocks take part, by class.
inline Counts count_classes(const uint64_t* want, const uint64_t* present, uint64_t n) {
  Counts c;
  for (uint64_t g = 0; g < n; ++g) {
    const uint32_t k = key_of(want, present, g);
    if (k == kNone) continue;
    if (k & kWantedBit)
      ++c.wanted;
    else
      ++c.present;
  }
  return c;
}

// match[0 .. n) by the rule above, from n digests of 32 bytes.
inline Counts host_match(const uint8_t* digests, uint64_t n, const uint64_t* want,
                         const uint64_t* present, uint32_t* match,
                         uint64_t seed = 0x243F6A8885A308D3ull) {
  std::unordered_map<sources::Key32, uint32_t, sources::Key32Hash> map(16,
                                                                      sources::Key32Hash{seed});
  map.reserve((size_t)n);
  sources::Key32 k;
  Counts c;
  for (uint64_t g = 0; g < n; ++g) {
    const uint32_t key = key_of(want, present, g);
    if (key == kNone) continue;
    if (key & kWantedBit)
      ++c.wanted;
    else
      ++c.present;
    memcpy(k.b, digests + 32 * g, 32);
    const auto ins = map.emplace(k, key);
    if (!ins.second && key < ins.first->second) ins.first->second = key;  // the smaller key wins
  }
  for (uint64_t g = 0; g < n; ++g) {
    const uint32_t key = key_of(want, present, g);
    match[g] = kNone;
    if (!key_wanted(key)) continue;
    memcpy(k.b, digests + 32 * g, 32);
    match[g] = match_of(key, map.find(k)->second, n);
    if (match[g] != kNone) ++c.repeats;
  }
  return c;
}

// The pool run table of the rule: need's runs twice, the second copy's `first`
// raised by need.n and its src 1.
inline sources::BlockList doubled(const sources::BlockList& need) {
  sources::BlockList pool;
  pool.runs.reserve(2 * need.runs.size());
  for (uint32_t x = 0; x < 2; ++x)
    for (const sources::FileRun& r : need.runs)
      pool.runs.push_back(sources::FileRun{r.first + x * need.n, r.size, r.file, x});
  pool.n = 2 * need.n;
  return pool;
}

}  // namespace repeats
}  // namespace cir
#endif
