// The rule of cir_block_extents / cir_match_extents_dev, written once: where a
// needed block's local copy sits, and whether two neighbouring blocks' copies
// continue one another.  Free of HIP and of the standard library, compiled by
// host and device code alike (the way idxscan.hpp holds the parser's rule):
// the kernels (extents.hip), the host path (sources.hpp extents_of) and the
// fuzz (tools/extents_fuzz.cpp) all use this text.
//
// Inputs: match[g] for g < n_need as the join leaves it (a pool ordinal, or
// anything >= n_pool for "none"); a need run table and a pool run table of
// four u64 per non-empty file {first, size, file, x}, `first` ascending; in
// the need table x is ignored (cir_index_digests_dev's table fits as it is),
// in the pool table `first` is a pool ordinal across all sources and x the
// source ordinal (its low 32 bits: sources::FileRun is this record); n_pool,
// the block size, and an optional `want` bitmap.
//
// Per block g (sources::map_matches' rule): its need run is the last one with
// first <= g; if there is none, or g - first >= ceil(size / bs), the block
// lies in no file: not wanted, not found.  Otherwise it is wanted iff its
// `want` bit is set (or want is null).  A wanted block with match[g] = j <
// n_pool whose pool run covers j is found iff the two blocks' lengths min(bs,
// size - b bs) are equal; unequal lengths count as dropped and no second
// candidate is looked for.
//
// cont(g), g >= 1: g - 1 and g are both found, lie in the same need run, have
// the same src and src_file, and src_block(g) == src_block(g - 1) + 1.  An
// extent is a maximal stretch of blocks joined by cont.
//
// Whatever the tables and match hold, nothing outside need[0 .. 4 n_need_runs),
// pool[0 .. 4 n_pool_runs), match[0 .. n_need) and want[0 .. ceil(n_need / 64))
// is read; every loop is bounded by a table's length.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CIR_EXT_HD __host__ __device__ inline
#else
#define CIR_EXT_HD inline
#endif

namespace cir {
namespace extents {

constexpr uint32_t kNoSrc = 0xFFFFFFFFu;
constexpr uint64_t kNone64 = ~0ull;
constexpr int kRecWords = 8;  // {first, count, need_file, need_block, src, src_file, src_block, bytes}
constexpr int kResFields = 6;  // {status, wanted, found, bytes, dropped, extents}
constexpr uint64_t kOk = 0, kCapacity = 1;

struct Tables {
  const uint32_t* match;
  uint64_t n_need;
  const uint64_t* need;  // 4 u64 per run
  uint64_t n_need_runs;
  const uint64_t* pool;
  uint64_t n_pool_runs;
  uint64_t n_pool;
  uint64_t bs;
  const uint64_t* want;  // or null: every block
};

constexpr uint32_t kWanted = 1, kFound = 2, kDropped = 4;

// What the rule says of one block.  run / need_*: meaningful when the block
// lies in a file (need_end: the byte offset in its file at which the block
// ends); src / file / block / len: when it is found (kNoSrc / kNone64 / 0
// otherwise, the per-block arrays' "not found").
struct Map {
  uint32_t flags;
  uint32_t src;
  uint64_t run;
  uint64_t need_file, need_block, need_end;
  uint64_t file, block, len;
};

CIR_EXT_HD uint64_t blocks_of(uint64_t size, uint64_t bs) { return size / bs + (size % bs != 0); }

// min(bs, size - b bs), for b < blocks_of(size, bs) (so b bs < size).
CIR_EXT_HD uint64_t block_len(uint64_t size, uint64_t bs, uint64_t b) {
  const uint64_t off = b * bs;
  return size - off < bs ? size - off : bs;
}

// The last run with first <= j, if any.  At most 64 steps whatever the table
// holds: hi - lo halves.
CIR_EXT_HD bool find_run(const uint64_t* runs, uint64_t n, uint64_t j, uint64_t* at) {
  if (n == 0) return false;
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (runs[4 * mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  if (runs[4 * lo] > j) return false;
  *at = lo;
  return true;
}

CIR_EXT_HD Map map_block(const Tables& t, uint64_t g) {
  Map m;
  m.flags = 0;
  m.src = kNoSrc;
  m.run = kNone64;
  m.need_file = m.need_block = m.need_end = 0;
  m.file = m.block = kNone64;
  m.len = 0;
  uint64_t r;
  if (g >= t.n_need || !find_run(t.need, t.n_need_runs, g, &r)) return m;
  const uint64_t first = t.need[4 * r], size = t.need[4 * r + 1];
  const uint64_t b = g - first;
  if (b >= blocks_of(size, t.bs)) return m;
  const uint64_t mine = block_len(size, t.bs, b);
  m.run = r;
  m.need_file = t.need[4 * r + 2];
  m.need_block = b;
  m.need_end = b * t.bs + mine;
  if (t.want && !(t.want[g >> 6] >> (g & 63) & 1)) return m;
  m.flags = kWanted;
  const uint64_t j = t.match[g];
  uint64_t p;
  if (j >= t.n_pool || !find_run(t.pool, t.n_pool_runs, j, &p)) return m;
  const uint64_t psize = t.pool[4 * p + 1];
  const uint64_t pb = j - t.pool[4 * p];
  if (pb >= blocks_of(psize, t.bs)) return m;
  if (block_len(psize, t.bs, pb) != mine) {
    m.flags |= kDropped;  // the source index lies, or a digest collided
    return m;
  }
  m.flags |= kFound;
  m.src = (uint32_t)t.pool[4 * p + 3];
  m.file = t.pool[4 * p + 2];
  m.block = pb;
  m.len = mine;
  return m;
}

// Does block g continue the extent of block g - 1?  (a = g - 1's, b = g's.)
CIR_EXT_HD bool cont(uint32_t a_flags, uint64_t a_run, uint32_t a_src, uint64_t a_file,
                     uint64_t a_block, uint32_t b_flags, uint64_t b_run, uint32_t b_src,
                     uint64_t b_file, uint64_t b_block) {
  return (a_flags & b_flags & kFound) && a_run == b_run && a_src == b_src && a_file == b_file &&
         b_block == a_block + 1;
}
CIR_EXT_HD bool cont(const Map& a, const Map& b) {
  return cont(a.flags, a.run, a.src, a.file, a.block, b.flags, b.run, b.src, b.file, b.block);
}

// An extent's bytes from its head's block number inside the need file and the
// offset at which its tail block ends: min(size, (need_block + count) bs) -
// need_block bs.
CIR_EXT_HD uint64_t extent_bytes(uint64_t head_need_block, uint64_t tail_need_end, uint64_t bs) {
  return tail_need_end - head_need_block * bs;
}

}  // namespace extents
}  // namespace cir
