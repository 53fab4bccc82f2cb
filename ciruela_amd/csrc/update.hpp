// The rule behind cir_update_blocks, written once for the host and the device:
// which blocks of a new image stay where they are, which are copied inside
// device memory and which of those go through a staging scratch, when the
// destinations may be the resident buffers themselves.  Built on copyblk.hpp
// (the copy of runs, take_of); no HIP runtime call; compiled by update.hip (the
// kernels), update.cpp (the call) and, alone under the sanitizers, by
// tools/update_fuzz.cpp.  The reference has no counterpart: it holds no image
// in device memory.
//
// Inputs: copyblk::Plan's, the digests of the resident blocks (pool_dig, 32
// bytes per ordinal), the digests of the new index (need_dig, 32 bytes per
// global block), the cap of the scratch in units of 16 bytes (cap_units) and
// the scratch's address.
//
// The resident table {first_block, address, size} is sorted by address, so
// first_block and address both ascend, and its buffers do not overlap one
// another: the call writes into them.  One bisection by address finds the
// buffer that holds a byte.
//
// The classes.  Every global block g of the new index whose file has a
// destination gets exactly one; dst = dests[file] + j bs, len = min(bs, size -
// j bs).
//   KEPT     dst lies in a resident buffer, (dst - that buffer's address) is a
//            multiple of bs, that resident block's length is len and its digest
//            in pool_dig equals g's in need_dig.  Nothing is read or written;
//            the bit is set.  This test comes first, before the join's answer
//            is looked at: a file full of equal blocks is kept, not moved onto
//            itself from the join's smallest ordinal.
//   otherwise copyblk::take_of decides as in cir_reload_blocks (a match, a
//   destination, equal lengths; a match that fails only the length test is
//   dropped and counted), and a taken block is
//   DIRECT   when [dst, dst + len) overlaps no resident buffer: copied from
//            source to destination in phase 1;
//   STAGED   otherwise: a candidate for the scratch.
// The scratch cap.  STAGED candidates are numbered in block order; a
// candidate's scratch position is 16 x the exclusive prefix of the units
// (scatter::units(len)) of all earlier STAGED candidates, staged or not.  It is
// staged when prefix + units <= cap_units and DEMOTED otherwise: not taken, bit
// 0, counted, read from disk like any missing block.  prefix + units is the
// inclusive prefix, which never descends, so the cut is a prefix in block
// order: a later, smaller candidate that would still fit is demoted too, and
// the answer does not depend on timing.
//
// The two tables, both copyblk tables in block order {unit_first, src, dst,
// bytes}:
//   A, phase 1: every DIRECT block src -> dst, every staged block src ->
//               scratch + pos;
//   B, phase 2: every staged block scratch + pos -> dst.
// Each meets copyblk.hpp's precondition that the sources and destinations of
// one table do not overlap.  Table A reads resident buffers only (a source is a
// resident block) and writes only to the scratch and to memory that no resident
// buffer covers (the definition of DIRECT).  Table B reads only the scratch and
// writes only outside it.  The scratch is the call's own allocation.  Inside a
// table the destinations of distinct blocks are disjoint because the
// destinations of distinct file entries are (the call refuses others) and the
// scratch positions are an exclusive prefix.
//
// The rule rests on stream order, not on an order of the copies: the resident
// hash, the join and the plan read the buffers, phase 1 reads them for the last
// time, phase 2 and the disk pipeline's scatter write afterwards.  Swaps,
// cycles and shifts by a block need nothing more.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "copyblk.hpp"

namespace cir {
namespace update {

constexpr uint32_t kNone = 0, kKept = 1, kDirect = 2, kStaged = 3;  // a block's candidate class
constexpr uint64_t kNoCap = ~0ull;
// res of the plan {table A's records, A's units, table B's records (the staged
// blocks), B's units (the scratch's), kept blocks, kept bytes, direct blocks,
// direct bytes, staged bytes, demoted blocks, demoted bytes, dropped matches,
// and the candidates' totals: A records, A units, STAGED records, STAGED units}
constexpr int kResFields = 16;
enum Res {
  kARecs, kAUnits, kBRecs, kBUnits, kKeptBlocks, kKeptBytes, kDirectBlocks, kDirectBytes,
  kStagedBytes, kDemotedBlocks, kDemotedBytes, kDroppedMatches, kCandARecs, kCandAUnits,
  kCandSRecs, kCandSUnits
};

struct Plan {
  copyblk::Plan c;          // c.have sorted by address, its buffers disjoint
  const uint8_t* pool_dig;  // 32 c.n_pool bytes
  const uint8_t* need_dig;  // 32 c.n_need bytes
  uint64_t cap_units;       // kNoCap: whatever the staged blocks need
  uint64_t scratch;         // the scratch's address (k_update_emit, plan_host)
};

// Block g's candidate class and, unless kNone, its len bytes at dst; src for
// kDirect and kStaged.
struct Cand {
  uint64_t src, dst;
  uint32_t len, cls;
  bool dropped;
};

// 32 bytes against 32 bytes: two 16-byte loads per operand, as k_first_bad.
CIR_SCAT_HD inline bool digest_eq(const uint8_t* a, const uint8_t* b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4* p = reinterpret_cast<const u32x4*>(a);
  const u32x4* q = reinterpret_cast<const u32x4*>(b);
  const u32x4 x = p[0] ^ q[0], y = p[1] ^ q[1];
  return ((x.x | x.y | x.z | x.w) | (y.x | y.y | y.z | y.w)) == 0;
#else
  return memcmp(a, b, 32) == 0;
#endif
}

// The resident buffer that holds the byte at address `at`; ~0 when none does.
CIR_SCAT_HD inline uint64_t buffer_at(const copyblk::Plan& c, uint64_t at) {
  // (the table's second word is the address: it ascends like the first)
  const uint64_t h = copyblk::rec_at(c.have + 1, c.nhave, copyblk::kHaveWords, at);
  if (h == ~0ull) return h;
  const uint64_t* f = c.have + copyblk::kHaveWords * h;
  return at - f[1] < f[2] ? h : ~0ull;
}

CIR_SCAT_HD inline Cand classify(const Plan& p, uint64_t g) {
  Cand k{0, 0, 0, kNone, false};
  const copyblk::Plan& c = p.c;
  if (g >= c.n_need) return k;
  const uint64_t r = copyblk::rec_at(c.need_runs, c.n_need_runs, copyblk::kNeedRunWords, g);
  if (r == ~0ull) return k;
  const uint64_t* q = c.need_runs + copyblk::kNeedRunWords * r;
  const uint64_t j = g - q[0], file = q[2];
  const uint64_t len = copyblk::block_len(q[1], c.bs, j);
  if (!len || file >= c.ndests || !c.dests[file]) return k;
  const uint64_t dst = c.dests[file] + j * c.bs;
  k.dst = dst;
  k.len = (uint32_t)len;
  // kept?
  const uint64_t h = buffer_at(c, dst);
  if (h != ~0ull) {
    const uint64_t* f = c.have + copyblk::kHaveWords * h;
    const uint64_t off = dst - f[1];
    if (off % c.bs == 0 && copyblk::block_len(f[2], c.bs, off / c.bs) == len &&
        digest_eq(p.pool_dig + 32 * (f[0] + off / c.bs), p.need_dig + 32 * g)) {
      k.cls = kKept;
      return k;
    }
  }
  const copyblk::Take t = copyblk::take_of(c, g);
  k.dropped = t.flags & copyblk::kDropped;
  if (!(t.flags & copyblk::kTaken)) return k;
  k.src = t.src;
  // does [dst, dst + len) meet a resident buffer?  The last buffer that begins
  // at or below the block's last byte reaches furthest of those that could.
  const uint64_t e = copyblk::rec_at(c.have + 1, c.nhave, copyblk::kHaveWords, dst + len - 1);
  bool over = false;
  if (e != ~0ull) {
    const uint64_t* f = c.have + copyblk::kHaveWords * e;
    over = f[1] + f[2] > dst;
  }
  k.cls = over ? kStaged : kDirect;
  return k;
}

// Is a STAGED candidate whose earlier candidates have `prefix` units staged?
CIR_SCAT_HD inline bool fits(uint64_t prefix, uint64_t units, uint64_t cap_units) {
  return prefix <= cap_units && units <= cap_units - prefix;
}

}  // namespace update
}  // namespace cir

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <utility>
#include <vector>

namespace cir {
namespace update {

// Do any two of the intervals [lo, hi) overlap?  (Empty ones overlap nothing.)
inline bool spans_overlap(std::vector<std::pair<uint64_t, uint64_t>> v) {
  std::sort(v.begin(), v.end());
  uint64_t end = 0;
  for (const auto& s : v) {
    if (s.first >= s.second) continue;
    if (s.first < end) return true;
    end = std::max(end, s.second);
  }
  return false;
}

// The host executor, block by block in order as k_update_plan, k_update_scan
// and k_update_emit leave it: the have bitmap (ceil(n_need / 64) words, every
// one written; KEPT, DIRECT and staged blocks), table A and table B (room for
// n_need records each) and res[kResFields].
inline void plan_host(const Plan& p, uint64_t* have_bits, uint64_t* runs_a, uint64_t* runs_b,
                      uint64_t* res) {
  const uint64_t n = p.c.n_need;
  for (uint64_t w = 0; w < (n + 63) / 64; ++w) have_bits[w] = 0;
  for (int i = 0; i < kResFields; ++i) res[i] = 0;
  uint64_t s_prefix = 0;  // the units of the STAGED candidates so far
  for (uint64_t g = 0; g < n; ++g) {
    const Cand k = classify(p, g);
    if (k.dropped) ++res[kDroppedMatches];
    if (k.cls == kNone) continue;
    const uint64_t units = scatter::units(k.len);
    bool have = true;
    if (k.cls == kKept) {
      ++res[kKeptBlocks];
      res[kKeptBytes] += k.len;
    } else {
      ++res[kCandARecs];
      res[kCandAUnits] += units;
      uint64_t to = k.dst;
      if (k.cls == kStaged) {
        const uint64_t pos = s_prefix;
        ++res[kCandSRecs];
        res[kCandSUnits] += units;
        s_prefix += units;
        have = fits(pos, units, p.cap_units);
        if (have) {
          to = p.scratch + 16 * pos;
          uint64_t* q = runs_b + copyblk::kRunWords * res[kBRecs]++;
          q[0] = res[kBUnits];
          q[1] = to;
          q[2] = k.dst;
          q[3] = k.len;
          res[kBUnits] += units;
          res[kStagedBytes] += k.len;
        } else {
          ++res[kDemotedBlocks];
          res[kDemotedBytes] += k.len;
        }
      } else {
        ++res[kDirectBlocks];
        res[kDirectBytes] += k.len;
      }
      if (have) {
        uint64_t* q = runs_a + copyblk::kRunWords * res[kARecs]++;
        q[0] = res[kAUnits];
        q[1] = k.src;
        q[2] = to;
        q[3] = k.len;
        res[kAUnits] += units;
      }
    }
    if (have) have_bits[g >> 6] |= 1ull << (g & 63);
  }
}

}  // namespace update
}  // namespace cir
#endif
