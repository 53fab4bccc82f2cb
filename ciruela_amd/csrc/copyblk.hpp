// The two rules behind cir_reload_blocks, written once for the host and the
// device: the copy of runs of bytes between buffers of any alignment
// (cir_copy_runs, cir_copy_runs_dev) and the decision which blocks of a new
// image are taken from buffers that are resident in device memory (k_copy_plan).
// No HIP runtime call; compiled by copyblk.hip (the kernels), reload.cpp (the
// host forms) and, alone under the sanitizers, by tools/copyblk_fuzz.cpp.  The
// reference has no counterpart: it holds no image in device memory.
//
// The copy.  Table: one record of kRunWords u64 per run {unit_first, src, dst,
// bytes}: `bytes` (> 0) bytes at the address `src` go to the address `dst`,
// both of any alignment.  A record has units(bytes) units of 16 bytes, the last
// one maybe shorter; unit_first is the unit count of all earlier records and
// nunits that of the table, as in scatter.hpp and gather.hpp, whose units(),
// run_at() and lanes() this rule uses.
//
// Unit u belongs to the record found by bisection on unit_first; with k = u -
// unit_first it is the bytes [16 k, 16 k + n), n = min(16, bytes - 16 k), of
// the source and of the destination alike.  A unit reads only its own n source
// bytes and stores only its own n destination bytes, so no two units store to
// one byte as long as the records' destinations do not overlap.  Sources and
// destinations of one table must not overlap either: a unit may read a byte
// that another unit has or has not yet written.
//
// Untrusted tables: record r is bad when its bytes is 0 or its unit_first is
// not that of record r - 1 plus r - 1's units (0 for r = 0; the last record must
// also end at nunits).  A bad record is read nowhere and written nowhere, and
// it is counted once, by unit r, exactly as in scatter.hpp; a unit past its
// record's units copies nothing.
//
// The plan.  For every global block g of the new index: is it taken from
// memory, and from where?  match[g] is the join's answer (the smallest ordinal
// of a resident block with g's digest, or kNoMatch); the need runs are
// cir_index_digests_dev's, one per non-empty file {first, size, file, x}; dests
// holds one address per file entry (0: no destination); the resident table has
// one record per resident buffer {first_block, address, size}, first_block
// ascending, each buffer cut into blocks of bs bytes from its offset 0.  Block g
// is taken when it has a match, its file has a destination and the two blocks'
// lengths agree (min(bs, size - j bs) on either side: cir_block_sources' length
// rule); a match that fails only the length test is counted as dropped.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scatter.hpp"

namespace cir {
namespace copyblk {

constexpr int kRunWords = scatter::kRunWords;  // {unit_first, src, dst, bytes}
constexpr uint64_t kMaxRuns = scatter::kMaxRuns;
constexpr uint64_t kMaxUnits = 1ull << 60;  // (the kernel strides: no grid bounds the units)

// Is record r (< nruns) one that nothing may be read or written through?
CIR_SCAT_HD inline bool run_bad(const uint64_t* runs, uint64_t nruns, uint64_t nunits, uint64_t r) {
  const uint64_t* q = runs + kRunWords * r;
  const uint64_t first = q[0], bytes = q[3];
  if (bytes == 0) return true;
  const uint64_t want = r ? q[-kRunWords] + scatter::units(q[-kRunWords + 3]) : 0;
  if (first != want) return true;
  return r + 1 == nruns && first + scatter::units(bytes) != nunits;
}

// What unit u copies: n bytes (0: nothing) from the address src to the address dst.
struct Unit {
  uint64_t src, dst;
  uint32_t n;
};

CIR_SCAT_HD inline Unit unit_of(const uint64_t* runs, uint64_t nruns, uint64_t nunits, uint64_t u) {
  Unit w{0, 0, 0};
  if (u >= nunits) return w;
  const uint64_t r = scatter::run_at(runs, nruns, u);
  if (r == scatter::kNoRun || run_bad(runs, nruns, nunits, r)) return w;
  const uint64_t* q = runs + kRunWords * r;
  const uint64_t k = u - q[0];
  if (k >= scatter::units(q[3])) return w;
  const uint64_t left = q[3] - 16 * k;
  w.src = q[1] + 16 * k;
  w.dst = q[2] + 16 * k;
  w.n = (uint32_t)(left < 16 ? left : 16);
  return w;
}

// ---- the plan ---------------------------------------------------------------

constexpr int kNeedRunWords = 4;  // {first, size, file, x}: idxscan::Run
constexpr int kHaveWords = 3;     // {first_block, address, size}
constexpr uint32_t kNoMatch = 0xFFFFFFFFu;
constexpr uint32_t kTaken = 1, kDropped = 2;
// res of the plan: {records, units, bytes, dropped}
constexpr int kPlanResFields = 4;

struct Plan {
  const uint32_t* match;  // n_need entries
  uint64_t n_need;
  const uint64_t* need_runs;  // first ascending
  uint64_t n_need_runs;
  const uint64_t* dests;  // one address per file entry, 0: none
  uint64_t ndests;
  const uint64_t* have;  // first_block ascending
  uint64_t nhave;
  uint64_t n_pool;  // resident blocks in all
  uint64_t bs;
};

// Block g's copy: flags (kTaken, kDropped or 0) and, when taken, len bytes
// from src to dst.
struct Take {
  uint64_t src, dst;
  uint32_t len, flags;
};

// The last record (of `words` u64 each) whose first word is at or below v; ~0 when none.
CIR_SCAT_HD inline uint64_t rec_at(const uint64_t* tab, uint64_t n, int words, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (tab[(uint64_t)words * mid] <= v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : ~0ull;
}

// Block j of `size` bytes cut into blocks of bs: its length, 0 when there is no such block.
CIR_SCAT_HD inline uint64_t block_len(uint64_t size, uint64_t bs, uint64_t j) {
  if (j >= size / bs + (size % bs != 0)) return 0;
  const uint64_t rest = size - j * bs;
  return rest < bs ? rest : bs;
}

CIR_SCAT_HD inline Take take_of(const Plan& p, uint64_t g) {
  Take t{0, 0, 0, 0};
  if (g >= p.n_need) return t;
  const uint32_t m = p.match[g];
  if (m == kNoMatch || m >= p.n_pool) return t;
  const uint64_t r = rec_at(p.need_runs, p.n_need_runs, kNeedRunWords, g);
  if (r == ~0ull) return t;
  const uint64_t* q = p.need_runs + kNeedRunWords * r;
  const uint64_t j = g - q[0], file = q[2];
  const uint64_t need_len = block_len(q[1], p.bs, j);
  if (!need_len || file >= p.ndests || !p.dests[file]) return t;
  const uint64_t h = rec_at(p.have, p.nhave, kHaveWords, m);
  if (h == ~0ull) return t;
  const uint64_t* f = p.have + kHaveWords * h;
  const uint64_t pj = m - f[0];
  const uint64_t have_len = block_len(f[2], p.bs, pj);
  if (!have_len) return t;
  if (have_len != need_len) {
    t.flags = kDropped;
    return t;
  }
  t.src = f[1] + pj * p.bs;
  t.dst = p.dests[file] + j * p.bs;
  t.len = (uint32_t)need_len;
  t.flags = kTaken;
  return t;
}

}  // namespace copyblk
}  // namespace cir

#if !defined(__HIP_DEVICE_COMPILE__)
namespace cir {
namespace copyblk {

// The copy's host executor: every unit in turn, as the kernel's lanes would;
// returns the count of bad records.
inline uint64_t apply_host(const uint64_t* runs, uint64_t nruns, uint64_t nunits) {
  uint64_t bad = 0;
  const uint64_t n = scatter::lanes(nruns, nunits);
  for (uint64_t u = 0; u < n; ++u) {
    if (u < nruns && run_bad(runs, nruns, nunits, u)) ++bad;
    const Unit w = unit_of(runs, nruns, nunits, u);
    if (w.n)
      memcpy(reinterpret_cast<void*>((uintptr_t)w.dst), reinterpret_cast<const void*>((uintptr_t)w.src),
             w.n);
  }
  return bad;
}

// The plan's host executor, block by block in order as the kernels' count,
// scan and emit leave it: the have bitmap (ceil(n_need / 64) words, every one
// written), the records of the taken blocks in block order (room for n_need)
// and res[kPlanResFields].
inline void plan_host(const Plan& p, uint64_t* have_bits, uint64_t* runs, uint64_t* res) {
  for (uint64_t w = 0; w < (p.n_need + 63) / 64; ++w) have_bits[w] = 0;
  uint64_t nrec = 0, nunits = 0, bytes = 0, dropped = 0;
  for (uint64_t g = 0; g < p.n_need; ++g) {
    const Take t = take_of(p, g);
    if (t.flags & kDropped) ++dropped;
    if (!(t.flags & kTaken)) continue;
    have_bits[g >> 6] |= 1ull << (g & 63);
    uint64_t* q = runs + kRunWords * nrec++;
    q[0] = nunits;
    q[1] = t.src;
    q[2] = t.dst;
    q[3] = t.len;
    nunits += scatter::units(t.len);
    bytes += t.len;
  }
  res[0] = nrec;
  res[1] = nunits;
  res[2] = bytes;
  res[3] = dropped;
}

}  // namespace copyblk
}  // namespace cir
#endif
