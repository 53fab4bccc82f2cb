// The rule of the scatter behind cir_load_blocks (cir_scatter_runs,
// cir_scatter_runs_dev), written once for the host and the device: the packed
// runs of a staging slot copied to their places in the caller's buffers.  No
// HIP runtime call; compiled by scatter.hip (the kernel), check.cpp (the table
// and the host form) and, alone under the sanitizers, by tools/scatter_fuzz.cpp.
// The reference has no counterpart: its consumers read committed files from
// disk (commit_image, src/daemon/disk/commit.rs:51-117, is the last look at
// the bytes).
//
// Table: one record of kRunWords u64 per packed run {unit_first, src_pos, dst,
// bytes}: `bytes` (> 0) bytes at byte `src_pos` of the source (a multiple of
// 16, as pack_run lays runs out) go to the address `dst` (any alignment).  A
// record has units(bytes) = ceil(bytes / 16) units of 16 bytes, the last one
// maybe shorter; unit_first is the unit count of all earlier records, so the
// units of a table are numbered 0 .. nunits - 1 and nunits is the last record's
// unit_first + units.
//
// Unit u belongs to the record found by bisection on unit_first (run_at, at
// most 32 steps: nruns <= kMaxRuns); with k = u - unit_first it is the source
// bytes [src_pos + 16 k, src_pos + 16 k + n), n = min(16, bytes - 16 k), and
// goes to dst + 16 k.  A unit stores only its own n bytes, so two units never
// store to the same byte as long as the records' destinations do not overlap.
//
// Untrusted tables: record r is bad when its src_pos is not a multiple of 16,
// its bytes is 0, its source range does not lie inside [0, src_bytes), or its
// unit_first is not that of record r - 1 plus r - 1's units (0 for r = 0; the
// last record must also end at nunits).  A bad record is written nowhere and
// read nowhere -- every unit looks at its own record before it touches
// anything -- and it is counted once: unit r looks at record r (a table has at
// least as many units as records), so the count does not depend on what
// unit_first holds.  A unit past its record's units (a gap that a wrong
// unit_first leaves) copies nothing.  Each record is checked against its
// predecessor as it stands: one wrong unit_first in the middle of a table
// makes that record and the one behind it bad.  The count is exact whatever
// the table holds; that every sound record is written whole needs a
// unit_first that does not descend (the bisection's premise).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CIR_SCAT_HD __host__ __device__
#else
#define CIR_SCAT_HD
#endif

namespace cir {
namespace scatter {

constexpr int kRunWords = 4;                  // {unit_first, src_pos, dst, bytes}
constexpr uint64_t kUnitBytes = 16;           // bytes per unit, one lane of k_scatter_runs
constexpr uint64_t kMaxRuns = 0xFFFFFFFFull;  // the bisection's 32 steps
constexpr uint64_t kMaxUnits = 0xFFFFFFFFull;
constexpr uint64_t kNoRun = ~0ull;

CIR_SCAT_HD inline uint64_t units(uint64_t bytes) { return bytes / 16 + (bytes % 16 != 0); }

// The last record whose unit_first is at or below u; kNoRun when there is none.
CIR_SCAT_HD inline uint64_t run_at(const uint64_t* runs, uint64_t nruns, uint64_t u) {
  uint64_t lo = 0, hi = nruns;  // runs[< lo].unit_first <= u < runs[>= hi].unit_first
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (runs[kRunWords * mid] <= u)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : kNoRun;
}

// Is record r (< nruns) one that nothing may be read or written through?
CIR_SCAT_HD inline bool run_bad(const uint64_t* runs, uint64_t nruns, uint64_t nunits,
                                uint64_t src_bytes, uint64_t r) {
  const uint64_t* q = runs + kRunWords * r;
  const uint64_t first = q[0], pos = q[1], bytes = q[3];
  if ((pos & 15) || bytes == 0 || bytes > src_bytes || pos > src_bytes - bytes) return true;
  const uint64_t want = r ? q[-kRunWords] + units(q[-kRunWords + 3]) : 0;
  if (first != want) return true;
  return r + 1 == nruns && first + units(bytes) != nunits;
}

// What unit u copies: n bytes (0: nothing) from byte src_off of the source to
// the address dst.
struct Unit {
  uint64_t src_off, dst;
  uint32_t n;
};

CIR_SCAT_HD inline Unit unit_of(const uint64_t* runs, uint64_t nruns, uint64_t nunits,
                                uint64_t src_bytes, uint64_t u) {
  Unit w{0, 0, 0};
  if (u >= nunits) return w;
  const uint64_t r = run_at(runs, nruns, u);
  if (r == kNoRun || run_bad(runs, nruns, nunits, src_bytes, r)) return w;
  const uint64_t* q = runs + kRunWords * r;
  const uint64_t k = u - q[0];
  if (k >= units(q[3])) return w;
  const uint64_t left = q[3] - 16 * k;
  w.src_off = q[1] + 16 * k;
  w.dst = q[2] + 16 * k;
  w.n = (uint32_t)(left < 16 ? left : 16);
  return w;
}

// Lanes (and host steps) a table takes: one per unit, and one per record for
// its look at the record.
CIR_SCAT_HD inline uint64_t lanes(uint64_t nruns, uint64_t nunits) {
  return nunits > nruns ? nunits : nruns;
}

}  // namespace scatter
}  // namespace cir

#if !defined(__HIP_DEVICE_COMPILE__)
#include <string.h>

#include "pack.hpp"

namespace cir {
namespace scatter {

// The host executor: every unit in turn, as the kernel's lanes would; returns
// the count of bad records.
inline uint64_t apply_host(const uint8_t* src, uint64_t src_bytes, const uint64_t* runs,
                           uint64_t nruns, uint64_t nunits) {
  uint64_t bad = 0;
  const uint64_t n = lanes(nruns, nunits);
  for (uint64_t u = 0; u < n; ++u) {
    if (u < nruns && run_bad(runs, nruns, nunits, src_bytes, u)) ++bad;
    const Unit w = unit_of(runs, nruns, nunits, src_bytes, u);
    if (w.n) memcpy(reinterpret_cast<void*>((uintptr_t)w.dst), src + w.src_off, w.n);
  }
  return bad;
}

// The record of one packed run (pack.hpp pack_run) of a file whose buffer
// starts at `base`: the run holds the file's blocks from `fblk` on, so it goes
// to base + fblk * bs.  unit_first: the units of the batch's earlier records;
// returns the units behind this one.
inline uint64_t record_of(const Run& r, uint64_t base, uint64_t fblk, uint64_t bs,
                          uint64_t unit_first, uint64_t* rec) {
  rec[0] = unit_first;
  rec[1] = r.pos;
  rec[2] = base + fblk * bs;
  rec[3] = r.bytes;
  return unit_first + units(r.bytes);
}

}  // namespace scatter
}  // namespace cir
#endif
