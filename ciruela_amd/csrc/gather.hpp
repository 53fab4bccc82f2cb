// The rule of the gather behind cir_store_blocks (cir_gather_runs,
// cir_gather_runs_dev), written once for the host and the device: bytes that
// lie anywhere in memory copied into the packed runs of a staging slot.  The
// inverse of scatter.hpp, whose table shape, units() and run_at() it uses.  No
// HIP runtime call; compiled by gather.hip (the kernel), store.cpp (the table
// and the host form) and, alone under the sanitizers, by tools/gather_fuzz.cpp.
// The reference has no counterpart: what it writes to an image directory comes
// from the network, block by block (src/daemon/disk/public.rs write_block).
//
// Table: one record of kRunWords u64 per packed run {unit_first, dst_pos, src,
// bytes}: `bytes` (> 0) bytes at the address `src` (any alignment) go to byte
// `dst_pos` of the destination (a multiple of 16, as pack_run lays runs out).
// A record has units(bytes) units of 16 bytes; unit_first is the unit count of
// all earlier records, nunits that of the table.
//
// Unit u belongs to the record found by bisection on unit_first
// (scatter::run_at); with k = u - unit_first it owns the 16 aligned destination
// bytes [dst_pos + 16 k, dst_pos + 16 k + 16) and writes all of them: its n =
// min(16, bytes - 16 k) source bytes [src + 16 k, src + 16 k + n), then zeros.
// So no two units store to one byte (the records' rounded ranges do not overlap
// when their runs do not: runs start on multiples of 16), nothing is read
// outside [src, src + bytes), and nothing is written outside the records'
// ranges rounded up to 16.
//
// Untrusted tables: record r is bad when its dst_pos is not a multiple of 16,
// its bytes is 0, its rounded range [dst_pos, dst_pos + 16 units(bytes)) does
// not lie inside [0, dst_bytes] (decided without overflow), or its unit_first is
// not that of record r - 1 plus r - 1's units (0 for r = 0; the last record must
// also end at nunits).  A bad record is written nowhere and read nowhere, and
// it is counted once, by unit r, exactly as in scatter.hpp; a unit past its
// record's units copies nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scatter.hpp"

namespace cir {
namespace gather {

constexpr int kRunWords = scatter::kRunWords;  // {unit_first, dst_pos, src, bytes}
constexpr uint64_t kMaxRuns = scatter::kMaxRuns;
constexpr uint64_t kMaxUnits = scatter::kMaxUnits;

// Is record r (< nruns) one that nothing may be read or written through?
CIR_SCAT_HD inline bool run_bad(const uint64_t* runs, uint64_t nruns, uint64_t nunits,
                                uint64_t dst_bytes, uint64_t r) {
  const uint64_t* q = runs + kRunWords * r;
  const uint64_t first = q[0], pos = q[1], bytes = q[3];
  const uint64_t un = scatter::units(bytes);  // (<= 2^60: 16 * un wraps only above dst_bytes / 16)
  if ((pos & 15) || bytes == 0 || un > dst_bytes / 16 || pos > dst_bytes - 16 * un) return true;
  const uint64_t want = r ? q[-kRunWords] + scatter::units(q[-kRunWords + 3]) : 0;
  if (first != want) return true;
  return r + 1 == nruns && first + un != nunits;
}

// What unit u does: n source bytes (0: nothing at all) at the address src go
// to byte dst_off of the destination, 16 - n zeros behind them.
struct Unit {
  uint64_t src, dst_off;
  uint32_t n;
};

CIR_SCAT_HD inline Unit unit_of(const uint64_t* runs, uint64_t nruns, uint64_t nunits,
                                uint64_t dst_bytes, uint64_t u) {
  Unit w{0, 0, 0};
  if (u >= nunits) return w;
  const uint64_t r = scatter::run_at(runs, nruns, u);
  if (r == scatter::kNoRun || run_bad(runs, nruns, nunits, dst_bytes, r)) return w;
  const uint64_t* q = runs + kRunWords * r;
  const uint64_t k = u - q[0];
  if (k >= scatter::units(q[3])) return w;
  const uint64_t left = q[3] - 16 * k;
  w.dst_off = q[1] + 16 * k;
  w.src = q[2] + 16 * k;
  w.n = (uint32_t)(left < 16 ? left : 16);
  return w;
}

}  // namespace gather
}  // namespace cir

#if !defined(__HIP_DEVICE_COMPILE__)
namespace cir {
namespace gather {

// The host executor: every unit in turn, as the kernel's lanes would; returns
// the count of bad records.
inline uint64_t apply_host(uint8_t* dst, uint64_t dst_bytes, const uint64_t* runs, uint64_t nruns,
                           uint64_t nunits) {
  uint64_t bad = 0;
  const uint64_t n = scatter::lanes(nruns, nunits);
  for (uint64_t u = 0; u < n; ++u) {
    if (u < nruns && run_bad(runs, nruns, nunits, dst_bytes, u)) ++bad;
    const Unit w = unit_of(runs, nruns, nunits, dst_bytes, u);
    if (!w.n) continue;
    uint8_t line[16] = {0};
    memcpy(line, reinterpret_cast<const void*>((uintptr_t)w.src), w.n);
    memcpy(dst + w.dst_off, line, 16);
  }
  return bad;
}

// The record of one packed run (pack.hpp pack_run) of a file whose bytes start
// at `base`: the run holds the file's blocks from `fblk` on, so it comes from
// base + fblk * bs.  unit_first: the units of the batch's earlier records;
// returns the units behind this one.
inline uint64_t record_of(const Run& r, uint64_t base, uint64_t fblk, uint64_t bs,
                          uint64_t unit_first, uint64_t* rec) {
  rec[0] = unit_first;
  rec[1] = r.pos;
  rec[2] = base + fblk * bs;
  rec[3] = r.bytes;
  return unit_first + scatter::units(r.bytes);
}

}  // namespace gather
}  // namespace cir
#endif
