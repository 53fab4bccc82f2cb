// Join of two digest lists on the device (cir_match_digests_dev, the device
// half of cir_block_sources): for every needed digest, the smallest ordinal
// of an equal digest in a pool.
//
// The daemon queues every block of every file it could not hardlink whole
// (fill_blocks, src/daemon/tracking/progress.rs:129-170), although older
// images of the same base directory may hold most of those blocks
// (scan_links matches whole files only, src/daemon/metadata/
// hardlink_sources.rs:131-133).  Which of the new index's blocks an older
// index lists, and where, is a join of two lists of 32-byte digests.
//
// An open-addressing table of u32 pool ordinals, linear probing, two kernels
// behind one memset on the caller's stream:
//   k_join_build  lane j puts pool ordinal j into the table;
//   k_join_probe  lane i looks need[i] up and stores its match.
// The home slot folds all 32 bytes of a digest under the caller's seed (pool
// digests come from other parties' indexes: digests crafted to share a prefix
// must not share a home slot, and a caller that joins untrusted digests
// passes a seed they cannot predict):
//   x = seed; for the four little-endian u64 words w of the digest, in order:
//   x = (x ^ w) * 0x9E3779B97F4A7C15, x ^= x >> 32;  home = x & (slots - 1).
// At the worst load (0.5) a CPU simulation of this mix gives 1.5 probed slots
// on average and about 40 at most for 2^20 random digests, and about 3,200
// distinct home slots of 8192 -- what random digests give -- for 4096 digests
// that differ only in their last word.
#include "digest_slot.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

// Lane j walks from its digest's home slot.  At each slot: read it (a relaxed
// agent-scope atomic load); if it is empty, atomicCAS(slot, EMPTY, j) -- done
// when that returned EMPTY, else go on with the value it returned; an
// occupied slot's ordinal v names a pool digest: equal to the lane's own ->
// atomicMin(slot, j) and done, else the next slot.
//
// What makes this correct whatever the timing:
//   * no lane ever waits for another lane's write: every retry follows a CAS
//     that returned a non-empty value, which the lane then examines, so the
//     walk is a `for` over at most `slots` steps and ends on its own (the
//     table has at least twice as many slots as digests: an empty slot, or
//     the digest's own, is met before the walk wraps);
//   * a slot never returns to empty, and an occupied slot's value is only
//     ever replaced (atomicMin) by the ordinal of an equal digest.  So every
//     distinct digest owns exactly one slot, the first free one of its probe
//     sequence at the time its first lane arrived -- every later lane with
//     that digest meets only slots that were already taken by other digests,
//     then this one -- and that slot ends holding the digest's smallest
//     ordinal;
//   * a stale read can show "empty" (the CAS then tells the truth) or an
//     older, larger ordinal of an equal digest (it compares equal all the
//     same): both are harmless.
// All table accesses are the ordinary vector atomics on global u32 at agent
// scope; the pool is read-only.  (v < n cannot fail after the memset; the
// compare keeps a table the call did not initialise from sending a load
// outside the pool.)
__global__ __launch_bounds__(kThreads) void k_join_build(const uint8_t* __restrict__ pool,
                                                         uint32_t n, uint32_t* __restrict__ table,
                                                         uint64_t slots, uint64_t seed) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const Digest mine = load_digest(pool, j);
  const uint64_t mask = slots - 1;
  uint64_t at = home_slot(mine, seed, mask);
  for (uint64_t step = 0; step < slots; ++step) {
    uint32_t v = __hip_atomic_load(table + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == kJoinEmpty) {
      v = atomicCAS(table + at, kJoinEmpty, (uint32_t)j);
      if (v == kJoinEmpty) return;
    }
    if (v < n && same_digest(load_digest(pool, v), mine)) {
      if (v > (uint32_t)j) atomicMin(table + at, (uint32_t)j);  // (the value only ever falls)
      return;
    }
    at = (at + 1) & mask;
  }
}

// Launched behind k_join_build on the same stream, so plain loads of the
// table see its final state.  Lane i walks from its digest's home slot: an
// empty slot is a miss, an occupied slot whose pool digest equals the lane's
// is a hit, anything else the next slot (bounded as above).  One ballot per
// wave and one atomicAdd per wave that has a hit.
__global__ __launch_bounds__(kThreads) void k_join_probe(const uint8_t* __restrict__ need,
                                                         uint64_t n_need,
                                                         const uint8_t* __restrict__ pool,
                                                         uint32_t n, const uint32_t* __restrict__ table,
                                                         uint64_t slots, uint64_t seed,
                                                         uint32_t* __restrict__ match,
                                                         uint32_t* __restrict__ nmatch) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool hit = false;
  if (i < n_need) {
    const Digest mine = load_digest(need, i);
    const uint64_t mask = slots - 1;
    uint64_t at = home_slot(mine, seed, mask);
    uint32_t found = kJoinEmpty;
    for (uint64_t step = 0; step < slots; ++step) {
      const uint32_t v = table[at];
      if (v >= n) break;  // empty (or not an ordinal: never after the build)
      if (same_digest(load_digest(pool, v), mine)) {
        found = v;
        break;
      }
      at = (at + 1) & mask;
    }
    match[i] = found;
    hit = found != kJoinEmpty;
  }
  const uint64_t votes = __ballot(hit);
  if (nmatch && votes && (threadIdx.x & 63) == 0) atomicAdd(nmatch, (uint32_t)__popcll(votes));
}

hipError_t launch_join(const uint8_t* need, uint64_t n_need, const uint8_t* pool, uint64_t n_pool,
                       uint32_t* table, uint64_t table_slots, uint64_t seed, uint32_t* match,
                       uint32_t* nmatch, hipStream_t s, const hipEvent_t* tev) {
  static_assert(kThreads % 64 == 0, "whole waves per workgroup");
  hipError_t e = hipSuccess;
  if (nmatch) e = hipMemsetAsync(nmatch, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (n_need == 0 || n_pool == 0) {  // nothing to build: every entry is a miss
    if (n_need) e = hipMemsetAsync(match, 0xFF, n_need * sizeof(uint32_t), s);
    for (int k = 0; k < 3 && tev && e == hipSuccess; ++k) e = hipEventRecord(tev[k], s);
    return e;
  }
  e = hipMemsetAsync(table, 0xFF, table_slots * sizeof(uint32_t), s);
  if (e == hipSuccess && tev) e = hipEventRecord(tev[0], s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_join_build, dim3((unsigned)((n_pool + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, pool, (uint32_t)n_pool, table, table_slots, seed);
  e = hipGetLastError();
  if (e == hipSuccess && tev) e = hipEventRecord(tev[1], s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_join_probe, dim3((unsigned)((n_need + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, need, n_need, pool, (uint32_t)n_pool, table, table_slots,
                     seed, match, nmatch);
  e = hipGetLastError();
  if (e == hipSuccess && tev) e = hipEventRecord(tev[2], s);
  return e;
}

}  // namespace dev
}  // namespace cir
