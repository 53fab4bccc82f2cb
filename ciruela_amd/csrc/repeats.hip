// Join of one digest list with itself on the device (cir_match_repeats_dev, the
// device half of cir_block_repeats): for every wanted block, the leader of its
// digest among the blocks of the same index that take part.
//
// After the hardlinks, the resume bitmap and the copies from older images,
// fill_blocks (src/daemon/tracking/progress.rs:129-170) still queues one Block
// per (path, offset): a digest that occurs twice inside the new image -- a
// vendored directory, one shared object under two paths, a zero-filled file --
// is fetched twice.  The rule is repeats.hpp: a block's key is g when present
// and 2^31 + g when wanted, and the leader of a digest is its smallest key.
//
// join.hip's table on join.hip's discipline, holding keys instead of pool
// ordinals (the home slot and its seed contract are digest_slot.hpp), two
// kernels behind one memset on the caller's stream:
//   k_repeat_build  lane g puts its key into the table;
//   k_repeat_probe  lane g looks its own digest up and stores its match.
#include "digest_slot.hpp"
#include "kernels.hpp"
#include "repeats.hpp"

namespace cir {
namespace dev {

static_assert(kRepeatMaxBlocks == repeats::kMaxBlocks && kJoinEmpty == repeats::kNone,
              "the launcher's limits are the rule's");

// Lane g reads its want and present bits; a block that takes no part returns.
// Otherwise it walks from its digest's home slot.  At each slot: read it (a
// relaxed agent-scope atomic load); if it is empty, atomicCAS(slot, EMPTY,
// key) -- done when that returned EMPTY, else go on with the value it
// returned; an occupied slot's key v names block v & 0x7FFFFFFF: its digest
// equal to the lane's own -> atomicMin(slot, key) when v > key, and done, else
// the next slot.
//
// What makes this correct whatever the timing (join.hip's argument, for keys):
//   * no lane ever waits for another lane's write: every retry follows a CAS
//     that returned a non-empty value, which the lane then examines, so the
//     walk is a `for` over at most `slots` steps and ends on its own (the
//     table has at least twice as many slots as blocks: an empty slot, or the
//     digest's own, is met before the walk wraps);
//   * a slot never returns to empty, and an occupied slot's value is only
//     ever replaced (atomicMin) by the key of an equal digest.  So every
//     distinct digest owns exactly one slot, the first free one of its probe
//     sequence at the time its first lane arrived -- every later lane with
//     that digest meets only slots that were already taken by other digests,
//     then this one -- and that slot ends holding the digest's smallest key:
//     its leader;
//   * a stale read can show "empty" (the CAS then tells the truth) or an
//     older, larger key of an equal digest (it compares equal all the same):
//     both are harmless.
// All table accesses are the ordinary vector atomics on global u32 at agent
// scope; the digests and the bitmaps are read-only.  (The ordinal of a key is
// below n after the memset; the compare keeps a table the call did not
// initialise from sending a load outside the digests.  EMPTY's ordinal is
// 2^31 - 1 > n.)
__global__ __launch_bounds__(kThreads) void k_repeat_build(const uint8_t* __restrict__ digests,
                                                           uint32_t n,
                                                           const uint64_t* __restrict__ want,
                                                           const uint64_t* __restrict__ present,
                                                           uint32_t* __restrict__ table,
                                                           uint64_t slots, uint64_t seed) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= n) return;
  const uint32_t key = repeats::key_of(want, present, g);
  if (key == repeats::kNone) return;
  const Digest mine = load_digest(digests, g);
  const uint64_t mask = slots - 1;
  uint64_t at = home_slot(mine, seed, mask);
  for (uint64_t step = 0; step < slots; ++step) {
    uint32_t v = __hip_atomic_load(table + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == kJoinEmpty) {
      v = atomicCAS(table + at, kJoinEmpty, key);
      if (v == kJoinEmpty) return;
    }
    const uint32_t b = repeats::key_block(v);
    if (b < n && same_digest(load_digest(digests, b), mine)) {
      if (v > key) atomicMin(table + at, key);  // (the value only ever falls)
      return;
    }
    at = (at + 1) & mask;
  }
}

// Launched behind k_repeat_build on the same stream, so plain loads of the
// table see its final state.  A wanted lane walks from its digest's home slot
// to the slot whose block has its digest -- its own build put one there; the
// walk is bounded all the same, and one that ends without a hit (an empty
// slot, a value that is no key) stores UINT32_MAX.  The slot's key is the
// leader: the lane's own key -> UINT32_MAX, a present block L -> L, a wanted
// block L -> n + L.  Unwanted lanes store UINT32_MAX.  One ballot per wave
// and one atomicAdd per wave that has a repeat.
__global__ __launch_bounds__(kThreads) void k_repeat_probe(const uint8_t* __restrict__ digests,
                                                           uint32_t n,
                                                           const uint64_t* __restrict__ want,
                                                           const uint64_t* __restrict__ present,
                                                           const uint32_t* __restrict__ table,
                                                           uint64_t slots, uint64_t seed,
                                                           uint32_t* __restrict__ match,
                                                           uint32_t* __restrict__ nmatch) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool hit = false;
  if (g < n) {
    const uint32_t key = repeats::key_of(want, present, g);
    uint32_t found = repeats::kNone;
    if (repeats::key_wanted(key)) {
      const Digest mine = load_digest(digests, g);
      const uint64_t mask = slots - 1;
      uint64_t at = home_slot(mine, seed, mask);
      for (uint64_t step = 0; step < slots; ++step) {
        const uint32_t v = table[at];
        const uint32_t b = repeats::key_block(v);
        if (b >= n) break;  // empty (or not a key: never after the build)
        if (same_digest(load_digest(digests, b), mine)) {
          found = repeats::match_of(key, v, n);
          break;
        }
        at = (at + 1) & mask;
      }
    }
    match[g] = found;
    hit = found != repeats::kNone;
  }
  const uint64_t votes = __ballot(hit);
  if (nmatch && votes && (threadIdx.x & 63) == 0) atomicAdd(nmatch, (uint32_t)__popcll(votes));
}

hipError_t launch_repeat_join(const uint8_t* digests, uint64_t n, const uint64_t* want,
                              const uint64_t* present, uint32_t* table, uint64_t table_slots,
                              uint64_t seed, uint32_t* match, uint32_t* nmatch, hipStream_t s,
                              const hipEvent_t* tev) {
  static_assert(kThreads % 64 == 0, "whole waves per workgroup");
  hipError_t e = hipSuccess;
  if (nmatch) e = hipMemsetAsync(nmatch, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (n == 0) {  // nothing to join: only the count is written
    for (int k = 0; k < 3 && tev && e == hipSuccess; ++k) e = hipEventRecord(tev[k], s);
    return e;
  }
  e = hipMemsetAsync(table, 0xFF, table_slots * sizeof(uint32_t), s);
  if (e == hipSuccess && tev) e = hipEventRecord(tev[0], s);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_repeat_build, grid, dim3(kThreads), 0, s, digests, (uint32_t)n, want,
                     present, table, table_slots, seed);
  e = hipGetLastError();
  if (e == hipSuccess && tev) e = hipEventRecord(tev[1], s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_repeat_probe, grid, dim3(kThreads), 0, s, digests, (uint32_t)n, want,
                     present, table, table_slots, seed, match, nmatch);
  e = hipGetLastError();
  if (e == hipSuccess && tev) e = hipEventRecord(tev[2], s);
  return e;
}

}  // namespace dev
}  // namespace cir
