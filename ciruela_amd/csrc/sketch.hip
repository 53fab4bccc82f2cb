// The content sketch of a digest list on the device (cir_sketch_digests_dev,
// the device half of cir_index_sketch): the k smallest distinct 64-bit keys of
// n digests, ascending.  The rule -- the key of a digest, what a sketch is -- is
// sketch.hpp.
//
// The reference picks the older images it compares a new one with by timestamp
// (the 37 most recent of the base directory, src/daemon/metadata/
// hardlink_sources.rs:66-90); a sketch per image lets a caller pick them by
// content before any of their texts is uploaded.
//
// Five steps behind two memsets on the caller's stream, each a launch of its
// own: no workgroup waits for another.
//   k_sketch_insert   lane j folds digest j to its key and puts the key into an
//                     open-addressing set of u64 (linear probing, the CAS idiom
//                     of k_join_build); the lane that wins a key's slot -- one
//                     per distinct key -- bumps a histogram of the key's top bits;
//   k_sketch_scan     one workgroup walks the histogram to the first bin at
//                     which the distinct count reaches k (the last bin when it
//                     never does);
//   k_sketch_compact  one pass over the set's slots appends the keys at or
//                     below that bin to the candidate buffer, one atomic add
//                     per wave;
//   k_sketch_sort     one workgroup sorts the candidates in LDS and writes the
//                     first k and the result words.
// The candidates are every distinct key at or below the bin that holds the
// k-th smallest, so the first k of them sorted are the sketch.
//
// What the scratch cannot hold is declined, never cut short: more than
// kSketchCands candidates (a histogram bin has about 64 keys of uniformly
// spread ones; thousands of distinct keys that share their top bits are a
// crafted index), or a key whose probe walk passes kSketchWalk slots (keys are
// placed by a fixed mix of their own bits, so an author who chooses keys can
// cluster them; at load <= 0.5 random keys walk a few tens of slots at most).
//
// The key 2^64 - 1 is the set's "empty": a digest with that key sets a flag
// instead, and the last kernel appends it -- the largest key there is -- when
// fewer than k others exist.  The key 0 is an ordinary member.
//
// work, in u64 words: head[kSketchHeadWords] = {cursor, has-max flag,
// threshold bin, candidates expected, declined flag, ...}, kSketchCands
// candidates, the histogram (u32 bins), the set.
#include "digest_slot.hpp"
#include "kernels.hpp"
#include "sketch.hpp"

namespace cir {
namespace dev {

constexpr int kSketchWide = 1024;  // threads of the two single-workgroup kernels
enum : int { kHeadCursor = 0, kHeadMax = 1, kHeadBin = 2, kHeadCum = 3, kHeadDeclined = 4 };

__device__ __forceinline__ uint64_t sketch_key(const Digest& d) {
  uint64_t x = sketch::kSeed;
  x = mix_word(x, d.lo.x, d.lo.y);
  x = mix_word(x, d.lo.z, d.lo.w);
  x = mix_word(x, d.hi.x, d.hi.y);
  x = mix_word(x, d.hi.z, d.hi.w);
  return x;
}

// Lane j walks from its key's home slot.  At each slot: read it (a relaxed
// agent-scope atomic load); if it is empty, CAS the key in -- done, and this
// lane counts the key, when that returned empty, else go on with the value it
// returned; a slot that holds the lane's key: done; else the next slot.  As in
// k_join_build no lane waits for another's write, a slot never returns to
// empty and never changes once taken, so every distinct key owns exactly one
// slot and is counted once.  The walk ends after kSketchWalk slots at the
// latest (fewer than the set's slots: at least 1024), and a lane that runs out
// declines the call.
__global__ __launch_bounds__(kThreads) void k_sketch_insert(const uint8_t* __restrict__ digests,
                                                            uint32_t n,
                                                            unsigned long long* __restrict__ table,
                                                            uint32_t slot_bits,
                                                            uint32_t* __restrict__ hist,
                                                            uint32_t hist_shift,
                                                            uint64_t* head) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint64_t key = sketch_key(load_digest(digests, j));
  if (key == kSketchEmpty) {
    __hip_atomic_store(head + kHeadMax, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const uint64_t mask = (1ull << slot_bits) - 1;
  uint64_t at = (key * sketch::kMul) >> (64 - slot_bits);
  for (uint32_t step = 0; step < kSketchWalk; ++step) {
    unsigned long long v =
        __hip_atomic_load(table + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == kSketchEmpty) {
      v = atomicCAS(table + at, (unsigned long long)kSketchEmpty, (unsigned long long)key);
      if (v == kSketchEmpty) {
        atomicAdd(hist + (key >> hist_shift), 1u);
        return;
      }
    }
    if (v == key) return;
    at = (at + 1) & mask;
  }
  __hip_atomic_store(head + kHeadDeclined, (uint64_t)1, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup, kSketchWide bins per turn (bins is a multiple of it): a
// workgroup-wide inclusive sum of the turn's bins on top of the turns before;
// the sums rise with the thread index, so the first thread at or past k is the
// number of threads below it.  head[kHeadBin] = that bin, head[kHeadCum] = the
// distinct keys up to and including it; the last bin and every key when k is
// never reached.
__global__ __launch_bounds__(kSketchWide) void k_sketch_scan(const uint32_t* __restrict__ hist,
                                                             uint32_t bins, uint32_t k,
                                                             uint64_t* __restrict__ head) {
  __shared__ uint32_t wsum[kSketchWide / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t running = 0;
  for (uint32_t base = 0; base < bins; base += kSketchWide) {
    uint32_t incl = hist[base + tid];
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t below = 0, total = 0;
    for (uint32_t w = 0; w < kSketchWide / 64; ++w) {
      const uint32_t t = wsum[w];
      if (w < wave) below += t;
      total += t;
    }
    const uint64_t mine = running + below + incl;
    const uint32_t short_of_k = (uint32_t)__syncthreads_count(mine < k);
    if (short_of_k < kSketchWide) {
      if (tid == short_of_k) {
        head[kHeadBin] = base + tid;
        head[kHeadCum] = mine;
        if (mine > kSketchCands) head[kHeadDeclined] = 1;
      }
      return;
    }
    running += total;
  }
  if (tid == 0) {
    head[kHeadBin] = bins - 1;
    head[kHeadCum] = running;  // (< k <= kSketchCands)
  }
}

// Lane i reads slot i (the grid is exactly the set's slots).  One ballot per
// wave, one atomic add on the cursor per wave that has a candidate; a lane
// whose place is past the buffer (never, when the histogram and the set agree)
// writes nothing and declines the call.
__global__ __launch_bounds__(kThreads) void k_sketch_compact(const uint64_t* __restrict__ table,
                                                             uint32_t hist_shift,
                                                             uint64_t* head,
                                                             uint64_t* __restrict__ cands) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t v = table[i];
  const bool take = head[kHeadDeclined] == 0 && v != kSketchEmpty &&
                    (v >> hist_shift) <= head[kHeadBin];
  const uint64_t votes = __ballot(take);
  if (votes == 0) return;
  uint32_t base = 0;
  if (lane == 0)
    base = (uint32_t)atomicAdd((unsigned long long*)(head + kHeadCursor),
                               (unsigned long long)__popcll(votes));
  base = __shfl(base, 0, 64);
  if (!take) return;
  const uint32_t pos = base + (uint32_t)__popcll(votes & ((1ull << lane) - 1));
  if (pos < kSketchCands)
    cands[pos] = v;
  else
    __hip_atomic_store(head + kHeadDeclined, (uint64_t)1, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup: the candidates into LDS, padded with 2^64 - 1 (no candidate
// has that key) to 2048, 4096 or 8192, a bitonic sort, the first k out.
__global__ __launch_bounds__(kSketchWide) void k_sketch_sort(const uint64_t* __restrict__ head,
                                                             const uint64_t* __restrict__ cands,
                                                             uint32_t k, uint64_t n,
                                                             uint64_t* __restrict__ keys,
                                                             uint64_t* __restrict__ res) {
  __shared__ uint64_t s[kSketchCands];
  const uint32_t tid = threadIdx.x;
  const uint64_t cum = head[kHeadCum];
  if (head[kHeadDeclined] != 0 || cum > kSketchCands || head[kHeadCursor] != cum) {
    if (tid == 0) {
      res[0] = kSketchDeclined;
      res[1] = 0;
      res[2] = n;
      res[3] = cum;
    }
    return;
  }
  const uint32_t m = (uint32_t)cum;
  const uint32_t len = m <= 2048 ? 2048 : m <= 4096 ? 4096 : kSketchCands;
  for (uint32_t i = tid; i < len; i += kSketchWide) s[i] = i < m ? cands[i] : kSketchEmpty;
  __syncthreads();
  for (uint32_t size = 2; size <= len; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t p = tid; p < len / 2; p += kSketchWide) {
        const uint32_t lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
        const uint64_t a = s[lo], b = s[hi];
        const bool up = (lo & size) == 0;
        if ((a > b) == up) {
          s[lo] = b;
          s[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  uint32_t count = m < k ? m : k;
  for (uint32_t i = tid; i < count; i += kSketchWide) keys[i] = s[i];
  if (tid == 0) {
    if (m < k && head[kHeadMax] != 0) keys[count++] = kSketchEmpty;
    res[0] = kSketchOk;
    res[1] = count;
    res[2] = n;
    res[3] = cum;
  }
}

hipError_t launch_sketch(const uint8_t* digests, uint64_t n, uint32_t k, uint64_t* keys,
                         uint64_t* work, uint64_t* res, hipStream_t s, const hipEvent_t* tev) {
  static_assert(kSketchCands * sizeof(uint64_t) == 65536, "the sort's LDS is 64 KiB");
  static_assert(kSketchCands >= 2 * sketch::kMaxK && kSketchWalk <= 1024, "see above");
  const uint32_t hist_bits = sketch_hist_bits(n), hist_shift = 64 - hist_bits;
  const uint64_t slots = sketch_table_slots(n);
  uint32_t slot_bits = 0;
  while ((1ull << slot_bits) < slots) ++slot_bits;
  uint64_t* head = work;
  uint64_t* cands = head + kSketchHeadWords;
  uint32_t* hist = reinterpret_cast<uint32_t*>(cands + kSketchCands);
  uint64_t* table = cands + kSketchCands + ((1ull << hist_bits) / 2);
  hipError_t e = hipSuccess;
  if (tev && (e = hipEventRecord(tev[0], s)) != hipSuccess) return e;
  // the head and the histogram (the candidates between them ride along)
  e = hipMemsetAsync(work, 0, 8 * (kSketchHeadWords + (uint64_t)kSketchCands) + (4ull << hist_bits),
                     s);
  if (e != hipSuccess) return e;
  if (n) {
    if ((e = hipMemsetAsync(table, 0xFF, 8 * slots, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sketch_insert, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, digests, (uint32_t)n, (unsigned long long*)table,
                       slot_bits, hist, hist_shift, head);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_sketch_scan, dim3(1), dim3(kSketchWide), 0, s, hist, 1u << hist_bits, k,
                     head);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (n) {
    hipLaunchKernelGGL(k_sketch_compact, dim3((unsigned)(slots / kThreads)), dim3(kThreads), 0, s,
                       table, hist_shift, head, cands);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_sketch_sort, dim3(1), dim3(kSketchWide), 0, s, head, cands, k, n, keys,
                     res);
  e = hipGetLastError();
  if (e == hipSuccess && tev) e = hipEventRecord(tev[1], s);
  return e;
}

}  // namespace dev
}  // namespace cir
