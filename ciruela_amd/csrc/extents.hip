// A new image's local block copies merged into extents on the device
// (cir_match_extents_dev, behind the join of cir_block_sources /
// cir_block_extents): match[] and the two run tables in, the per-block
// (src, file, block) arrays, the bitmap of what is left to fetch and one
// record per extent out.  The rule -- where a block's copy sits, and when two
// neighbours' copies continue one another -- is extents.hpp, shared with the
// host path and fuzzed there.
//
// Map, scan, emit, finish: four launches on the caller's stream, and no
// workgroup ever waits for another:
//   k_map_matches   one lane per need block, kExtTile blocks per workgroup in
//                   kExtTile / kThreads turns.  A lane maps its block (two
//                   bisections, one length check), gets block g - 1's mapping
//                   from the lane below by wave shuffles (lane 0 maps g - 1
//                   itself, lane 63 maps g + 1 itself) and so knows whether it
//                   is the head and whether it is the tail of an extent.  A
//                   wave owns one aligned word of each bitmap per turn: the
//                   fetch word goes to the caller, the head and the tail word
//                   to scratch, the head count into the tile's total.  The
//                   counts are reduced per wave, one atomicAdd per wave and
//                   count that has any.
//   k_extent_scan   one workgroup turns the tile totals into exclusive
//                   prefixes in place and writes the extent count and the
//                   status.  A launch of its own on purpose: no look-back.
//   k_extent_emit   the same tiling, gated on the status.  Heads and tails
//                   alternate, so a tail's ordinal is (heads at or before it)
//                   - 1.  The head lane of extent k maps its block again and
//                   writes first, need_file, need_block, src, src_file,
//                   src_block; the tail lane writes its own block number and
//                   the offset at which it ends into the count and bytes
//                   words.  Nobody walks an extent.
//   k_extent_finish one lane per record: count = tail - first + 1, bytes =
//                   tail's end - need_block bs.
// Every loop is bounded by an argument (the bisections by the table lengths,
// the turns by the tile), none by data, and no barrier sits in divergent code.
#include "extents.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

namespace {

using extents::Map;
using extents::Tables;

constexpr uint32_t kTurns = kExtTile / kThreads;
constexpr uint32_t kTileWords = kExtTile / 64;
static_assert(kExtTile % kThreads == 0 && kThreads % 64 == 0, "a wave owns whole bitmap words");
static_assert(kTileWords <= 64, "a wave scans a tile's head words in one shuffle scan");
constexpr uint32_t kScanPer = 8;  // tiles per lane and step of k_extent_scan

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v) {
  return __shfl_up((unsigned long long)v, 1, 64);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor((unsigned long long)v, d, 64);
  return v;
}

}  // namespace

// work: head words [0, nwords), tail words [nwords, 2 nwords), tile totals
// [2 nwords, 2 nwords + ntiles], the last one the gate.  res[1..4] were zeroed
// on the same stream before the launch.
__global__ __launch_bounds__(kThreads) void k_map_matches(
    Tables t, uint32_t* __restrict__ src, uint64_t* __restrict__ file, uint64_t* __restrict__ block,
    uint64_t* __restrict__ fetch, uint64_t* __restrict__ heads, uint64_t* __restrict__ tails,
    uint64_t* __restrict__ tot, uint64_t* __restrict__ res) {
  __shared__ uint32_t wave_heads[kThreads / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t n = t.n_need;
  uint32_t n_heads = 0, wanted = 0, found = 0, dropped = 0;  // (wave-uniform: ballot counts)
  uint64_t bytes = 0;                                        // (per lane)
#pragma unroll 1
  for (uint32_t turn = 0; turn < kTurns; ++turn) {
    const uint64_t g = (uint64_t)blockIdx.x * kExtTile + turn * kThreads + threadIdx.x;
    const uint64_t g0 = g - lane;  // the wave's first block: a multiple of 64
    if (g0 >= n) break;            // (wave-uniform; no barrier inside the loop)
    const Map m = extents::map_block(t, g);  // (g >= n: in no file)
    if (g < n && src) {
      src[g] = m.src;
      file[g] = m.file;
      block[g] = m.block;
    }
    // block g - 1's mapping: the lane below, or our own bisection at the wave's edge
    uint32_t p_flags = __shfl_up(m.flags, 1, 64);
    uint32_t p_src = __shfl_up(m.src, 1, 64);
    uint64_t p_run = shfl_up64(m.run), p_file = shfl_up64(m.file), p_block = shfl_up64(m.block);
    if (lane == 0) {
      p_flags = 0;
      if (g >= 1) {
        const Map p = extents::map_block(t, g - 1);
        p_flags = p.flags;
        p_src = p.src;
        p_run = p.run;
        p_file = p.file;
        p_block = p.block;
      }
    }
    const bool is_found = m.flags & extents::kFound;
    const bool c = extents::cont(p_flags, p_run, p_src, p_file, p_block, m.flags, m.run, m.src,
                                 m.file, m.block);
    // cont(g + 1): the lane above, or our own bisection at the wave's edge
    bool c_next = __shfl_down((int)c, 1, 64);
    if (lane == 63) c_next = g + 1 < n && extents::cont(m, extents::map_block(t, g + 1));
    const bool head = is_found && !c;
    const bool tail = is_found && !c_next;  // (g + 1 >= n: map_block is "in no file", cont false)
    const uint64_t w_fetch = __ballot((m.flags & extents::kWanted) && !is_found);
    const uint64_t w_head = __ballot(head), w_tail = __ballot(tail);
    wanted += (uint32_t)__popcll(__ballot(m.flags & extents::kWanted));
    found += (uint32_t)__popcll(__ballot(is_found));
    dropped += (uint32_t)__popcll(__ballot(m.flags & extents::kDropped));
    n_heads += (uint32_t)__popcll(w_head);
    bytes += m.len;
    if (lane == 0) {
      const uint64_t w = g0 >> 6;  // (g0 < n: the word exists)
      if (fetch) fetch[w] = w_fetch;
      heads[w] = w_head;
      tails[w] = w_tail;
    }
  }
  bytes = wave_sum(bytes);
  if (lane == 0) {
    wave_heads[wave] = n_heads;
    unsigned long long* r = reinterpret_cast<unsigned long long*>(res);
    if (wanted) atomicAdd(r + 1, (unsigned long long)wanted);
    if (found) atomicAdd(r + 2, (unsigned long long)found);
    if (bytes) atomicAdd(r + 3, (unsigned long long)bytes);
    if (dropped) atomicAdd(r + 4, (unsigned long long)dropped);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kThreads / 64; ++k) sum += wave_heads[k];
    tot[blockIdx.x] = sum;
  }
}

// One workgroup: tot[t] becomes the number of heads in the tiles before t;
// res[5] = the extents, res[0] = the status, tot[ntiles] = the same status,
// the gate of the emit pass.
__global__ __launch_bounds__(kThreads) void k_extent_scan(uint64_t* __restrict__ tot,
                                                          uint64_t ntiles, uint64_t cap_extents,
                                                          uint64_t* __restrict__ res) {
  __shared__ uint64_t lds[kThreads / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = 0;  // the same in every lane
  for (uint64_t base = 0; base < ntiles; base += (uint64_t)kThreads * kScanPer) {
    const uint64_t i0 = base + (uint64_t)threadIdx.x * kScanPer;
    uint64_t v[kScanPer], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      v[k] = i0 + k < ntiles ? tot[i0 + k] : 0;
      mine += v[k];
    }
    uint64_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t a = __shfl_up((unsigned long long)inc, d, 64);
      if ((int)lane >= d) inc += a;
    }
    __syncthreads();  // (the previous step's readers are done with lds)
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint64_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kThreads / 64; ++k) {
      const uint64_t x = lds[k];
      if (k < wave) before += x;
      sum += x;
    }
    uint64_t p = carry + before + inc - mine;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      if (i0 + k < ntiles) tot[i0 + k] = p;
      p += v[k];
    }
    carry += sum;
  }
  if (threadIdx.x == 0) {
    const uint64_t st = carry > cap_extents ? extents::kCapacity : extents::kOk;
    res[5] = carry;
    res[0] = st;
    tot[ntiles] = st;
  }
}

// Nothing unless the scan's status (*gate) is OK (then every ordinal is below
// cap_extents; the compare stays all the same).
__global__ __launch_bounds__(kThreads) void k_extent_emit(
    Tables t, const uint64_t* __restrict__ heads, const uint64_t* __restrict__ tails,
    const uint64_t* __restrict__ tot, const uint64_t* __restrict__ gate,
    uint64_t* __restrict__ ext, uint64_t cap_extents) {
  if (*gate != extents::kOk) return;  // (uniform: every lane reads the same word)
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t n = t.n_need;
  const uint64_t nwords = (n + 63) / 64;
  // heads in the tile's words before word k, in lane k: one shuffle scan per wave
  const uint64_t w0 = (uint64_t)blockIdx.x * kTileWords;
  const uint32_t pc = lane < kTileWords && w0 + lane < nwords ? (uint32_t)__popcll(heads[w0 + lane]) : 0;
  uint32_t inc = pc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t a = __shfl_up(inc, d, 64);
    if ((int)lane >= d) inc += a;
  }
  const uint32_t excl = inc - pc;
  const uint64_t tile_base = tot[blockIdx.x];
#pragma unroll 1
  for (uint32_t turn = 0; turn < kTurns; ++turn) {
    const uint32_t wi = turn * (kThreads / 64) + wave;  // the wave's word inside the tile
    const uint32_t before = __shfl(excl, (int)wi, 64);  // (every lane takes part)
    const uint64_t g = (uint64_t)blockIdx.x * kExtTile + turn * kThreads + threadIdx.x;
    if (g < n) {
      const uint64_t hw = heads[w0 + wi], tw = tails[w0 + wi];
      const bool head = hw >> lane & 1, tail = tw >> lane & 1;
      const uint64_t upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1;
      // heads at or before g, minus one: the extent a head or a tail at g belongs to
      const uint64_t k = tile_base + before + (uint32_t)__popcll(hw & upto) - 1;
      if ((head || tail) && k < cap_extents) {
        const Map m = extents::map_block(t, g);
        uint64_t* o = ext + extents::kRecWords * k;
        if (head) {
          o[0] = g;
          o[2] = m.need_file;
          o[3] = m.need_block;
          o[4] = m.src;
          o[5] = m.file;
          o[6] = m.block;
        }
        if (tail) {
          o[1] = g;           // k_extent_finish: count = this - first + 1
          o[7] = m.need_end;  // k_extent_finish: bytes = this - need_block bs
        }
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_extent_finish(uint64_t* __restrict__ ext,
                                                            const uint64_t* __restrict__ res,
                                                            const uint64_t* __restrict__ gate,
                                                            uint64_t cap_extents, uint64_t bs) {
  if (*gate != extents::kOk) return;
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= res[5] || k >= cap_extents) return;
  uint64_t* o = ext + extents::kRecWords * k;
  o[1] = o[1] - o[0] + 1;
  o[7] = extents::extent_bytes(o[3], o[7], bs);
}

namespace {
inline Tables tables_of(const ExtentArgs& a) {
  return Tables{a.match, a.n_need, a.need_runs, a.n_need_runs, a.pool_runs,
                a.n_pool_runs, a.n_pool, a.bs, a.want};
}
}  // namespace

hipError_t launch_extent_map(const ExtentArgs& a, uint32_t* src, uint64_t* file, uint64_t* block,
                             uint64_t* fetch, uint64_t cap_extents, uint64_t* work, uint64_t* res,
                             hipStream_t s, const hipEvent_t* tev) {
  hipError_t e = hipMemsetAsync(res, 0, extents::kResFields * sizeof(uint64_t), s);
  if (e == hipSuccess && tev) e = hipEventRecord(tev[0], s);
  if (e != hipSuccess) return e;
  const uint64_t nwords = (a.n_need + 63) / 64, ntiles = ext_tiles(a.n_need);
  uint64_t* tot = work + 2 * nwords;
  if (ntiles) {
    hipLaunchKernelGGL(k_map_matches, dim3((unsigned)ntiles), dim3(kThreads), 0, s, tables_of(a),
                       src, file, block, fetch, work, work + nwords, tot, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (tev && (e = hipEventRecord(tev[1], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_extent_scan, dim3(1), dim3(kThreads), 0, s, tot, ntiles, cap_extents, res);
  e = hipGetLastError();
  if (e == hipSuccess && tev) e = hipEventRecord(tev[2], s);
  return e;
}

hipError_t launch_extent_emit(const ExtentArgs& a, uint64_t* ext, uint64_t cap_extents,
                              uint64_t max_extents, uint64_t* work, uint64_t* res, hipStream_t s) {
  const uint64_t nwords = (a.n_need + 63) / 64, ntiles = ext_tiles(a.n_need);
  if (ntiles == 0 || cap_extents == 0 || max_extents == 0) return hipSuccess;
  const uint64_t* tot = work + 2 * nwords;
  hipLaunchKernelGGL(k_extent_emit, dim3((unsigned)ntiles), dim3(kThreads), 0, s, tables_of(a),
                     work, work + nwords, tot, tot + ntiles, ext, cap_extents);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (max_extents > cap_extents) max_extents = cap_extents;
  hipLaunchKernelGGL(k_extent_finish, dim3((unsigned)((max_extents + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, ext, res, tot + ntiles, cap_extents, a.bs);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace cir
