// The kernels of cir_copy_runs_dev and of cir_reload_blocks' memory half: runs
// of bytes copied between buffers of any alignment inside device memory, and
// the table of those runs made on the device from the join's answer.  The rules
// are copyblk.hpp; the reference has no counterpart (it holds no image in
// device memory).
//
//   k_copy_runs : one lane per 16-byte unit of the table, in a 64-bit
//                 grid-stride loop whose bounds are uniform over the workgroup.
//                 The lane bisects the table by unit_first (scatter::run_at, at
//                 most 32 steps), looks at its record (copyblk::run_bad) and,
//                 if the record is sound, loads its n source bytes into four
//                 registers with the widest loads the source's alignment allows
//                 (k_gather_runs' ladder: one dwordx4 at 16, else 8, 4, 2 bytes
//                 or single bytes; a short last unit byte by byte, so nothing is
//                 read outside [src, src + bytes)) and stores them with the
//                 widest stores the destination's alignment allows
//                 (k_scatter_runs' ladder), only its own n bytes.  Lane r also
//                 looks at record r and counts it when it is bad: one
//                 atomicAdd per wave that met any, behind the launcher's memset
//                 on the same stream.  No LDS, no scratch, no lane waits for
//                 another; the ballots sit where every lane of the wave arrives.
//   k_copy_plan : one lane per global block of the new index, a wave per tile
//                 of 64 blocks.  The lane decides its block (copyblk::take_of:
//                 two bisections and a length test); the wave's 64 verdicts are
//                 one ballot and lane 0 stores it to the have bitmap with one
//                 vector store, k_block_bits' discipline: every word of [0,
//                 ceil(n / 64)) is written, no atomic touches the bitmap.  The
//                 tile's record and unit counts go to the tile's two words of
//                 scratch; bytes and dropped matches take one atomicAdd per
//                 wave that has any.  No LDS.
//   k_copy_scan : one workgroup turns the tile counts into exclusive prefixes in
//                 place and writes the totals.  A launch of its own: no look-back.
//   k_copy_emit : the same tiling.  A lane decides its block again; its record's
//                 place is the tile's prefix plus its rank among the wave's taken
//                 lanes (one ballot), its unit_first the tile's unit prefix plus
//                 a wave scan.  The table's order is the block order, whatever
//                 the timing.
// Every loop is bounded by an argument, none by data.
#include "copyblk.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

using ull = unsigned long long;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// (sources and destinations are global memory: accesses through an
// address-space-1 pointer are global_load / global_store, not flat)
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint16_t g_u16;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) uint64_t g_u64;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

constexpr uint32_t kCopyMaxGrid = 1u << 16;  // workgroups; the loop strides over the rest
constexpr uint32_t kPlanTile = 64;           // blocks per tile: one wave

__device__ __forceinline__ void copy_unit(const copyblk::Unit& t) {
  uint32_t w[4] = {0, 0, 0, 0};
  const g_u8* s = (const g_u8*)(uintptr_t)t.src;
  const uint32_t a = (uint32_t)t.src & 15u;
  if (t.n == 16 && a == 0) {
    const u32x4 v = *(const g_u32x4*)s;
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
  } else if (t.n == 16 && (a & 7u) == 0) {
    const g_u64* p = (const g_u64*)s;
    const uint64_t lo = p[0], hi = p[1];
    w[0] = (uint32_t)lo;
    w[1] = (uint32_t)(lo >> 32);
    w[2] = (uint32_t)hi;
    w[3] = (uint32_t)(hi >> 32);
  } else if (t.n == 16 && (a & 3u) == 0) {
    const g_u32* p = (const g_u32*)s;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = p[i];
  } else if (t.n == 16 && (a & 1u) == 0) {
    const g_u16* p = (const g_u16*)s;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i >> 1] |= (uint32_t)p[i] << (16 * (i & 1));
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((uint32_t)i < t.n) w[i >> 2] |= (uint32_t)s[i] << (8 * (i & 3));
  }
  g_u8* d = (g_u8*)(uintptr_t)t.dst;
  const uint32_t b = (uint32_t)t.dst & 15u;
  if (t.n == 16 && b == 0) {
    u32x4 v;
    v.x = w[0];
    v.y = w[1];
    v.z = w[2];
    v.w = w[3];
    *(g_u32x4*)d = v;
  } else if (t.n == 16 && (b & 7u) == 0) {
    g_u64* p = (g_u64*)d;
    p[0] = (uint64_t)w[0] | (uint64_t)w[1] << 32;
    p[1] = (uint64_t)w[2] | (uint64_t)w[3] << 32;
  } else if (t.n == 16 && (b & 3u) == 0) {
    g_u32* p = (g_u32*)d;
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = w[i];
  } else if (t.n == 16 && (b & 1u) == 0) {
    g_u16* p = (g_u16*)d;
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((uint32_t)i < t.n) d[i] = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
  }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor((ull)v, d, 64);
  return v;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void k_copy_runs(const uint64_t* __restrict__ runs,
                                                        uint64_t nruns, uint64_t nunits,
                                                        uint64_t lanes, ull* __restrict__ res) {
  uint32_t nbad = 0;  // (wave-uniform: ballot counts)
  const uint64_t step = (uint64_t)gridDim.x * kThreads;
#pragma unroll 1
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < lanes; base += step) {
    const uint64_t u = base + threadIdx.x;
    const bool bad = u < nruns && copyblk::run_bad(runs, nruns, nunits, u);
    const copyblk::Unit t = copyblk::unit_of(runs, nruns, nunits, u);
    if (t.n) copy_unit(t);
    nbad += (uint32_t)__popcll(__ballot(bad));
  }
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(res, (ull)nbad);
}

// tot: two words per tile {records, units}.  res[2..3] were zeroed on the same
// stream before the launch.
__global__ __launch_bounds__(kThreads) void k_copy_plan(copyblk::Plan p, uint64_t* __restrict__ have,
                                                        uint64_t* __restrict__ tot,
                                                        ull* __restrict__ res) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const copyblk::Take t = copyblk::take_of(p, g);  // (g >= n_need: nothing)
  const bool taken = t.flags & copyblk::kTaken;
  const uint64_t word = __ballot(taken), dropped = __ballot(t.flags & copyblk::kDropped);
  const uint64_t units = wave_sum(taken ? scatter::units(t.len) : 0);
  const uint64_t bytes = wave_sum(taken ? (uint64_t)t.len : 0);
  // (lane 0's g is the wave's first block, a multiple of 64)
  if ((threadIdx.x & 63) == 0 && g < p.n_need) {
    have[g >> 6] = word;
    tot[2 * (g >> 6)] = (uint64_t)__popcll(word);
    tot[2 * (g >> 6) + 1] = units;
    if (bytes) atomicAdd(&res[2], (ull)bytes);
    if (dropped) atomicAdd(&res[3], (ull)__popcll(dropped));
  }
}

__global__ __launch_bounds__(kThreads) void k_copy_scan(uint64_t* __restrict__ tot, uint64_t ntiles,
                                                        uint64_t* __restrict__ res) {
  __shared__ uint64_t part[2 * kThreads];
  const uint64_t per = (ntiles + kThreads - 1) / kThreads;
  const uint64_t lo = per * threadIdx.x < ntiles ? per * threadIdx.x : ntiles;
  const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
  uint64_t a = 0, b = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    a += tot[2 * i];
    b += tot[2 * i + 1];
  }
  part[2 * threadIdx.x] = a;
  part[2 * threadIdx.x + 1] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t ra = 0, rb = 0;
    for (int i = 0; i < kThreads; ++i) {
      const uint64_t xa = part[2 * i], xb = part[2 * i + 1];
      part[2 * i] = ra;
      part[2 * i + 1] = rb;
      ra += xa;
      rb += xb;
    }
    res[0] = ra;
    res[1] = rb;
  }
  __syncthreads();
  a = part[2 * threadIdx.x];
  b = part[2 * threadIdx.x + 1];
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t xa = tot[2 * i], xb = tot[2 * i + 1];
    tot[2 * i] = a;
    tot[2 * i + 1] = b;
    a += xa;
    b += xb;
  }
}

__global__ __launch_bounds__(kThreads) void k_copy_emit(copyblk::Plan p,
                                                        const uint64_t* __restrict__ tot,
                                                        uint64_t cap_runs,
                                                        uint64_t* __restrict__ runs) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const copyblk::Take t = copyblk::take_of(p, g);
  const bool taken = t.flags & copyblk::kTaken;
  const uint64_t word = __ballot(taken);
  const uint64_t mine = taken ? scatter::units(t.len) : 0;
  uint64_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up((ull)incl, d, 64);
    if (lane >= (uint32_t)d) incl += o;
  }
  if (!taken) return;  // (behind the wave's ballot and shuffles)
  const uint64_t rank = (uint64_t)__popcll(word & ((1ull << lane) - 1));
  const uint64_t r = tot[2 * (g >> 6)] + rank;
  if (r >= cap_runs) return;
  uint64_t* q = runs + copyblk::kRunWords * r;
  q[0] = tot[2 * (g >> 6) + 1] + incl - mine;
  q[1] = t.src;
  q[2] = t.dst;
  q[3] = t.len;
}

hipError_t launch_copy_runs(const uint64_t* runs, uint64_t nruns, uint64_t nunits, uint64_t* res,
                            hipStream_t s) {
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * kCopyResFields, s);
  const uint64_t lanes = scatter::lanes(nruns, nunits);
  if (e != hipSuccess || lanes == 0) return e;
  const uint64_t wgs = (lanes + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)(wgs < kCopyMaxGrid ? wgs : kCopyMaxGrid));
  hipLaunchKernelGGL(k_copy_runs, grid, dim3(kThreads), 0, s, runs, nruns, nunits, lanes,
                     reinterpret_cast<ull*>(res));
  return hipGetLastError();
}

hipError_t launch_copy_plan(const copyblk::Plan& p, uint64_t* have, uint64_t* runs,
                            uint64_t cap_runs, uint64_t* work, uint64_t* res, hipStream_t s) {
  static_assert(kThreads % kPlanTile == 0, "whole waves per workgroup: a wave owns one aligned word");
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * copyblk::kPlanResFields, s);
  if (e != hipSuccess || p.n_need == 0) return e;
  const dim3 grid((unsigned)((p.n_need + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_copy_plan, grid, dim3(kThreads), 0, s, p, have, work,
                     reinterpret_cast<ull*>(res));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_copy_scan, dim3(1), dim3(kThreads), 0, s, work, copy_plan_tiles(p.n_need),
                     res);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_copy_emit, grid, dim3(kThreads), 0, s, p, work, cap_runs, runs);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace cir
