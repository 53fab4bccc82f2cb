// The kernel of cir_gather_runs_dev and of cir_store_blocks' batches: bytes
// that lie anywhere in device memory copied into the packed runs of a staging
// slot.  The rule is gather.hpp; the reference has no counterpart (what it
// writes to an image directory arrives block by block from the network,
// src/daemon/disk/public.rs write_block).
//
//   k_gather_runs : one lane per 16-byte unit of the table.  The lane bisects
//                   the table by unit_first (scatter::run_at, at most 32 steps,
//                   bounded by the record count), looks at its record
//                   (gather::run_bad) and, if the record is sound, loads its n
//                   source bytes: a whole unit with one dwordx4 load when the
//                   source is 16-byte aligned, else with the widest loads the
//                   source's alignment allows (8, 4, 2 bytes or single bytes:
//                   k_scatter_runs' store ladder turned round; the compiler may
//                   fuse those of a 4- or 8-byte aligned unit into one dwordx4
//                   load again, which the hardware takes at dword alignment);
//                   a short last unit loads its own n bytes one by one, so
//                   nothing is read outside [src, src + bytes).  It always
//                   stores all 16 bytes of its unit -- the bytes, then zeros --
//                   with one dwordx4 store: the slot is 16-byte aligned and a
//                   run starts on a multiple of 16.  Lane r also looks at
//                   record r and counts it when it is bad: one atomicAdd per
//                   wave that met any, behind the launcher's memset on the same
//                   stream.
//
// No LDS, no scratch, no lane waits for another; the wave's count is one ballot
// that every lane of the wave reaches.
#include "gather.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

using ull = unsigned long long;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// (the sources are global memory: loads through an address-space-1 pointer are
// global_load, not flat_load)
typedef const __attribute__((address_space(1))) uint8_t g_u8;
typedef const __attribute__((address_space(1))) uint16_t g_u16;
typedef const __attribute__((address_space(1))) uint32_t g_u32;
typedef const __attribute__((address_space(1))) uint64_t g_u64;
typedef const __attribute__((address_space(1))) u32x4 g_u32x4;

}  // namespace

__global__ void k_gather_runs(uint8_t* __restrict__ dst, uint64_t dst_bytes,
                              const uint64_t* __restrict__ runs, uint64_t nruns, uint64_t nunits,
                              ull* __restrict__ res) {
  const uint64_t u = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool bad = u < nruns && gather::run_bad(runs, nruns, nunits, dst_bytes, u);
  const gather::Unit t = gather::unit_of(runs, nruns, nunits, dst_bytes, u);
  if (t.n) {
    uint32_t w[4] = {0, 0, 0, 0};
    g_u8* s = (g_u8*)(uintptr_t)t.src;
    const uint32_t a = (uint32_t)t.src & 15u;
    if (t.n == 16 && a == 0) {
      const u32x4 v = *(g_u32x4*)s;
      w[0] = v.x;
      w[1] = v.y;
      w[2] = v.z;
      w[3] = v.w;
    } else if (t.n == 16 && (a & 7u) == 0) {
      g_u64* p = (g_u64*)s;
      const uint64_t lo = p[0], hi = p[1];
      w[0] = (uint32_t)lo;
      w[1] = (uint32_t)(lo >> 32);
      w[2] = (uint32_t)hi;
      w[3] = (uint32_t)(hi >> 32);
    } else if (t.n == 16 && (a & 3u) == 0) {
      g_u32* p = (g_u32*)s;
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = p[i];
    } else if (t.n == 16 && (a & 1u) == 0) {
      g_u16* p = (g_u16*)s;
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i >> 1] |= (uint32_t)p[i] << (16 * (i & 1));
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((uint32_t)i < t.n) w[i >> 2] |= (uint32_t)s[i] << (8 * (i & 3));
    }
    u32x4 v;
    v.x = w[0];
    v.y = w[1];
    v.z = w[2];
    v.w = w[3];
    *reinterpret_cast<u32x4*>(dst + t.dst_off) = v;
  }
  const uint32_t sum = (uint32_t)__popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(res, (ull)sum);
}

hipError_t launch_gather_runs(uint8_t* dst, uint64_t dst_bytes, const uint64_t* runs,
                              uint64_t nruns, uint64_t nunits, uint64_t* res, hipStream_t s) {
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * kGatherResFields, s);
  const uint64_t lanes = scatter::lanes(nruns, nunits);
  if (e != hipSuccess || lanes == 0) return e;
  const dim3 grid((unsigned)((lanes + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_gather_runs, grid, dim3(kThreads), 0, s, dst, dst_bytes, runs, nruns,
                     nunits, reinterpret_cast<ull*>(res));
  return hipGetLastError();
}

}  // namespace dev
}  // namespace cir
