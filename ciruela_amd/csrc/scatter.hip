// The kernel of cir_scatter_runs_dev and of cir_load_blocks' batches: the packed
// runs of a staging slot copied to their places in the caller's buffers.  The
// rule is scatter.hpp; the reference has no counterpart (its consumers read
// committed files from disk, src/daemon/disk/commit.rs:51-117).
//
//   k_scatter_runs : one lane per 16-byte unit of the table.  The lane bisects
//                    the table by unit_first (scatter::run_at, at most 32 steps,
//                    bounded by the record count), looks at its record
//                    (scatter::run_bad) and, if the record is sound, loads its
//                    16 bytes from the slot with one dwordx4 load -- the slot is
//                    16-byte aligned and a run starts on a multiple of 16; a
//                    unit whose 16 bytes would reach past src_bytes loads its
//                    bytes one by one -- and stores only its own n bytes: one
//                    dwordx4 store when n == 16 and the destination is 16-byte
//                    aligned, else narrower stores by the destination's
//                    alignment (8, 4, 2 bytes or single bytes; the compiler
//                    fuses those of a 2-, 4- or 8-byte aligned whole unit into
//                    one dwordx4 store again, which the hardware takes at any
//                    dword-or-smaller alignment; an odd destination and a
//                    short last unit store bytes).  Lane r
//                    also looks at record r and counts it when it is bad: one
//                    atomicAdd per wave that met any, behind the launcher's
//                    memset on the same stream.
//
// No LDS, no scratch, no lane waits for another; the wave's count is one ballot
// that every lane of the wave reaches.
#include "kernels.hpp"
#include "scatter.hpp"

namespace cir {
namespace dev {

using ull = unsigned long long;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint16_t g_u16;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) uint64_t g_u64;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

// byte i (0 .. 15) of the unit in w
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], int i) {
  return (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
}

}  // namespace

__global__ void k_scatter_runs(const uint8_t* __restrict__ src, uint64_t src_bytes,
                               const uint64_t* __restrict__ runs, uint64_t nruns, uint64_t nunits,
                               ull* __restrict__ res) {
  const uint64_t u = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool bad = u < nruns && scatter::run_bad(runs, nruns, nunits, src_bytes, u);
  const scatter::Unit t = scatter::unit_of(runs, nruns, nunits, src_bytes, u);
  if (t.n) {
    uint32_t w[4] = {0, 0, 0, 0};
    const uint8_t* s = src + t.src_off;
    if (t.src_off + 16 <= src_bytes) {
      const uint4 v = *reinterpret_cast<const uint4*>(s);
      w[0] = v.x;
      w[1] = v.y;
      w[2] = v.z;
      w[3] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((uint32_t)i < t.n) w[i >> 2] |= (uint32_t)s[i] << (8 * (i & 3));
    }
    // (the destination is global memory: stores through an address-space-1
    // pointer are global_store, not flat_store)
    g_u8* d = (g_u8*)(uintptr_t)t.dst;
    const uint32_t a = (uint32_t)t.dst & 15u;
    if (t.n == 16 && a == 0) {
      u32x4 v;
      v.x = w[0];
      v.y = w[1];
      v.z = w[2];
      v.w = w[3];
      *(g_u32x4*)d = v;
    } else if (t.n == 16 && (a & 7u) == 0) {
      g_u64* p = (g_u64*)d;
      p[0] = (uint64_t)w[0] | (uint64_t)w[1] << 32;
      p[1] = (uint64_t)w[2] | (uint64_t)w[3] << 32;
    } else if (t.n == 16 && (a & 3u) == 0) {
      g_u32* p = (g_u32*)d;
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = w[i];
    } else if (t.n == 16 && (a & 1u) == 0) {
      g_u16* p = (g_u16*)d;
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((uint32_t)i < t.n) d[i] = (uint8_t)byte_of(w, i);
    }
  }
  const uint32_t sum = (uint32_t)__popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(res, (ull)sum);
}

hipError_t launch_scatter_runs(const uint8_t* src, uint64_t src_bytes, const uint64_t* runs,
                               uint64_t nruns, uint64_t nunits, uint64_t* res, hipStream_t s) {
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * kScatterResFields, s);
  const uint64_t lanes = scatter::lanes(nruns, nunits);
  if (e != hipSuccess || lanes == 0) return e;
  const dim3 grid((unsigned)((lanes + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_scatter_runs, grid, dim3(kThreads), 0, s, src, src_bytes, runs, nruns,
                     nunits, reinterpret_cast<ull*>(res));
  return hipGetLastError();
}

}  // namespace dev
}  // namespace cir
