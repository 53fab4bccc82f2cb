// The glue kernels of cir_fetch_plan (cir_plan_links_dev, cir_plan_want_dev):
// what stands between the four joins of a download plan, so that they run back
// to back in device memory.  The rule is plan.hpp; the reference has no
// counterpart (it plans nothing: scan_links, src/daemon/metadata/
// hardlink_sources.rs:107-153, then every remaining block is fetched,
// src/daemon/tracking/progress.rs:129-170).
//
//   k_plan_links : one lane per need file behind cir_match_files_dev's
//                  candidates: withdraws those that `deny` forbids and writes
//                  the skip bitmap of cir_match_copies_dev.
//   k_plan_want  : one lane per global block behind cir_match_copies_dev: the
//                  want bitmap of cir_match_extents_dev.
//
// Both follow k_block_bits' discipline (kernels.hip): kThreads is a multiple of
// the wave size, so a wave's first item is a multiple of 64 and the wave owns
// exactly one aligned word of the bitmap; its 64 verdicts are one ballot and
// lane 0 stores it with one vector store.  A wave whose first item is at or
// past n stores nothing, lanes at or past n vote 0, and every word of [0,
// ceil(n / 64)) is stored by its wave: nothing needs initialising, no atomic
// touches a bitmap, the bits at and past n are 0.  The counters take one
// atomicAdd per wave that has something to add, behind the launcher's memset of
// res on the same stream.  No LDS, no lane waits for another, and the only loop
// (plan::run_at's bisection) is bounded by n_runs.
#include "kernels.hpp"
#include "plan.hpp"

namespace cir {
namespace dev {

using ull = unsigned long long;

__global__ void k_plan_links(const uint64_t* __restrict__ deny, uint64_t n_files,
                             uint32_t* __restrict__ cand_src, uint64_t* __restrict__ cand_file,
                             uint64_t* __restrict__ skip, ull* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool skipped = false, kept = false, gone = false;
  if (i < n_files) {
    const uint32_t c = cand_src[i];
    skipped = plan::skip_bit(deny, i, c);
    gone = plan::withdrawn(deny, i, c);
    kept = c != plan::kNoSrc && !gone;
    if (gone) {
      cand_src[i] = plan::kNoSrc;
      cand_file[i] = plan::kNoFile;
    }
  }
  const uint64_t word = __ballot(skipped), nkept = __ballot(kept), ngone = __ballot(gone);
  // (lane 0's i is the wave's first file, a multiple of 64)
  if ((threadIdx.x & 63) == 0 && i < n_files) {
    skip[i >> 6] = word;
    if (nkept) atomicAdd(&res[0], (ull)__popcll(nkept));
    if (ngone) atomicAdd(&res[1], (ull)__popcll(ngone));
  }
}

__global__ void k_plan_want(const uint64_t* __restrict__ runs, uint64_t n_runs, uint64_t n_blocks,
                            uint64_t bs, uint64_t n_files, const uint32_t* __restrict__ cand_a,
                            const uint32_t* __restrict__ cand_b, const uint64_t* __restrict__ have,
                            uint64_t* __restrict__ want, ull* __restrict__ res) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  plan::Class c = plan::kOutside;
  if (g < n_blocks) c = plan::class_of(runs, n_runs, bs, n_files, cand_a, cand_b, have, g);
  const uint64_t word = __ballot(c == plan::kWanted);
  const uint64_t linked = __ballot(c == plan::kLinked), held = __ballot(c == plan::kHave);
  if ((threadIdx.x & 63) == 0 && g < n_blocks) {
    want[g >> 6] = word;
    if (word) atomicAdd(&res[0], (ull)__popcll(word));
    if (linked) atomicAdd(&res[1], (ull)__popcll(linked));
    if (held) atomicAdd(&res[2], (ull)__popcll(held));
  }
}

hipError_t launch_plan_links(const uint64_t* deny, uint64_t n_files, uint32_t* cand_src,
                             uint64_t* cand_file, uint64_t* skip, uint64_t* res, hipStream_t s) {
  static_assert(kThreads % 64 == 0, "whole waves per workgroup: a wave owns one aligned word");
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * plan::kLinksResFields, s);
  if (e != hipSuccess || n_files == 0) return e;
  const dim3 grid((unsigned)((n_files + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_plan_links, grid, dim3(kThreads), 0, s, deny, n_files, cand_src, cand_file,
                     skip, reinterpret_cast<ull*>(res));
  return hipGetLastError();
}

hipError_t launch_plan_want(const uint64_t* runs, uint64_t n_runs, uint64_t n_blocks, uint64_t bs,
                            uint64_t n_files, const uint32_t* cand_a, const uint32_t* cand_b,
                            const uint64_t* have, uint64_t* want, uint64_t* res, hipStream_t s) {
  static_assert(kThreads % 64 == 0, "whole waves per workgroup: a wave owns one aligned word");
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * plan::kWantResFields, s);
  if (e != hipSuccess || n_blocks == 0) return e;
  const dim3 grid((unsigned)((n_blocks + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_plan_want, grid, dim3(kThreads), 0, s, runs, n_runs, n_blocks, bs, n_files,
                     cand_a, cand_b, have, want, reinterpret_cast<ull*>(res));
  return hipGetLastError();
}

}  // namespace dev
}  // namespace cir
