// The plan kernels of cir_update_blocks: the two copy tables and the bitmap of
// an image updated in the buffers that hold it, made on the device from the
// join's answer.  The rule is update.hpp; the copies themselves are
// copyblk.hip's k_copy_runs, unchanged, launched once per table.  The
// reference has no counterpart (it holds no image in device memory).
//
//   k_update_plan : one lane per global block of the new index, a wave per tile
//                   of 64 blocks.  The lane decides its block's candidate class
//                   (update::classify: KEPT, DIRECT, STAGED or none; three
//                   bisections, two 16-byte loads per digest).  The tile's four
//                   words of scratch are {A records, A units, STAGED records,
//                   STAGED units}: DIRECT and STAGED both count into A.
//                   Dropped matches take one atomicAdd per wave that has any.
//                   No LDS.
//   k_update_scan : one workgroup, a launch of its own: the four columns become
//                   exclusive prefixes in place, and the candidates' totals go
//                   to res.  The demoted blocks are exactly the last STAGED
//                   candidates, so the final totals are DERIVED here from the
//                   candidate totals and the cap, not counted a second time:
//                   the one tile the cut runs through is decided again by the
//                   workgroup's first wave, which gives the count and the units
//                   of the staged blocks (table B's, the scratch's), and table
//                   A's are the candidates' minus the demoted ones'.  The host
//                   reads them after one synchronise and sizes the scratch.
//   k_update_emit : the same tiling as k_update_plan; a lane decides its block
//                   again.  A STAGED candidate's position is the tile's
//                   STAGED-unit prefix plus a wave scan of units; the cap makes
//                   it staged or demoted.  The have word is one ballot (KEPT,
//                   DIRECT or staged) that lane 0 stores with one vector store:
//                   every word of [0, ceil(n / 64)) is written, no atomic
//                   touches the bitmap.  Table A's record stands at the tile's A
//                   prefix plus the lane's rank, less the demoted blocks in
//                   front of it (those STAGED candidates in front of it beyond
//                   the scan's staged count), so demoted blocks leave no hole;
//                   table B's at the tile's STAGED prefix plus the lane's rank
//                   among the STAGED lanes.  Both tables are in block order
//                   whatever the timing.  Kept, direct, staged and demoted
//                   blocks and their bytes take one atomicAdd each per wave
//                   that has any.  No LDS.
// Every loop is bounded by an argument, none by data.
#include "kernels.hpp"
#include "update.hpp"

namespace cir {
namespace dev {

using ull = unsigned long long;

namespace {

constexpr uint32_t kTile = 64;  // blocks per tile: one wave
constexpr int kCols = 4;        // {A records, A units, STAGED records, STAGED units}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor((ull)v, d, 64);
  return v;
}

// the sum over the lanes below this one
__device__ __forceinline__ uint64_t wave_excl(uint64_t mine, uint32_t lane) {
  uint64_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up((ull)incl, d, 64);
    if (lane >= (uint32_t)d) incl += o;
  }
  return incl - mine;
}

}  // namespace

// tot: kCols words per tile.  res was zeroed on the same stream before the launch.
__global__ __launch_bounds__(kThreads) void k_update_plan(update::Plan p, uint64_t* __restrict__ tot,
                                                          ull* __restrict__ res) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const update::Cand k = update::classify(p, g);  // (g >= n_need: none)
  const bool staged = k.cls == update::kStaged, a = staged || k.cls == update::kDirect;
  const uint64_t aw = __ballot(a), sw = __ballot(staged), dw = __ballot(k.dropped);
  const uint64_t units = a ? scatter::units(k.len) : 0;
  const uint64_t au = wave_sum(units), su = wave_sum(staged ? units : 0);
  // (lane 0's g is the wave's first block, a multiple of 64)
  if ((threadIdx.x & 63) == 0 && g < p.c.n_need) {
    uint64_t* t = tot + kCols * (g >> 6);
    t[0] = (uint64_t)__popcll(aw);
    t[1] = au;
    t[2] = (uint64_t)__popcll(sw);
    t[3] = su;
    if (dw) atomicAdd(&res[update::kDroppedMatches], (ull)__popcll(dw));
  }
}

__global__ __launch_bounds__(kThreads) void k_update_scan(update::Plan p, uint64_t* __restrict__ tot,
                                                          uint64_t ntiles,
                                                          uint64_t* __restrict__ res) {
  __shared__ uint64_t part[kCols * kThreads];
  __shared__ uint64_t total[kCols];
  __shared__ ull cut;  // the first tile that does not fit whole, ~0: every one does
  const uint64_t per = (ntiles + kThreads - 1) / kThreads;
  const uint64_t lo = per * threadIdx.x < ntiles ? per * threadIdx.x : ntiles;
  const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
  uint64_t v[kCols] = {0, 0, 0, 0};
  for (uint64_t i = lo; i < hi; ++i)
#pragma unroll
    for (int c = 0; c < kCols; ++c) v[c] += tot[kCols * i + c];
#pragma unroll
  for (int c = 0; c < kCols; ++c) part[kCols * threadIdx.x + c] = v[c];
  if (threadIdx.x == 0) cut = ~0ull;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t run[kCols] = {0, 0, 0, 0};
    for (int i = 0; i < kThreads; ++i)
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
        const uint64_t x = part[kCols * i + c];
        part[kCols * i + c] = run[c];
        run[c] += x;
      }
#pragma unroll
    for (int c = 0; c < kCols; ++c) total[c] = run[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kCols; ++c) v[c] = part[kCols * threadIdx.x + c];
  uint64_t mine = ~0ull;
  for (uint64_t i = lo; i < hi; ++i) {
    // (the inclusive prefix never descends: the first tile past the cap is the cut)
    if (mine == ~0ull && tot[kCols * i + 2] && !update::fits(v[3], tot[kCols * i + 3], p.cap_units))
      mine = i;
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
      const uint64_t x = tot[kCols * i + c];
      tot[kCols * i + c] = v[c];
      v[c] += x;
    }
  }
  if (mine != ~0ull) atomicMin(&cut, (ull)mine);
  __syncthreads();  // (the prefixes written above are read below, by this workgroup)
  if (threadIdx.x >= kTile) return;
  // the staged blocks: every STAGED candidate in front of the cut tile, and
  // those of the cut tile that the cap still takes
  uint64_t b_recs = total[2], b_units = total[3];
  const uint64_t ct = cut;  // (uniform)
  if (ct != ~0ull) {
    const uint64_t r0 = tot[kCols * ct + 2], u0 = tot[kCols * ct + 3];
    const update::Cand k = update::classify(p, kTile * ct + threadIdx.x);
    const bool cand = k.cls == update::kStaged;
    const uint64_t units = cand ? scatter::units(k.len) : 0;
    const uint64_t pos = u0 + wave_excl(units, threadIdx.x);
    const bool in = cand && update::fits(pos, units, p.cap_units);
    b_recs = r0 + (uint64_t)__popcll(__ballot(in));
    b_units = u0 + wave_sum(in ? units : 0);
  }
  if (threadIdx.x == 0) {
    res[update::kCandARecs] = total[0];
    res[update::kCandAUnits] = total[1];
    res[update::kCandSRecs] = total[2];
    res[update::kCandSUnits] = total[3];
    res[update::kARecs] = total[0] - (total[2] - b_recs);
    res[update::kAUnits] = total[1] - (total[3] - b_units);
    res[update::kBRecs] = b_recs;
    res[update::kBUnits] = b_units;
  }
}

// tot: the prefixes; res: k_update_scan's totals are read, the class counts added.
__global__ __launch_bounds__(kThreads) void k_update_emit(update::Plan p,
                                                          const uint64_t* __restrict__ tot,
                                                          uint64_t cap_runs,
                                                          uint64_t* __restrict__ have,
                                                          uint64_t* __restrict__ runs_a,
                                                          uint64_t* __restrict__ runs_b,
                                                          ull* __restrict__ res) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const update::Cand k = update::classify(p, g);
  const bool cand = k.cls == update::kStaged, direct = k.cls == update::kDirect;
  const bool kept = k.cls == update::kKept;
  const uint64_t units = cand || direct ? scatter::units(k.len) : 0;
  const uint64_t tile = g >> 6;
  // (a wave wholly past the image has no tile; its lanes are all kNone)
  const bool live = (g & ~63ull) < p.c.n_need;
  const uint64_t a_rec0 = live ? tot[kCols * tile] : 0, a_unit0 = live ? tot[kCols * tile + 1] : 0;
  const uint64_t s_rec0 = live ? tot[kCols * tile + 2] : 0, s_unit0 = live ? tot[kCols * tile + 3] : 0;
  const uint64_t aw = __ballot(cand || direct), sw = __ballot(cand);
  const uint64_t below = (1ull << lane) - 1;
  const uint64_t a_rank = a_rec0 + (uint64_t)__popcll(aw & below);
  const uint64_t s_rank = s_rec0 + (uint64_t)__popcll(sw & below);
  const uint64_t a_first = a_unit0 + wave_excl(units, lane);
  const uint64_t s_first = s_unit0 + wave_excl(cand ? units : 0, lane);
  const bool staged = cand && update::fits(s_first, units, p.cap_units);
  const bool demoted = cand && !staged;
  const uint64_t word = __ballot(kept || direct || staged);
  const uint64_t kw = __ballot(kept), dw = __ballot(direct), mw = __ballot(demoted);
  const uint64_t kept_b = wave_sum(kept ? (uint64_t)k.len : 0);
  const uint64_t direct_b = wave_sum(direct ? (uint64_t)k.len : 0);
  const uint64_t staged_b = wave_sum(staged ? (uint64_t)k.len : 0);
  const uint64_t demoted_b = wave_sum(demoted ? (uint64_t)k.len : 0);
  if (lane == 0 && live) {
    have[tile] = word;
    if (kw) {
      atomicAdd(&res[update::kKeptBlocks], (ull)__popcll(kw));
      atomicAdd(&res[update::kKeptBytes], (ull)kept_b);
    }
    if (dw) {
      atomicAdd(&res[update::kDirectBlocks], (ull)__popcll(dw));
      atomicAdd(&res[update::kDirectBytes], (ull)direct_b);
    }
    if (staged_b) atomicAdd(&res[update::kStagedBytes], (ull)staged_b);
    if (mw) {
      atomicAdd(&res[update::kDemotedBlocks], (ull)__popcll(mw));
      atomicAdd(&res[update::kDemotedBytes], (ull)demoted_b);
    }
  }
  if (!direct && !staged) return;  // (behind the wave's ballots and shuffles)
  // the staged blocks are the first res[kBRecs] STAGED candidates with the
  // first res[kBUnits] units: what lies in front of this block beyond them is demoted
  const uint64_t b_recs = res[update::kBRecs], b_units = res[update::kBUnits];
  const uint64_t ra = a_rank - (s_rank - (s_rank < b_recs ? s_rank : b_recs));
  const uint64_t ua = a_first - (s_first - (s_first < b_units ? s_first : b_units));
  const uint64_t at = p.scratch + 16 * s_first;
  if (ra < cap_runs) {
    uint64_t* q = runs_a + copyblk::kRunWords * ra;
    q[0] = ua;
    q[1] = k.src;
    q[2] = staged ? at : k.dst;
    q[3] = k.len;
  }
  if (staged && s_rank < cap_runs) {
    uint64_t* q = runs_b + copyblk::kRunWords * s_rank;
    q[0] = s_first;
    q[1] = at;
    q[2] = k.dst;
    q[3] = k.len;
  }
}

hipError_t launch_update_count(const update::Plan& p, uint64_t* work, uint64_t* res, hipStream_t s) {
  static_assert(kThreads % kTile == 0, "whole waves per workgroup: a wave owns one aligned word");
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * update::kResFields, s);
  if (e != hipSuccess || p.c.n_need == 0) return e;
  const dim3 grid((unsigned)((p.c.n_need + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_update_plan, grid, dim3(kThreads), 0, s, p, work,
                     reinterpret_cast<ull*>(res));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_update_scan, dim3(1), dim3(kThreads), 0, s, p, work,
                     update_plan_tiles(p.c.n_need), res);
  return hipGetLastError();
}

hipError_t launch_update_emit(const update::Plan& p, const uint64_t* work, uint64_t cap_runs,
                              uint64_t* have, uint64_t* runs_a, uint64_t* runs_b, uint64_t* res,
                              hipStream_t s) {
  if (p.c.n_need == 0) return hipSuccess;
  const dim3 grid((unsigned)((p.c.n_need + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_update_emit, grid, dim3(kThreads), 0, s, p, work, cap_runs, have, runs_a,
                     runs_b, reinterpret_cast<ull*>(res));
  return hipGetLastError();
}

}  // namespace dev
}  // namespace cir
