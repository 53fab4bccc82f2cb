// A DIRSIGNATURE.v1 index's block digests, parsed on the device
// (cir_index_digests_dev): index text in, the digests as one flat list and a
// run record per non-empty file out.
//
// Every consumer of an index used to get its digests from dirsig::parse on
// the host -- one std::string per line, one vector per hash -- although 65 of
// every ~65.1 bytes of a large index are " " + 64 hex digits at a fixed
// stride behind a short head.  The rule which lines the device takes (a
// canonical subset of the host parser's; everything else is declined and left
// to the host) is idxscan.hpp, shared with the host and fuzzed there.
//
// Count, scan, emit, decode -- four launches on the caller's stream, and no
// workgroup ever waits for another:
//   k_idx_count   a workgroup per tile of kIdxTile bytes of text, 16 bytes per
//                 lane.  A lane that finds a '\n' inside the body owns the
//                 line behind it (the lane whose span holds body_off owns the
//                 first line), parses its head and adds (file entries,
//                 non-empty files, blocks) to its tile's totals; a declined
//                 line does atomicMin of its start into res[4].
//   k_idx_scan    one workgroup turns the tile totals into exclusive prefixes
//                 in place and writes the totals and the status.  A launch of
//                 its own on purpose: no look-back, no spin.
//   k_idx_emit    the same walk again (heads are short), an in-workgroup
//                 exclusive scan in byte order, and every non-empty file line
//                 writes its run record {first, size, file, hash_off} at its
//                 scanned ordinal.
//   k_idx_decode  balanced per block, not per line (a 1 GiB file is one 2 MB
//                 line): four lanes per digest.  Block g finds its run by
//                 bisecting the run table (sources::run_of's loop); lane j of
//                 the four loads the 16 hex digits at hash_off + 65 (g -
//                 first) + 1 + 16 j -- any alignment -- checks them (lane 0
//                 the separator too) and stores 8 bytes at digests + 32 g +
//                 8 j.  A bad token declines its line.
// Four lanes per digest: a lane's work is then one 16-byte load (one
// global_load_dwordx4 at byte alignment in the built code object) and one
// 8-byte store, a wave reads 16 x 65 contiguous bytes and stores 512
// contiguous bytes, and the 64 hexval steps of a token are spread over four
// lanes instead of serialised in one; one lane per digest would need 17
// loads at a 65-byte stride per lane and a 32-byte store per lane at a stride
// no store instruction coalesces.
//
// emit and decode do nothing unless the status the scan wrote is OK, so a
// declined or over-capacity index costs one pass over its text.  When nothing
// is declined no atomic is issued.
#include "idxscan.hpp"
#include "idxwalk.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

namespace {

constexpr uint32_t kScanPer = 8;  // tiles per lane and step of k_idx_scan

__device__ __forceinline__ void decline_line(uint64_t* res, uint64_t line) {
  atomicMin(reinterpret_cast<unsigned long long*>(res + 4), (unsigned long long)line);
}

// What the lane's lines add: file entries, non-empty files, blocks.
__device__ __forceinline__ Pair lane_counts(const uint8_t* __restrict__ text, uint64_t len,
                                            uint64_t s, uint64_t body_off, uint64_t body_end,
                                            uint64_t bs, uint64_t* res) {
  Pair c = {0, 0};
  walk_span(text, len, s, body_off, body_end, [&](uint64_t p) {
    const Head h = head_at(text, p, body_off, body_end, bs);
    if (h.kind == idxscan::kDecline) {
      if (res) decline_line(res, p);
    } else if (h.kind == idxscan::kFile) {
      c.fr += 1 + (h.nblk ? 1ull << 32 : 0);
      c.blk += h.nblk;
    }
  });
  return c;
}

}  // namespace

// tot[3 t .. 3 t + 3) = (file entries, non-empty files, blocks) of the lines
// tile tile0 + t owns.
__global__ __launch_bounds__(kThreads) void k_idx_count(const uint8_t* __restrict__ text,
                                                        uint64_t len, uint64_t body_off,
                                                        uint64_t body_end, uint64_t bs,
                                                        uint64_t tile0, uint64_t* __restrict__ tot,
                                                        uint64_t* __restrict__ res) {
  __shared__ Pair lds[kThreads / 64 + 1];
  const uint64_t s = (tile0 + blockIdx.x) * kIdxTile + threadIdx.x * kSpan;
  const Pair c = lane_counts(text, len, s, body_off, body_end, bs, res);
  Pair sum;
  (void)block_excl_scan(c, &sum, lds);
  if (threadIdx.x == 0) {
    uint64_t* o = tot + 3 * (uint64_t)blockIdx.x;
    o[0] = sum.fr & 0xFFFFFFFFu;
    o[1] = sum.fr >> 32;
    o[2] = sum.blk;
  }
}

// One workgroup: tot[3 t ..] becomes the exclusive prefix over the tiles
// before t; res[1..3] = the totals; res[0] = the status so far (a bad token
// found by k_idx_decode raises it to DECLINED later); tot[3 ntiles] = the same
// status, which no later kernel changes.
__global__ __launch_bounds__(kThreads) void k_idx_scan(uint64_t* __restrict__ tot, uint64_t ntiles,
                                                       uint64_t cap_blocks, uint64_t cap_runs,
                                                       uint64_t* __restrict__ res) {
  __shared__ Pair lds[kThreads / 64 + 1];
  uint64_t cf = 0, cr = 0, cb = 0;  // the carry: the same in every lane
  for (uint64_t base = 0; base < ntiles; base += (uint64_t)kThreads * kScanPer) {
    const uint64_t i0 = base + (uint64_t)threadIdx.x * kScanPer;
    uint64_t f[kScanPer], r[kScanPer], b[kScanPer];
    Pair mine = {0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      const bool in = i0 + k < ntiles;
      f[k] = in ? tot[3 * (i0 + k)] : 0;
      r[k] = in ? tot[3 * (i0 + k) + 1] : 0;
      b[k] = in ? tot[3 * (i0 + k) + 2] : 0;
      mine.fr += f[k] + (r[k] << 32);  // (a step holds < 2^32 of either: 2048 tiles of 4 KiB)
      mine.blk += b[k];
    }
    Pair sum;
    const Pair ex = block_excl_scan(mine, &sum, lds);
    uint64_t pf = cf + (ex.fr & 0xFFFFFFFFu), pr = cr + (ex.fr >> 32), pb = cb + ex.blk;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      if (i0 + k < ntiles) {
        tot[3 * (i0 + k)] = pf;
        tot[3 * (i0 + k) + 1] = pr;
        tot[3 * (i0 + k) + 2] = pb;
      }
      pf += f[k];
      pr += r[k];
      pb += b[k];
    }
    cf += sum.fr & 0xFFFFFFFFu;
    cr += sum.fr >> 32;
    cb += sum.blk;
  }
  if (threadIdx.x == 0) {
    res[1] = cf;
    res[2] = cr;
    res[3] = cb;
    const uint64_t st = res[4] != ~0ull ? kIdxDeclined
                                        : (cb > cap_blocks || cr > cap_runs) ? kIdxCapacity : kIdxOk;
    res[0] = st;
    tot[3 * ntiles] = st;  // the gate of emit and decode: res[0] may still rise, this word not
  }
}

// runs[4 r .. 4 r + 4) = {first, size, file, hash_off} of the r-th non-empty
// file.  Nothing unless the scan's status (*gate) is OK (then r < cap_runs
// holds for every r).
__global__ __launch_bounds__(kThreads) void k_idx_emit(const uint8_t* __restrict__ text,
                                                       uint64_t len, uint64_t body_off,
                                                       uint64_t body_end, uint64_t bs,
                                                       uint64_t tile0,
                                                       const uint64_t* __restrict__ tot,
                                                       uint64_t* __restrict__ runs,
                                                       uint64_t cap_runs,
                                                       const uint64_t* __restrict__ gate) {
  __shared__ Pair lds[kThreads / 64 + 1];
  if (*gate != kIdxOk) return;  // (uniform: every lane reads the same word)
  const uint64_t s = (tile0 + blockIdx.x) * kIdxTile + threadIdx.x * kSpan;
  const Pair c = lane_counts(text, len, s, body_off, body_end, bs, nullptr);
  Pair sum;
  const Pair ex = block_excl_scan(c, &sum, lds);
  if ((c.fr >> 32) == 0) return;  // no run starts in this lane's span
  const uint64_t* t = tot + 3 * (uint64_t)blockIdx.x;
  uint64_t file = t[0] + (ex.fr & 0xFFFFFFFFu), run = t[1] + (ex.fr >> 32), blk = t[2] + ex.blk;
  walk_span(text, len, s, body_off, body_end, [&](uint64_t p) {
    const Head h = head_at(text, p, body_off, body_end, bs);
    if (h.kind != idxscan::kFile) return;
    if (h.nblk) {
      if (run < cap_runs) {
        uint64_t* o = runs + 4 * run;
        o[0] = blk;
        o[1] = h.size;
        o[2] = file;
        o[3] = h.hash_off;
      }
      ++run;
      blk += h.nblk;
    }
    ++file;
  });
}

// Four lanes per block: digests[32 g + 8 j ..] = the 16 hex digits j of block
// g's token.  Nothing unless the scan's status (*gate) is OK (then res[3] <=
// cap_blocks and res[2] <= cap_runs, the runs' `first` ascend from 0 and every
// token the heads promised lies inside the body).  Every workgroup decodes all
// of its tokens whatever the others found, so res[4] ends as the first bad
// line's start.
__global__ __launch_bounds__(kThreads) void k_idx_decode(const uint8_t* __restrict__ text,
                                                         uint64_t body_off, uint64_t body_end,
                                                         const uint64_t* __restrict__ runs,
                                                         uint8_t* __restrict__ digests,
                                                         const uint64_t* __restrict__ gate,
                                                         uint64_t* __restrict__ res) {
  if (*gate != kIdxOk) return;
  const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t g = gid >> 2;
  const uint32_t j = (uint32_t)gid & 3;
  if (g >= res[3]) return;
  uint64_t lo = 0, hi = res[2];  // invariant: runs[lo].first <= g < runs[hi].first
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (runs[4 * mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t first = runs[4 * lo], hash_off = runs[4 * lo + 3];
  const uint64_t k = g - first;
  // (what the head promised, checked again: no load leaves the body)
  if (hash_off >= body_end || k >= (body_end - hash_off) / idxscan::kTokenBytes) return;
  const uint8_t* tok = text + hash_off + idxscan::kTokenBytes * k;
  uint32_t w[4], o[2];
  __builtin_memcpy(w, tok + 1 + 16 * j, 16);
  bool ok = idxscan::hex16(w, o);
  if (j == 0) ok = ok && tok[0] == ' ';
  *reinterpret_cast<uint2*>(digests + 32 * g + 8 * j) = make_uint2(o[0], o[1]);
  if (!ok) {
    uint64_t p = hash_off;  // back to the line's start: a head is at most kMaxHead bytes
    while (p > body_off && text[p - 1] != '\n') --p;
    decline_line(res, p);
    atomicMax(reinterpret_cast<unsigned long long*>(res), (unsigned long long)kIdxDeclined);
  }
}

// The text's tiles: the first one and how many hold a byte of the body.
static inline void idx_tiles(uint64_t body_off, uint64_t body_end, uint64_t* tile0,
                             uint64_t* ntiles) {
  *tile0 = body_off / kIdxTile;
  *ntiles = body_end > body_off ? (body_end + kIdxTile - 1) / kIdxTile - *tile0 : 0;
}

hipError_t launch_index_count(const uint8_t* text, uint64_t len, uint64_t body_off,
                              uint64_t body_end, uint64_t bs, uint64_t cap_blocks,
                              uint64_t cap_runs, uint64_t* work, uint64_t* res, hipStream_t s) {
  hipError_t e = hipMemsetAsync(res, 0xFF, kIdxResFields * sizeof(uint64_t), s);
  if (e != hipSuccess) return e;
  uint64_t tile0, ntiles;
  idx_tiles(body_off, body_end, &tile0, &ntiles);
  if (ntiles) {
    hipLaunchKernelGGL(k_idx_count, dim3((unsigned)ntiles), dim3(kThreads), 0, s, text, len,
                       body_off, body_end, bs, tile0, work, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_idx_scan, dim3(1), dim3(kThreads), 0, s, work, ntiles, cap_blocks,
                     cap_runs, res);
  return hipGetLastError();
}

hipError_t launch_index_emit(const uint8_t* text, uint64_t len, uint64_t body_off,
                             uint64_t body_end, uint64_t bs, uint8_t* digests, uint64_t max_blocks,
                             uint64_t* runs, uint64_t cap_runs, uint64_t* work, uint64_t* res,
                             hipStream_t s) {
  uint64_t tile0, ntiles;
  idx_tiles(body_off, body_end, &tile0, &ntiles);
  if (ntiles == 0 || max_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_idx_emit, dim3((unsigned)ntiles), dim3(kThreads), 0, s, text, len,
                     body_off, body_end, bs, tile0, work, runs, cap_runs, work + 3 * ntiles);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_idx_decode, dim3((unsigned)((4 * max_blocks + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, text, body_off, body_end, runs, digests,
                     work + 3 * ntiles, res);
  return hipGetLastError();
}

hipError_t launch_index_digests(const uint8_t* text, uint64_t len, uint64_t body_off,
                                uint64_t body_end, uint64_t bs, uint8_t* digests,
                                uint64_t cap_blocks, uint64_t* runs, uint64_t cap_runs,
                                uint64_t* work, uint64_t* res, hipStream_t s) {
  hipError_t e = launch_index_count(text, len, body_off, body_end, bs, cap_blocks, cap_runs, work,
                                    res, s);
  if (e != hipSuccess) return e;
  // the blocks the body can hold, whatever the count pass finds
  uint64_t maxblk = (body_end - body_off) / idxscan::kTokenBytes;
  if (maxblk > cap_blocks) maxblk = cap_blocks;
  return launch_index_emit(text, len, body_off, body_end, bs, digests, maxblk, runs, cap_runs,
                           work, res, s);
}

}  // namespace dev
}  // namespace cir
