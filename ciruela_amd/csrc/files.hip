// The file entries of an index on the device (cir_index_files_dev) and the
// join of two file lists (cir_match_files_dev, the device half of
// cir_file_sources): which files of a new image an older image lists at the
// same path with the same exe flag, size and digests.
//
// Reference: scan_links (src/daemon/metadata/hardlink_sources.rs:107-153)
// walks the merged indexes on one host thread.  The rule -- records, path
// decoding, path hash, fold term -- is files.hpp, shared with the host and
// fuzzed there; the walk over the text is idxwalk.hpp, shared with
// idxscan.hip.
//
// cir_index_files_dev: count, scan, emit and a token check on the caller's
// stream, and no workgroup ever waits for another:
//   k_files_count  a workgroup per tile of kIdxTile bytes, 16 bytes per lane,
//                  as k_idx_count: the tile's file entries and blocks, and the
//                  start of the last directory line it owns (+ 1; 0: none).
//   k_files_scan   one workgroup: exclusive prefixes of the counts, and for
//                  every tile the last directory line before it (a running
//                  maximum: line starts ascend with the tiles); the totals and
//                  the status.
//   k_files_emit   the same walk, exclusive scans in byte order inside the
//                  workgroup, and every file line writes its record at its
//                  ordinal with the last directory line at or before it, from
//                  its own tile or from the carry.
//   k_files_tokens four lanes per block check the hash tokens' digits, so that
//                  the status is cir_index_digests_dev's on every text (skipped
//                  by cir_file_sources, which runs that call's decode pass).
//
// cir_match_files_dev: one memset of the scratch (folds and table), then
//   k_files_fold   (need, pool) one lane per block: the block's fold term,
//                  summed inside the wave over the lanes that share a file,
//                  one atomicAdd per (wave, file, word);
//   k_files_build  one lane per pool file into an open-addressing table of
//                  pool ordinals + 1 keyed by (source, decoded path): CAS on
//                  empty, atomicMin on equal, as join.hip;
//   k_files_probe  one lane per need file: the sources in order;
//   k_files_verify one lane per need block of a file with a candidate.
//
// cir_match_copies_dev (the device half of cir_file_copies; the rule and the
// argument for it are copies.hpp): the same memset, k_files_fold for both
// sides and k_files_verify, with a table keyed by content between them:
//   k_copies_build one lane per non-empty pool file into a table of pool
//                  ordinals + 1 keyed by {size, exe, fold}: CAS on empty,
//                  atomicMin on an equal key;
//   k_copies_probe one lane per need file that is neither empty nor skipped:
//                  from the key's home slot to an equal key or an empty slot.
#include "copies.hpp"
#include "files.hpp"
#include "idxwalk.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

namespace {

constexpr uint32_t kFilesScanPer = 8;  // tiles per lane and step of k_files_scan
constexpr uint32_t kTileWords = 4;     // {file entries, blocks, last directory line + 1, unused}

struct LaneCounts {
  Pair c;           // fr = file entries, blk = blocks
  uint64_t dir1;    // start of the lane's last directory line + 1; 0: none
};

__device__ __forceinline__ LaneCounts files_lane_counts(const uint8_t* __restrict__ text,
                                                        uint64_t len, uint64_t s, uint64_t body_off,
                                                        uint64_t body_end, uint64_t bs,
                                                        uint64_t* res) {
  LaneCounts l = {{0, 0}, 0};
  walk_span(text, len, s, body_off, body_end, [&](uint64_t p) {
    const Head h = head_at(text, p, body_off, body_end, bs);
    if (h.kind == idxscan::kDecline) {
      if (res) atomicMin(reinterpret_cast<unsigned long long*>(res + 3), (unsigned long long)p);
    } else if (h.kind == idxscan::kFile) {
      l.c.fr += 1;
      l.c.blk += h.nblk;
    } else if (h.kind == idxscan::kDir) {
      l.dir1 = p + 1;
    }
  });
  return l;
}

// Exclusive running maximum of v over the workgroup in thread order; *total =
// the maximum.  lds: kThreads / 64 entries.  Safe to call in a loop.
__device__ __forceinline__ uint64_t block_excl_max(uint64_t v, uint64_t* total, uint64_t* lds) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t a = __shfl_up((unsigned long long)inc, d, 64);
    if ((int)lane >= d && a > inc) inc = a;
  }
  uint64_t ex = __shfl_up((unsigned long long)inc, 1, 64);
  if (lane == 0) ex = 0;
  __syncthreads();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint64_t all = 0;
#pragma unroll
  for (uint32_t k = 0; k < kThreads / 64; ++k) {
    const uint64_t t = lds[k];
    if (k < wave && t > ex) ex = t;
    if (t > all) all = t;
  }
  *total = all;
  return ex;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void k_files_count(const uint8_t* __restrict__ text,
                                                          uint64_t len, uint64_t body_off,
                                                          uint64_t body_end, uint64_t bs,
                                                          uint64_t tile0, uint64_t* __restrict__ tot,
                                                          uint64_t* __restrict__ res) {
  __shared__ Pair lds[kThreads / 64 + 1];
  __shared__ uint64_t mlds[kThreads / 64];
  const uint64_t s = (tile0 + blockIdx.x) * kIdxTile + threadIdx.x * kSpan;
  const LaneCounts l = files_lane_counts(text, len, s, body_off, body_end, bs, res);
  Pair sum;
  uint64_t dmax;
  (void)block_excl_scan(l.c, &sum, lds);
  (void)block_excl_max(l.dir1, &dmax, mlds);
  if (threadIdx.x == 0) {
    uint64_t* o = tot + kTileWords * (uint64_t)blockIdx.x;
    o[0] = sum.fr;
    o[1] = sum.blk;
    o[2] = dmax;
    o[3] = 0;
  }
}

// One workgroup: tot[4 t ..] becomes {file entries before t, blocks before t,
// last directory line before t + 1}; res[1..2] = the totals; res[0] = the
// status; tot[4 ntiles] = the same status, the gate of the emit pass.
__global__ __launch_bounds__(kThreads) void k_files_scan(uint64_t* __restrict__ tot,
                                                         uint64_t ntiles, uint64_t cap_files,
                                                         uint64_t* __restrict__ res) {
  __shared__ Pair lds[kThreads / 64 + 1];
  __shared__ uint64_t mlds[kThreads / 64];
  uint64_t cf = 0, cb = 0, cd = 0;  // the carry: the same in every lane
  for (uint64_t base = 0; base < ntiles; base += (uint64_t)kThreads * kFilesScanPer) {
    const uint64_t i0 = base + (uint64_t)threadIdx.x * kFilesScanPer;
    uint64_t f[kFilesScanPer], b[kFilesScanPer], d[kFilesScanPer];
    Pair mine = {0, 0};
    uint64_t dmine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFilesScanPer; ++k) {
      const bool in = i0 + k < ntiles;
      f[k] = in ? tot[kTileWords * (i0 + k)] : 0;
      b[k] = in ? tot[kTileWords * (i0 + k) + 1] : 0;
      d[k] = in ? tot[kTileWords * (i0 + k) + 2] : 0;
      mine.fr += f[k];
      mine.blk += b[k];
      if (d[k] > dmine) dmine = d[k];
    }
    Pair sum;
    uint64_t dsum;
    const Pair ex = block_excl_scan(mine, &sum, lds);
    const uint64_t dex = block_excl_max(dmine, &dsum, mlds);
    uint64_t pf = cf + ex.fr, pb = cb + ex.blk, pd = dex > cd ? dex : cd;
#pragma unroll
    for (uint32_t k = 0; k < kFilesScanPer; ++k) {
      if (i0 + k < ntiles) {
        tot[kTileWords * (i0 + k)] = pf;
        tot[kTileWords * (i0 + k) + 1] = pb;
        tot[kTileWords * (i0 + k) + 2] = pd;
      }
      pf += f[k];
      pb += b[k];
      if (d[k] > pd) pd = d[k];
    }
    cf += sum.fr;
    cb += sum.blk;
    if (dsum > cd) cd = dsum;
  }
  if (threadIdx.x == 0) {
    res[1] = cf;
    res[2] = cb;
    const uint64_t st = res[3] != ~0ull ? kIdxDeclined : cf > cap_files ? kIdxCapacity : kIdxOk;
    res[0] = st;
    tot[kTileWords * ntiles] = st;
  }
}

// files[4 f .. 4 f + 4) = the record of the f-th file entry.  Nothing unless
// the scan's status (*gate) is OK (then f < cap_files holds for every f).
__global__ __launch_bounds__(kThreads) void k_files_emit(
    const uint8_t* __restrict__ text, uint64_t len, uint64_t body_off, uint64_t body_end,
    uint64_t bs, uint64_t tile0, uint64_t off_bias, uint64_t block_bias,
    const uint64_t* __restrict__ tot, uint64_t* __restrict__ files, uint64_t cap_files,
    const uint64_t* __restrict__ gate) {
  __shared__ Pair lds[kThreads / 64 + 1];
  __shared__ uint64_t mlds[kThreads / 64];
  if (*gate != kIdxOk) return;  // (uniform: every lane reads the same word)
  const uint64_t s = (tile0 + blockIdx.x) * kIdxTile + threadIdx.x * kSpan;
  const LaneCounts l = files_lane_counts(text, len, s, body_off, body_end, bs, nullptr);
  Pair sum;
  uint64_t dmax;
  const Pair ex = block_excl_scan(l.c, &sum, lds);
  const uint64_t dex = block_excl_max(l.dir1, &dmax, mlds);
  if (l.c.fr == 0) return;  // no file line starts in this lane's span
  const uint64_t* t = tot + kTileWords * (uint64_t)blockIdx.x;
  uint64_t file = t[0] + ex.fr, blk = t[1] + ex.blk;
  uint64_t dir1 = dex > t[2] ? dex : t[2];
  walk_span(text, len, s, body_off, body_end, [&](uint64_t p) {
    const Head h = head_at(text, p, body_off, body_end, bs);
    if (h.kind == idxscan::kDir) dir1 = p + 1;
    if (h.kind != idxscan::kFile) return;
    if (file < cap_files) {
      uint64_t* o = files + files::kFileWords * file;
      o[0] = p + 2 + off_bias;
      o[1] = (dir1 ? dir1 - 1 : body_off) + off_bias;
      o[2] = h.size;
      o[3] = (blk + block_bias) | (files::exe_of(text, h.hash_off) ? files::kExeBit : 0);
    }
    ++file;
    blk += h.nblk;
  });
}

// Four lanes per block, as k_idx_decode: the 16 hex digits j of block g's token
// are checked (lane 0 the separator too), nothing is stored.  Block g finds its
// file by bisecting the records the emit pass wrote and the head of that
// file's line again (heads are short).  A bad token declines its line, as it
// does in cir_index_digests_dev.  Nothing unless the scan's status (*gate) is OK.
__global__ __launch_bounds__(kThreads) void k_files_tokens(
    const uint8_t* __restrict__ text, uint64_t body_off, uint64_t body_end, uint64_t bs,
    uint64_t off_bias, uint64_t block_bias, const uint64_t* __restrict__ files, uint64_t cap_files,
    const uint64_t* __restrict__ gate, uint64_t* __restrict__ res) {
  if (*gate != kIdxOk) return;
  const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t g = gid >> 2;
  const uint32_t j = (uint32_t)gid & 3;
  const uint64_t nfiles = res[1] < cap_files ? res[1] : cap_files;
  if (g >= res[2] || nfiles == 0) return;
  uint64_t lo = 0, hi = nfiles;  // the last file whose first block is <= g
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((files[files::kFileWords * mid + 3] & ~files::kExeBit) - block_bias <= g)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t first = (files[files::kFileWords * lo + 3] & ~files::kExeBit) - block_bias;
  const uint64_t p = files[files::kFileWords * lo] - off_bias - 2;  // the line's start
  if (p < body_off || p >= body_end || g < first) return;
  const Head h = idxscan::parse_head(text, p, body_end, bs);
  const uint64_t k = g - first;
  // (what the head promised, checked again: no load leaves the body)
  if (h.kind != idxscan::kFile || k >= h.nblk || h.hash_off >= body_end ||
      k >= (body_end - h.hash_off) / idxscan::kTokenBytes)
    return;
  const uint8_t* tok = text + h.hash_off + idxscan::kTokenBytes * k;
  uint32_t w[4], o[2];
  __builtin_memcpy(w, tok + 1 + 16 * j, 16);
  bool ok = idxscan::hex16(w, o);
  if (j == 0) ok = ok && tok[0] == ' ';
  if (!ok) {
    atomicMin(reinterpret_cast<unsigned long long*>(res + 3), (unsigned long long)p);
    atomicMax(reinterpret_cast<unsigned long long*>(res), (unsigned long long)kIdxDeclined);
  }
}

static inline void files_tiles(uint64_t body_off, uint64_t body_end, uint64_t* tile0,
                               uint64_t* ntiles) {
  *tile0 = body_off / kIdxTile;
  *ntiles = body_end > body_off ? (body_end + kIdxTile - 1) / kIdxTile - *tile0 : 0;
}

hipError_t launch_index_files(const uint8_t* text, uint64_t len, uint64_t body_off,
                              uint64_t body_end, uint64_t bs, uint64_t off_bias,
                              uint64_t block_bias, uint64_t* files, uint64_t cap_files,
                              uint64_t* work, uint64_t* res, hipStream_t s, bool check_tokens) {
  hipError_t e = hipMemsetAsync(res, 0xFF, files::kResFields * sizeof(uint64_t), s);
  if (e != hipSuccess) return e;
  uint64_t tile0, ntiles;
  files_tiles(body_off, body_end, &tile0, &ntiles);
  if (ntiles) {
    hipLaunchKernelGGL(k_files_count, dim3((unsigned)ntiles), dim3(kThreads), 0, s, text, len,
                       body_off, body_end, bs, tile0, work, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_files_scan, dim3(1), dim3(kThreads), 0, s, work, ntiles, cap_files, res);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ntiles == 0 || cap_files == 0) return hipSuccess;
  hipLaunchKernelGGL(k_files_emit, dim3((unsigned)ntiles), dim3(kThreads), 0, s, text, len,
                     body_off, body_end, bs, tile0, off_bias, block_bias, work, files, cap_files,
                     work + kTileWords * ntiles);
  if ((e = hipGetLastError()) != hipSuccess || !check_tokens) return e;
  const uint64_t maxblk = (body_end - body_off) / idxscan::kTokenBytes;  // what the body can hold
  if (maxblk == 0) return hipSuccess;
  hipLaunchKernelGGL(k_files_tokens, dim3((unsigned)((4 * maxblk + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, text, body_off, body_end, bs, off_bias, block_bias, files,
                     cap_files, work + kTileWords * ntiles, res);
  return hipGetLastError();
}

// ---- the join ------------------------------------------------------------------

namespace {

// The file of block g: the last f with first(f) <= g (nfiles >= 1).  Empty
// files share their `first` with the file behind them, which this finds.
__device__ __forceinline__ uint64_t file_of(const uint64_t* __restrict__ recs, uint64_t nfiles,
                                            uint64_t g) {
  uint64_t lo = 0, hi = nfiles;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((recs[files::kFileWords * mid + 3] & ~files::kExeBit) <= g)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void load_words(const uint8_t* __restrict__ base, uint64_t g,
                                           uint64_t d[4]) {
  const uint4* p = reinterpret_cast<const uint4*>(base + 32 * g);
  const uint4 a = p[0], b = p[1];
  d[0] = a.x | ((uint64_t)a.y << 32);
  d[1] = a.z | ((uint64_t)a.w << 32);
  d[2] = b.x | ((uint64_t)b.y << 32);
  d[3] = b.z | ((uint64_t)b.w << 32);
}

}  // namespace

// fold[2 f + w] += the terms of file f's blocks.  One lane per block slot g <
// a.nblocks; a slot no file covers adds nothing.  Lanes of a wave that share a
// file are summed by a segmented scan over the wave (equal files are adjacent:
// `first` ascends), and the last lane of each segment issues the two adds.
// first_call: lane 0 of workgroup 0 also initialises res.
__global__ __launch_bounds__(kThreads) void k_files_fold(FilesSide a, uint64_t bs, uint64_t seed,
                                                         uint64_t* __restrict__ fold,
                                                         uint64_t* __restrict__ res,
                                                         uint64_t res3) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  if (res && g == 0) {
    res[0] = files::kOk;
    res[1] = 0;
    res[2] = 0;
    res[3] = res3;
  }
  uint64_t f = ~0ull, t0 = 0, t1 = 0;
  if (g < a.nblocks && a.nfiles) {
    const uint64_t cand = file_of(a.recs, a.nfiles, g);
    const uint64_t first = a.recs[files::kFileWords * cand + 3] & ~files::kExeBit;
    const uint64_t n = files::blocks_of(a.recs[files::kFileWords * cand + 2], bs);
    if (g >= first && g - first < n) {
      uint64_t d[4];
      load_words(a.digests, g, d);
      f = cand;
      t0 = files::fold_term(seed, g - first, d, 0);
      t1 = files::fold_term(seed, g - first, d, 1);
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t pf = __shfl_up((unsigned long long)f, d, 64);
    const uint64_t p0 = __shfl_up((unsigned long long)t0, d, 64);
    const uint64_t p1 = __shfl_up((unsigned long long)t1, d, 64);
    if ((int)lane >= d && pf == f) {
      t0 += p0;
      t1 += p1;
    }
  }
  const uint64_t nf = __shfl_down((unsigned long long)f, 1, 64);
  if (f != ~0ull && (lane == 63 || nf != f)) {
    atomicAdd(reinterpret_cast<unsigned long long*>(fold + files::kFoldWords * f),
              (unsigned long long)t0);
    atomicAdd(reinterpret_cast<unsigned long long*>(fold + files::kFoldWords * f + 1),
              (unsigned long long)t1);
  }
}

// Lane j puts pool file j into the table: join.hip's walk, a slot holding a
// pool ordinal + 1 (0 = empty, what the memset left).  Two files are equal
// when they belong to the same source and their decoded paths are equal byte
// by byte, so the slot of (source, path) ends holding the smallest ordinal:
// the source's first entry at that path.  No lane waits for another; the loop
// is bounded by the slot count.
__global__ __launch_bounds__(kThreads) void k_files_build(FilesSide pool,
                                                          const uint64_t* __restrict__ src_first,
                                                          uint64_t nsrc, uint32_t* __restrict__ table,
                                                          uint64_t slots, uint64_t seed) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= pool.nfiles || nsrc == 0) return;
  const uint64_t* r = pool.recs + files::kFileWords * j;
  const uint64_t dir = r[1], name = r[0];
  const uint64_t src = files::src_of(src_first, nsrc, j);
  const uint64_t mask = slots - 1;
  uint64_t at = files::home_slot(files::path_hash(pool.text, pool.text_len, dir, name, seed), src, mask);
  const uint32_t mine = (uint32_t)j + 1;
  for (uint64_t step = 0; step < slots; ++step) {
    uint32_t v = __hip_atomic_load(table + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == 0) {
      v = atomicCAS(table + at, 0u, mine);
      if (v == 0) return;
    }
    if (v <= pool.nfiles) {
      const uint64_t* o = pool.recs + files::kFileWords * (uint64_t)(v - 1);
      if (files::src_of(src_first, nsrc, v - 1) == src &&
          files::same_path(pool.text, pool.text_len, o[1], o[0], pool.text, pool.text_len, dir,
                           name)) {
        if (v > mine) atomicMin(table + at, mine);  // (the value only ever falls)
        return;
      }
    }
    at = (at + 1) & mask;
  }
}

// Lane i looks need file i up in the sources in order.  A hit is the source's
// first entry at the path: equal exe flag, size and fold make the candidate,
// anything else sends the lane to the next source.
__global__ __launch_bounds__(kThreads) void k_files_probe(
    FilesSide need, FilesSide pool, const uint64_t* __restrict__ src_first, uint64_t nsrc,
    const uint32_t* __restrict__ table, uint64_t slots, uint64_t seed,
    const uint64_t* __restrict__ need_fold, const uint64_t* __restrict__ pool_fold,
    uint32_t* __restrict__ cand_src, uint64_t* __restrict__ cand_file, uint64_t* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  uint64_t bytes = 0;
  bool hit = false;
  if (i < need.nfiles) {
    const uint64_t* r = need.recs + files::kFileWords * i;
    const uint64_t name = r[0], dir = r[1], size = r[2], exe = r[3] & files::kExeBit;
    const uint64_t f0 = need_fold[files::kFoldWords * i], f1 = need_fold[files::kFoldWords * i + 1];
    const uint64_t ph = files::path_hash(need.text, need.text_len, dir, name, seed);
    const uint64_t mask = slots - 1;
    uint32_t cs = files::kNoSrc;
    uint64_t cf = files::kNoFile;
    for (uint64_t s = 0; s < nsrc && !hit; ++s) {
      uint64_t at = files::home_slot(ph, s, mask);
      for (uint64_t step = 0; step < slots; ++step) {
        const uint32_t v = table[at];
        if (v == 0 || v > pool.nfiles) break;  // empty (or not an ordinal: never after the build)
        const uint64_t pv = v - 1;
        const uint64_t* o = pool.recs + files::kFileWords * pv;
        if (files::src_of(src_first, nsrc, pv) == s &&
            files::same_path(pool.text, pool.text_len, o[1], o[0], need.text, need.text_len, dir,
                             name)) {
          if (o[2] == size && (o[3] & files::kExeBit) == exe &&
              pool_fold[files::kFoldWords * pv] == f0 &&
              pool_fold[files::kFoldWords * pv + 1] == f1) {
            hit = true;
            cs = (uint32_t)s;
            cf = pv - src_first[s];
            bytes = size;
          }
          break;
        }
        at = (at + 1) & mask;
      }
    }
    cand_src[i] = cs;
    cand_file[i] = cf;
  }
  // one add per wave and word
  const uint64_t votes = __ballot(hit);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) bytes += __shfl_down((unsigned long long)bytes, d, 64);
  if (votes && (threadIdx.x & 63) == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(res + 1), (unsigned long long)__popcll(votes));
    atomicAdd(reinterpret_cast<unsigned long long*>(res + 2), (unsigned long long)bytes);
  }
}

// Lane g checks need block g when its file has a candidate: the digest must be
// the candidate's block at the same position.  A difference, or a position
// outside either list, is a collided fold (or records that do not describe the
// arrays): status kCollision.
__global__ __launch_bounds__(kThreads) void k_files_verify(
    FilesSide need, FilesSide pool, const uint8_t* __restrict__ pool_verify,
    const uint64_t* __restrict__ src_first, uint64_t nsrc, uint64_t bs,
    const uint32_t* __restrict__ cand_src, const uint64_t* __restrict__ cand_file,
    uint64_t* __restrict__ res) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= need.nblocks || need.nfiles == 0) return;
  const uint64_t f = file_of(need.recs, need.nfiles, g);
  const uint64_t first = need.recs[files::kFileWords * f + 3] & ~files::kExeBit;
  const uint64_t n = files::blocks_of(need.recs[files::kFileWords * f + 2], bs);
  if (g < first || g - first >= n) return;  // no file covers this slot
  const uint32_t s = cand_src[f];
  if (s == files::kNoSrc || s >= nsrc) return;
  const uint64_t pv = src_first[s] + cand_file[f];
  bool bad = pv >= pool.nfiles;
  if (!bad) {
    const uint64_t pg = (pool.recs[files::kFileWords * pv + 3] & ~files::kExeBit) + (g - first);
    bad = pg >= pool.nblocks;
    if (!bad) {
      uint64_t a[4], b[4];
      load_words(need.digests, g, a);
      load_words(pool_verify, pg, b);
      bad = ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) != 0;
    }
  }
  if (bad) atomicMax(reinterpret_cast<unsigned long long*>(res), (unsigned long long)files::kCollision);
}

hipError_t launch_match_files(const FilesSide& need, const FilesSide& pool,
                              const uint64_t* src_first, uint64_t nsrc, uint64_t bs,
                              const uint8_t* pool_verify, uint64_t seed, uint64_t* work,
                              uint32_t* cand_src, uint64_t* cand_file, uint64_t* res, hipStream_t s,
                              const hipEvent_t* tev) {
  const uint64_t slots = join_table_slots(pool.nfiles);
  uint64_t* need_fold = work;
  uint64_t* pool_fold = work + files::kFoldWords * need.nfiles;
  uint32_t* table = reinterpret_cast<uint32_t*>(pool_fold + files::kFoldWords * pool.nfiles);
  const FilesSide &na = need, &pa = pool;
  auto grid = [](uint64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); };
  auto mark = [&](int k) { return tev ? hipEventRecord(tev[k], s) : hipSuccess; };
  hipError_t e = hipMemsetAsync(work, 0, match_files_work_bytes(need.nfiles, pool.nfiles), s);
  if (e != hipSuccess || (e = mark(0)) != hipSuccess) return e;
  // (the need side's fold always runs: it initialises res)
  hipLaunchKernelGGL(k_files_fold, grid(need.nblocks ? need.nblocks : 1), dim3(kThreads), 0, s, na,
                     bs, seed, need_fold, res, need.nfiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (pool.nblocks && pool.nfiles) {
    hipLaunchKernelGGL(k_files_fold, grid(pool.nblocks), dim3(kThreads), 0, s, pa, bs, seed,
                       pool_fold, (uint64_t*)nullptr, 0ull);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(1)) != hipSuccess) return e;
  if (pool.nfiles && nsrc) {
    hipLaunchKernelGGL(k_files_build, grid(pool.nfiles), dim3(kThreads), 0, s, pa, src_first, nsrc,
                       table, slots, seed);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(2)) != hipSuccess) return e;
  if (need.nfiles) {
    hipLaunchKernelGGL(k_files_probe, grid(need.nfiles), dim3(kThreads), 0, s, na, pa, src_first,
                       nsrc, table, slots, seed, need_fold, pool_fold, cand_src, cand_file, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(3)) != hipSuccess) return e;
  if (need.nblocks && need.nfiles && pool.nfiles && nsrc) {
    hipLaunchKernelGGL(k_files_verify, grid(need.nblocks), dim3(kThreads), 0, s, na, pa,
                       pool_verify ? pool_verify : pool.digests, src_first, nsrc, bs, cand_src,
                       cand_file, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return mark(4);
}

// ---- the join by content (cir_match_copies_dev) ----------------------------------

// Lane j puts pool file j into the table under its key {size, exe, fold}
// (copies.hpp): k_files_build's walk with another equality.  The key of an
// occupant is read through its record and fold (the folds are complete: the
// fold kernels ran before on the stream).  Every occupant a slot ever has
// carries the key of the lane that claimed it, since only a lane with an equal
// key lowers it, so the slot ends holding the smallest ordinal with that key.
// An empty file takes no part.  No lane waits for another; the loop is bounded
// by the slot count.
__global__ __launch_bounds__(kThreads) void k_copies_build(FilesSide pool,
                                                           const uint64_t* __restrict__ pool_fold,
                                                           uint32_t* __restrict__ table,
                                                           uint64_t slots, uint64_t seed) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= pool.nfiles) return;
  const uint64_t* r = pool.recs + files::kFileWords * j;
  const uint64_t size = r[2], first = r[3];
  if (size == 0) return;
  const uint64_t f0 = pool_fold[files::kFoldWords * j], f1 = pool_fold[files::kFoldWords * j + 1];
  const uint64_t mask = slots - 1;
  uint64_t at = copies::home_slot(size, first & files::kExeBit, f0, f1, seed, mask);
  const uint32_t mine = (uint32_t)j + 1;
  for (uint64_t step = 0; step < slots; ++step) {
    uint32_t v = __hip_atomic_load(table + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == 0) {
      v = atomicCAS(table + at, 0u, mine);
      if (v == 0) return;
    }
    if (v <= pool.nfiles) {
      const uint64_t pv = v - 1;
      const uint64_t* o = pool.recs + files::kFileWords * pv;
      if (copies::same_key(o[2], o[3], pool_fold[files::kFoldWords * pv],
                           pool_fold[files::kFoldWords * pv + 1], size, first, f0, f1)) {
        if (v > mine) atomicMin(table + at, mine);  // (the value only ever falls)
        return;
      }
    }
    at = (at + 1) & mask;
  }
}

// Lane i looks need file i up by its key, unless it is empty or the caller's
// bitmap leaves it out: from the key's home slot to an equal key or an empty
// slot.  The hit is the smallest pool ordinal with that key; its source,
// its ordinal inside the source and the two text offsets of its record are
// the outputs.
__global__ __launch_bounds__(kThreads) void k_copies_probe(
    FilesSide need, FilesSide pool, const uint64_t* __restrict__ src_first, uint64_t nsrc,
    const uint64_t* __restrict__ skip, const uint32_t* __restrict__ table, uint64_t slots,
    uint64_t seed, const uint64_t* __restrict__ need_fold, const uint64_t* __restrict__ pool_fold,
    uint32_t* __restrict__ cand_src, uint64_t* __restrict__ cand_file,
    uint64_t* __restrict__ cand_place, uint64_t* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  uint64_t bytes = 0;
  bool hit = false;
  if (i < need.nfiles) {
    const uint64_t* r = need.recs + files::kFileWords * i;
    const uint64_t size = r[2], first = r[3];
    uint32_t cs = files::kNoSrc;
    uint64_t cf = files::kNoFile, name = copies::kNoPlace, dir = copies::kNoPlace;
    if (size != 0 && nsrc != 0 && !copies::skipped(skip, i)) {
      const uint64_t f0 = need_fold[files::kFoldWords * i], f1 = need_fold[files::kFoldWords * i + 1];
      const uint64_t mask = slots - 1;
      uint64_t at = copies::home_slot(size, first & files::kExeBit, f0, f1, seed, mask);
      for (uint64_t step = 0; step < slots; ++step) {
        const uint32_t v = table[at];
        if (v == 0 || v > pool.nfiles) break;  // empty (or not an ordinal: never after the build)
        const uint64_t pv = v - 1;
        const uint64_t* o = pool.recs + files::kFileWords * pv;
        if (copies::same_key(o[2], o[3], pool_fold[files::kFoldWords * pv],
                             pool_fold[files::kFoldWords * pv + 1], size, first, f0, f1)) {
          const uint64_t s = files::src_of(src_first, nsrc, pv);
          hit = true;
          cs = (uint32_t)s;
          cf = pv - src_first[s];
          name = o[0];
          dir = o[1];
          bytes = size;
          break;
        }
        at = (at + 1) & mask;
      }
    }
    cand_src[i] = cs;
    cand_file[i] = cf;
    cand_place[copies::kPlaceWords * i] = name;
    cand_place[copies::kPlaceWords * i + 1] = dir;
  }
  // one add per wave and word
  const uint64_t votes = __ballot(hit);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) bytes += __shfl_down((unsigned long long)bytes, d, 64);
  if (votes && (threadIdx.x & 63) == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(res + 1), (unsigned long long)__popcll(votes));
    atomicAdd(reinterpret_cast<unsigned long long*>(res + 2), (unsigned long long)bytes);
  }
}

hipError_t launch_match_copies(const FilesSide& need, const FilesSide& pool,
                               const uint64_t* src_first, uint64_t nsrc, uint64_t bs,
                               const uint64_t* skip, const uint8_t* pool_verify, uint64_t seed,
                               uint64_t* work, uint32_t* cand_src, uint64_t* cand_file,
                               uint64_t* cand_place, uint64_t* res, hipStream_t s,
                               const hipEvent_t* tev) {
  const uint64_t slots = join_table_slots(pool.nfiles);
  uint64_t* need_fold = work;
  uint64_t* pool_fold = work + files::kFoldWords * need.nfiles;
  uint32_t* table = reinterpret_cast<uint32_t*>(pool_fold + files::kFoldWords * pool.nfiles);
  const FilesSide &na = need, &pa = pool;
  auto grid = [](uint64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); };
  auto mark = [&](int k) { return tev ? hipEventRecord(tev[k], s) : hipSuccess; };
  hipError_t e = hipMemsetAsync(work, 0, match_files_work_bytes(need.nfiles, pool.nfiles), s);
  if (e != hipSuccess || (e = mark(0)) != hipSuccess) return e;
  // (the need side's fold always runs: it initialises res)
  hipLaunchKernelGGL(k_files_fold, grid(need.nblocks ? need.nblocks : 1), dim3(kThreads), 0, s, na,
                     bs, seed, need_fold, res, need.nfiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (pool.nblocks && pool.nfiles) {
    hipLaunchKernelGGL(k_files_fold, grid(pool.nblocks), dim3(kThreads), 0, s, pa, bs, seed,
                       pool_fold, (uint64_t*)nullptr, 0ull);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(1)) != hipSuccess) return e;
  if (pool.nfiles && nsrc) {
    hipLaunchKernelGGL(k_copies_build, grid(pool.nfiles), dim3(kThreads), 0, s, pa, pool_fold, table,
                       slots, seed);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(2)) != hipSuccess) return e;
  if (need.nfiles) {
    hipLaunchKernelGGL(k_copies_probe, grid(need.nfiles), dim3(kThreads), 0, s, na, pa, src_first,
                       nsrc, skip, table, slots, seed, need_fold, pool_fold, cand_src, cand_file,
                       cand_place, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(3)) != hipSuccess) return e;
  if (need.nblocks && need.nfiles && pool.nfiles && nsrc) {
    hipLaunchKernelGGL(k_files_verify, grid(need.nblocks), dim3(kThreads), 0, s, na, pa,
                       pool_verify ? pool_verify : pool.digests, src_first, nsrc, bs, cand_src,
                       cand_file, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return mark(4);
}

}  // namespace dev
}  // namespace cir
