// Host-side launchers for the gfx950 kernels in kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cir {
namespace emit {
struct Tables;  // emit.hpp
}
namespace update {
struct Plan;
}
namespace copyblk {
struct Plan;  // copyblk.hpp
}
namespace dev {

constexpr int kThreads = 256;  // 4 waves per workgroup (every kernel but the two below)
// k_chunks and k_compress_only: 8 waves per workgroup, two on every SIMD of
// the CU, kept in phase by PhaseBarrier (uniform.hpp); two workgroups per CU
// make the four waves per SIMD, 64 KiB of LDS each.  Batches that are not
// whole layers of two waves per SIMD run k_chunks_free at kThreads
// (kernels.hip chunks_phase_aligned).
constexpr int kChunkThreads = 512;

enum class Loader : int { kGlds = 0, kDirect = 1 };

// Chains of at least this many 128-B lines (128 KiB) run 4 lanes per chain.
// config 3 A/B (profiles/r01/cfg3_quad_threshold.log): 2048 lines 659 GiB/s,
// 1024 782, 512 760, 256 769 -- below 2048, the ragged 1 MiB blocks no
// longer trail the lane kernel.
constexpr uint32_t kQuadMinLines = 1024;
constexpr int kQuadMaxWg = 256;  // at most 256 x 64 = 16384 chains in quad mode

// Small batches: lane mode is latency-bound below about one wave per SIMD
// (64 x 1024 = 65536 chains; lane mode measured 2232 GiB/s at 8 M x 4 KiB
// but 1024 GiB/s at 32 K x 1 MiB and 258 at 8 K x 4 MiB).  Batches of at
// most 49152 chains run every chain of at least kQuadSmallMinLines lines in
// quad mode (4 x the waves, ~1/3 the latency per compression): 1648-1700
// GiB/s at 32 K x 1 MiB, 757-784 at 8 K x 4 MiB (asm quad G).  The two
// modes cross at ~49152 chains (within 4 % there at 32 KiB, 256 KiB and
// 1 MiB); at 65535 lane mode is ahead (1606 vs 1438 GiB/s at 32 KiB, 1916
// vs 1703 at 256 KiB; profiles/r01/quad_asm_ab.md).
constexpr uint64_t kQuadSmallBatch = 49153;
constexpr uint32_t kQuadSmallMinLines = 8;
inline uint32_t quad_min_lines(uint64_t n) {
  return n < kQuadSmallBatch ? kQuadSmallMinLines : kQuadMinLines;
}
inline uint64_t quad_max_wg(uint64_t n) {
  return n < kQuadSmallBatch ? (n + 63) / 64 : (uint64_t)kQuadMaxWg;
}

// nblk equal blocks of bs bytes at data (bs % 128 == 0, data 16-byte aligned,
// nblk % 256 == 0).  out: nblk x 32 bytes.
hipError_t launch_uniform(Loader loader, const uint8_t* data, uint64_t bs, uint64_t nblk,
                          uint8_t* out, hipStream_t s);

// Hashes::hash_file on one device-resident file: ceil(nbytes / bs) blocks, the
// last one short, digest i -> out + 32 i.  One launch (uniform body through
// LDS-DMA when bs % 128 == 0 and data is 16-byte aligned, ragged rest fused).
hipError_t launch_chunks(const uint8_t* data, uint64_t nbytes, uint64_t bs, uint8_t* out,
                         hipStream_t s);

// Device scratch of the relays (k_quad_relay, k_desc_relay): a flag and
// 64 x 16 B of chain values per group of 16 chains (one quad-mode wave).
// Every relay runs on the device's quad-part stream (qs), so relays of
// different calls are ordered by that one stream.
struct RelayScratch {
  uint32_t* flags = nullptr;
  uint64_t* state = nullptr;
  uint32_t groups = 0;  // capacity
};
constexpr uint32_t kRelayMaxGroups = 4096;
inline size_t relay_scratch_bytes(uint32_t groups) { return (size_t)groups * (4 + 64 * 16); }

// launch_chunks with the ragged rest in quad mode on qs, concurrently with
// the uniform part on s (fork / join events); a file of k whole lane waves
// per SIMD plus a few blocks runs the extra blocks as relayed
// quad chains on qs (relay, when given); launch_chunks where neither
// applies (small or misaligned files, no rest, qs null or == s).
hipError_t launch_chunks_split(const uint8_t* data, uint64_t nbytes, uint64_t bs, uint8_t* out,
                               hipStream_t s, hipStream_t qs, hipEvent_t fork, hipEvent_t join,
                               const RelayScratch* relay = nullptr);
// Number of blocks launch_chunks_split would relay (0: no relay) for a file
// of nfull whole blocks of bs bytes on the current device.
uint64_t relay_blocks(uint64_t nfull, uint64_t bs);

// Blocks first .. first+n-1 of Hashes::hash_file's split of [data, data+nbytes).
hipError_t launch_general_chunks(const uint8_t* data, uint64_t nbytes, uint64_t bs,
                                 uint64_t first, uint64_t n, uint8_t* out, hipStream_t s);

// Per-descriptor BlockHash::hash_bytes; digest of block b goes to out + 32*b.
// perm (nullable) is the processing order (a permutation of 0..n-1).
hipError_t launch_general_desc(const uint8_t* arena, const uint64_t* off, const uint32_t* len,
                               const uint32_t* perm, uint64_t n, uint8_t* out, hipStream_t s);

// Descriptor batch in the order perm (longest chain first); the first
// *n_long chains (device count) run in quad mode when 64 * quad_max_wg(n) hold them, on
// qs, the rest one lane per chain on s; the quad part forks from s (`fork`)
// and joins back into it (`qjoin`).
// relay (nullable): scratch for relaying the chains past k whole lane (or
// quad) waves per SIMD (k_desc_relay; decided on the device).
// tev (nullable, diagnostics): 4 timing events recorded around the quad
// part (0, 1; on its stream) and the lane part (2, 3; on s).
hipError_t launch_mixed(const uint8_t* arena, const uint64_t* off, const uint32_t* len,
                        const uint32_t* perm, uint32_t* n_long, uint64_t n, uint8_t* out,
                        hipStream_t s, hipStream_t qs, hipEvent_t fork, hipEvent_t qjoin,
                        const RelayScratch* relay = nullptr,
                        const hipEvent_t* tev = nullptr);

// Longest-chain-first order of a descriptor batch (order.hip): *perm points
// into `scratch` (order_scratch_bytes(n) bytes, device memory).
size_t order_scratch_bytes(uint64_t n);
// *n_long = number of chains with >= quad_min_lines(n) lines (device memory);
// (*n_long)[1] = 0, the started-workgroup counter of the quad part;
// (*n_long)[2] = the longest chain's compressions; (*n_long)[4..5] (u64) =
// the other chains' compressions + kLaneChainCost each.
constexpr uint32_t kLaneChainCost = 4;
hipError_t launch_order_desc(const uint32_t* len, uint64_t n, void* scratch, size_t bytes,
                             uint32_t** perm, uint32_t** n_long, hipStream_t s);

// Bounds of an untrusted descriptor batch (order.hip): in `scratch`
// (bound_scratch_bytes(n) bytes of device memory) *slen = the lengths with
// every out-of-range block's set to 0 (off + len wraps or passes
// arena_bytes), *flag = 1 per out-of-range block; *nflag (device u32, zeroed
// here; NULL: a counter inside the scratch) = their number.
size_t bound_scratch_bytes(uint64_t n);
hipError_t launch_desc_bound(const uint64_t* off, const uint32_t* len, uint64_t n,
                             uint64_t arena_bytes, void* scratch, uint32_t* nflag,
                             uint32_t** slen, uint8_t** flag, hipStream_t s);
// out + 32 b = 32 zero bytes for every flagged block b.
hipError_t launch_desc_zero(const uint8_t* flag, uint64_t n, uint8_t* out, hipStream_t s);

// SHA-512/256 per descriptor (one lane per block), digest b -> out + 32 b.
hipError_t launch_sha_desc(const uint8_t* arena, const uint64_t* off, const uint32_t* len,
                           const uint32_t* perm, uint64_t n, uint8_t* out, hipStream_t s);

// Resumable single-chain BLAKE2b-256 (quad mode).  st: 16 x u64 of device
// memory, zeroed before the first call.  Non-final calls take a multiple of
// 128 bytes; the final call takes the rest (>= 1 byte unless the whole input
// is empty) and leaves the digest in st[0..3].
hipError_t launch_chain_step(uint64_t* st, const uint8_t* data, uint32_t n, bool final,
                             hipStream_t s);

// One BLAKE2b-256 chain over n bytes of device-mapped pinned host memory
// h_src (16-B aligned, readable up to n rounded up to 16), staged through
// d_scratch (same rounding) by the kernel itself; the digest is written to
// device-mapped host memory h_out (32 B).  One launch, nothing else.
hipError_t launch_single(const uint8_t* h_src, uint32_t n, uint8_t* d_scratch, uint8_t* h_out,
                         hipStream_t s);

// Compare n digests (32 B each, both 16-B aligned) with the expected ones:
// ok[b] = 1 / 0 (ok may be null); *nbad += mismatches (nbad may be null).
// flag (nullable): a flagged block is a mismatch whatever its digest.
hipError_t launch_verify(const uint8_t* got, const uint8_t* want, uint64_t n, uint8_t* ok,
                         uint32_t* nbad, hipStream_t s, const uint8_t* flag = nullptr);

// The same compare, answering only "which digest first": *first (device u64)
// = base + the smallest b whose digest differs (or whose flag is set),
// UINT64_MAX when none; *nbad (device u32, nullable) = how many.  Both are
// initialised here, on the same stream (also when n == 0).
hipError_t launch_first_bad(const uint8_t* got, const uint8_t* want, uint64_t n, uint64_t base,
                            uint64_t* first, uint32_t* nbad, hipStream_t s,
                            const uint8_t* flag = nullptr);

// The same compare with a verdict per segment: segment s is the digests
// [seg_end[s-1], seg_end[s]) (seg_end non-decreasing, seg_end[nseg-1] == n);
// seg_bad[s] = 1 when any digest of s differs (or its flag is set), else 0;
// *nbad_seg (device u32, nullable) = how many segments are bad.  All nseg
// flags and the count are written here, on the same stream (also when n ==
// 0); a mismatch's segment index is clamped to [0, nseg), so nothing outside
// seg_bad[0 .. nseg) is written whatever seg_end holds.
hipError_t launch_seg_bad(const uint8_t* got, const uint8_t* want, uint64_t n,
                          const uint32_t* seg_end, uint64_t nseg, uint8_t* seg_bad,
                          uint32_t* nbad_seg, hipStream_t s, const uint8_t* flag = nullptr);

// The same compare as a bitmap: bit (b & 63) of have[b >> 6] (device u64s,
// 8-B aligned) = 1 when digest b equals the expected one and its flag is not
// set.  Every word of [0, ceil(n/64)) is stored here (the last word's bits at
// positions >= n as 0) and nothing past them; n == 0 stores no word.  *nbad
// (device u32, nullable) = how many of the n are not ok, initialised here on
// the same stream (also when n == 0).
hipError_t launch_block_bits(const uint8_t* got, const uint8_t* want, uint64_t n, uint64_t* have,
                             uint32_t* nbad, hipStream_t s, const uint8_t* flag = nullptr);

// Join of two digest lists (join.hip; cir_match_digests_dev): match[i] = the
// smallest j < n_pool with pool[j] == need[i] over all 32 bytes, or
// UINT32_MAX; *nmatch (device u32, nullable) = how many matched.  `table` is
// table_slots u32 of scratch (a power of two >= join_table_slots(n_pool)),
// initialised here; every match[0 .. n_need) and the count are written here,
// all on `s`.  n_pool <= kJoinMaxPool, n_need < 2^32; both lists 16-B aligned.
// tev (nullable, a traced cir_block_sources): 3 events recorded before the
// build kernel, between the two kernels and after the probe kernel.
constexpr uint32_t kJoinEmpty = 0xFFFFFFFFu;
constexpr uint64_t kJoinMaxPool = 0x7FFFFFFFull;
inline uint64_t join_table_slots(uint64_t n_pool) {
  if (n_pool > (1ull << 62)) return 0;  // no u64 holds it (callers cap n_pool far below)
  uint64_t s = 64;
  while (s < 2 * n_pool) s <<= 1;
  return s;
}
hipError_t launch_join(const uint8_t* need, uint64_t n_need, const uint8_t* pool, uint64_t n_pool,
                       uint32_t* table, uint64_t table_slots, uint64_t seed, uint32_t* match,
                       uint32_t* nmatch, hipStream_t s, const hipEvent_t* tev = nullptr);

// An index's block digests parsed on the device (idxscan.hip;
// cir_index_digests_dev): the body text[body_off, body_end) of a
// DIRSIGNATURE.v1 index of `len` bytes (text 8-B aligned) to digests (32 B
// per block, 16-B aligned, at most cap_blocks) and runs (4 u64 per non-empty
// file {first, size, file, hash_off}, at most cap_runs), all on `s`.  work:
// idx_work_bytes(len) bytes of scratch; res: kIdxResFields u64 {status, file
// entries, runs, blocks, start of the first declined line or UINT64_MAX}, all
// initialised here.  Unchecked: body_off <= body_end <= len <= kIdxMaxLen, bs
// != 0, cap_blocks < 2^32.
constexpr uint32_t kIdxTile = 4096;  // bytes of text per workgroup of the count and emit passes
// Longest text: below it no sum of per-line block counts can pass 2^64 even
// over lines that overlap (at most len / 8 lines of at most len / 65 blocks).
constexpr uint64_t kIdxMaxLen = 1ull << 36;
constexpr int kIdxResFields = 5;
constexpr uint64_t kIdxOk = 0, kIdxCapacity = 1, kIdxDeclined = 2;
inline uint64_t idx_work_bytes(uint64_t len) { return 24 * (len / kIdxTile + 2); }
hipError_t launch_index_digests(const uint8_t* text, uint64_t len, uint64_t body_off,
                                uint64_t body_end, uint64_t bs, uint8_t* digests,
                                uint64_t cap_blocks, uint64_t* runs, uint64_t cap_runs,
                                uint64_t* work, uint64_t* res, hipStream_t s);
// Its two halves, for a caller that learns the counts in between (a
// synchronise of its own) in order to place the digests: launch_index_count =
// the count and scan passes (res is complete but for a bad token's verdict);
// launch_index_emit = the emit and decode passes into digests / runs, gated on
// the scan's status in `work`; max_blocks = an upper bound of res[3] (the
// decode's grid), at most the digests' capacity.
hipError_t launch_index_count(const uint8_t* text, uint64_t len, uint64_t body_off,
                              uint64_t body_end, uint64_t bs, uint64_t cap_blocks,
                              uint64_t cap_runs, uint64_t* work, uint64_t* res, hipStream_t s);
hipError_t launch_index_emit(const uint8_t* text, uint64_t len, uint64_t body_off,
                             uint64_t body_end, uint64_t bs, uint8_t* digests, uint64_t max_blocks,
                             uint64_t* runs, uint64_t cap_runs, uint64_t* work, uint64_t* res,
                             hipStream_t s);

// Local copies merged into extents (extents.hip; cir_match_extents_dev; the
// rule is extents.hpp): match[0 .. n_need) as launch_join leaves it and the two
// run tables (4 u64 per non-empty file {first, size, file, x}, x = the source
// ordinal in the pool's) to the per-block arrays (src / file / block, all or
// none), the fetch bitmap (ceil(n_need / 64) u64, nullable), the counts and
// the extent records (extents::kRecWords u64 each), all on `s`.  work:
// ext_work_bytes(n_need) bytes of scratch; res: extents::kResFields u64
// {status, wanted, found, bytes, dropped, extents}, all initialised here.
// Unchecked: bs != 0, n_need < 2^32, n_pool <= kJoinMaxPool.
// A tile of 2048 blocks keeps the one-workgroup scan at 2^21 totals (1024
// steps of 2048) for 2^32 - 1 blocks, and a tile's 32 head words fit one
// shuffle scan of a wave.
constexpr uint32_t kExtTile = 2048;  // need blocks per workgroup of the map and emit passes
inline uint64_t ext_tiles(uint64_t n_need) { return (n_need + kExtTile - 1) / kExtTile; }
inline uint64_t ext_work_bytes(uint64_t n_need) {
  return 8 * (2 * ((n_need + 63) / 64) + ext_tiles(n_need) + 2);
}
struct ExtentArgs {
  const uint32_t* match;
  uint64_t n_need;
  const uint64_t* need_runs;
  uint64_t n_need_runs;
  const uint64_t* pool_runs;
  uint64_t n_pool_runs;
  uint64_t n_pool;
  uint64_t bs;
  const uint64_t* want;  // nullable
};
// Its two halves, for a caller that learns the extent count in between (a
// synchronise of its own) in order to size the records: launch_extent_map =
// the map and scan passes (every res word, the per-block arrays and the
// bitmap are final); launch_extent_emit = the emit and finish passes, gated on
// the scan's status in `work`; max_extents = an upper bound of res[5] (the
// finish pass's grid).  No record at or past cap_extents is written.  tev
// (nullable, a traced call): 3 events recorded before the map kernel, between
// the two kernels and after the scan kernel.
hipError_t launch_extent_map(const ExtentArgs& a, uint32_t* src, uint64_t* file, uint64_t* block,
                             uint64_t* fetch, uint64_t cap_extents, uint64_t* work, uint64_t* res,
                             hipStream_t s, const hipEvent_t* tev = nullptr);
hipError_t launch_extent_emit(const ExtentArgs& a, uint64_t* ext, uint64_t cap_extents,
                              uint64_t max_extents, uint64_t* work, uint64_t* res, hipStream_t s);

// Join of one digest list with itself (repeats.hip; cir_match_repeats_dev; the
// rule is repeats.hpp): match[g] = UINT32_MAX when block g is not wanted or is
// its digest's leader, else the leader as an ordinal of a pool of 2n (L when
// it is present, n + L when it is wanted); *nmatch (device u32, nullable) =
// how many are not UINT32_MAX.  want / present: bitmaps of ceil(n / 64) u64,
// nullable.  `table` is table_slots u32 of scratch (a power of two >=
// join_table_slots(n)), initialised here; every match[0 .. n) and the count
// are written here, all on `s`.  n <= kRepeatMaxBlocks; digests 16-B aligned.
// tev (nullable, a traced cir_block_repeats): 3 events as launch_join's.
constexpr uint64_t kRepeatMaxBlocks = 0x3FFFFFFFull;
hipError_t launch_repeat_join(const uint8_t* digests, uint64_t n, const uint64_t* want,
                              const uint64_t* present, uint32_t* table, uint64_t table_slots,
                              uint64_t seed, uint32_t* match, uint32_t* nmatch, hipStream_t s,
                              const hipEvent_t* tev = nullptr);

// An index's file entries parsed on the device (files.hip;
// cir_index_files_dev; the rule is files.hpp): the body of a text as
// launch_index_digests takes it to one record of 4 u64 per file entry {name_off
// + off_bias, dir_off + off_bias, size, (first + block_bias) | exe << 63}, at
// most cap_files, all on `s`.  work: files_work_bytes(len) bytes of scratch;
// res: 4 u64 {status (kIdx*), file entries, blocks, start of the first
// declined line or UINT64_MAX}, all initialised here.  check_tokens: a last
// pass reads every hash token's digits and declines a bad one's line (false: a
// caller that runs launch_index_emit on the same text has that verdict).
// Unchecked: as launch_index_digests; cap_files < 2^58.
inline uint64_t files_work_bytes(uint64_t len) { return 32 * (len / kIdxTile + 2); }
hipError_t launch_index_files(const uint8_t* text, uint64_t len, uint64_t body_off,
                              uint64_t body_end, uint64_t bs, uint64_t off_bias,
                              uint64_t block_bias, uint64_t* files, uint64_t cap_files,
                              uint64_t* work, uint64_t* res, hipStream_t s,
                              bool check_tokens = true);

// Join of two file lists (files.hip; cir_match_files_dev): per need file the
// first source, in order, whose first entry at the file's path has the same exe
// flag, size and digests: cand_src[i] (UINT32_MAX: none) and cand_file[i] (the
// file ordinal inside that source; UINT64_MAX: none).  A side is an arena of
// texts, the file records over it and the flat digests their `first` count
// into (16-B aligned); pool files are ordered by source, src_first (nsrc + 1
// u64) the first pool ordinal of each.  pool_verify (nullable: pool.digests):
// the digests the candidates are verified against.  work:
// match_files_work_bytes(need.nfiles, pool.nfiles) bytes of scratch, zeroed
// here; res: 4 u64 {status, candidates, their bytes, need files}, all written
// here; everything on `s`.  Unchecked: bs != 0, pool.nfiles <= kJoinMaxPool,
// need.nfiles < 2^32, both block counts < 2^32.  tev (nullable, a traced
// cir_file_sources): 5 events around the memset, the folds, the build, the
// probe and the verify.
struct FilesSide {
  const uint8_t* text;
  uint64_t text_len;
  const uint64_t* recs;
  uint64_t nfiles;
  const uint8_t* digests;
  uint64_t nblocks;
};
inline uint64_t match_files_work_bytes(uint64_t n_need_files, uint64_t n_pool_files) {
  return 16 * (n_need_files + n_pool_files) + 4 * join_table_slots(n_pool_files);
}
hipError_t launch_match_files(const FilesSide& need, const FilesSide& pool,
                              const uint64_t* src_first, uint64_t nsrc, uint64_t bs,
                              const uint8_t* pool_verify, uint64_t seed, uint64_t* work,
                              uint32_t* cand_src, uint64_t* cand_file, uint64_t* res, hipStream_t s,
                              const hipEvent_t* tev = nullptr);

// Join of two file lists by content (files.hip; cir_match_copies_dev; the rule
// is copies.hpp): per need file that is neither empty nor skipped (skip:
// nullable bitmap of u64 words over need file ordinals) the pool file of the
// smallest ordinal with the same exe flag, size and digests, at any path:
// cand_src / cand_file as launch_match_files writes them and cand_place[2 i
// ..] = that pool record's {name_off, dir_off} (UINT64_MAX: none).  The
// sides' texts are not read.  work, res, pool_verify, tev and what is
// unchecked: as launch_match_files.
hipError_t launch_match_copies(const FilesSide& need, const FilesSide& pool,
                               const uint64_t* src_first, uint64_t nsrc, uint64_t bs,
                               const uint64_t* skip, const uint8_t* pool_verify, uint64_t seed,
                               uint64_t* work, uint32_t* cand_src, uint64_t* cand_file,
                               uint64_t* cand_place, uint64_t* res, hipStream_t s,
                               const hipEvent_t* tev = nullptr);

// The glue of a download plan (plan.hip; cir_plan_links_dev, cir_plan_want_dev;
// the rule is plan.hpp).  launch_plan_links: behind launch_match_files, the
// candidates of files whose bit in deny (nullable) is set are withdrawn, skip
// (ceil(n_files / 64) u64, every word written) = deny | candidate kept, res = 2
// u64 {kept, withdrawn}.  launch_plan_want: behind launch_match_copies, want
// (ceil(n_blocks / 64) u64, every word written) = blocks of the file entries of
// the run table `runs` (4 u64 per non-empty file, `first` ascending) whose file
// has a candidate in neither cand_a nor cand_b (n_files u32 each, nullable) and
// whose bit in have (nullable) is 0; res = 3 u64 {wanted, blocks of linked
// files, left out by have}.  res is zeroed here, all on `s`.  Unchecked: bs !=
// 0, n_files and n_blocks < 2^32.
hipError_t launch_plan_links(const uint64_t* deny, uint64_t n_files, uint32_t* cand_src,
                             uint64_t* cand_file, uint64_t* skip, uint64_t* res, hipStream_t s);
hipError_t launch_plan_want(const uint64_t* runs, uint64_t n_runs, uint64_t n_blocks, uint64_t bs,
                            uint64_t n_files, const uint32_t* cand_a, const uint32_t* cand_b,
                            const uint64_t* have, uint64_t* want, uint64_t* res, hipStream_t s);

// The content sketch of a digest list (sketch.hip; cir_sketch_digests_dev; the
// rule is sketch.hpp): keys[0 .. res[1]) = the k smallest distinct keys of the
// n digests (16-B aligned), ascending, all on `s`.  work:
// sketch_work_bytes(n) bytes of scratch, initialised here; res:
// kSketchResFields u64 {status, keys written, n, candidates sorted}, all
// written here.  kSketchDeclined: the answer did not fit the scratch (more
// distinct keys than kSketchCands at or below the k-th key's histogram bin, or
// a probe walk past kSketchWalk slots); the keys then mean nothing.
// Unchecked: 1 <= k <= sketch::kMaxK, n < 2^32.  tev (nullable, a traced
// cir_index_sketch): 2 events around the whole of it.
constexpr int kSketchResFields = 4;
constexpr uint64_t kSketchOk = 0, kSketchDeclined = 1;
constexpr uint32_t kSketchCands = 8192;  // u64 keys the last kernel sorts in LDS (64 KiB)
constexpr uint32_t kSketchWalk = 1024;   // probed slots per key before the call declines
constexpr int kSketchHeadWords = 8;
constexpr uint64_t kSketchEmpty = ~0ull;  // (the key 2^64 - 1 is kept in a flag of its own)
inline uint64_t sketch_table_slots(uint64_t n) {
  uint64_t s = 1024;
  while (s < 2 * n) s <<= 1;
  return s;
}
// Histogram bins over the keys' top bits: about 64 distinct keys per bin when
// every digest is distinct, at least 2^10 and at most 2^26 bins.
inline uint32_t sketch_hist_bits(uint64_t n) {
  uint32_t b = 10;
  while (b < 26 && (64ull << b) < n) ++b;
  return b;
}
inline uint64_t sketch_work_bytes(uint64_t n) {
  return 8 * (kSketchHeadWords + (uint64_t)kSketchCands) + (4ull << sketch_hist_bits(n)) +
         8 * sketch_table_slots(n);
}
hipError_t launch_sketch(const uint8_t* digests, uint64_t n, uint32_t k, uint64_t* keys,
                         uint64_t* work, uint64_t* res, hipStream_t s,
                         const hipEvent_t* tev = nullptr);

// The body text of an index from digests in device memory (emit.hip;
// cir_index_emit_dev; the rule is emit.hpp): every byte of body[0,
// round_up(t.body_len, 16)) is written and nothing else (body 16-B aligned);
// res: kEmitResFields u64 {pieces whose literal or block range lies outside the
// arrays: their bytes are 0}, zeroed here, all on `s`.  Unchecked: t.npieces <=
// emit::kMaxPieces, t.body_len <= kEmitMaxBody, t.ndigests <= kEmitMaxDigests.
constexpr int kEmitResFields = 1;
constexpr uint64_t kEmitMaxBody = 1ull << 40;     // the grid: 2^36 lanes of 16 bytes
constexpr uint64_t kEmitMaxDigests = 1ull << 40;  // 65 x and 32 x a block ordinal stay in u64
hipError_t launch_emit_text(const emit::Tables& t, uint8_t* body, uint64_t* res, hipStream_t s);
// The descriptors of the blocks of files in device memory (emit.hip;
// cir_index_memory_dev): off[g], len[g] for every g < nblocks from the table of
// non-empty files (emit::kFileWords u64 each {first_block, base offset, size},
// first_block ascending), on `s`.  Unchecked: bs != 0 and below 2^32, nblocks <
// 2^32.
hipError_t launch_mem_desc(const uint64_t* files, uint64_t nfiles, uint64_t bs, uint64_t nblocks,
                           uint64_t* off, uint32_t* len, hipStream_t s);

// The packed runs of a staging slot copied to their places (scatter.hip;
// cir_scatter_runs_dev, cir_load_blocks; the rule is scatter.hpp): for every
// sound record {unit_first, src_pos, dst, bytes} of `runs` (scatter::kRunWords
// u64 each) the bytes src[src_pos, src_pos + bytes) stand at dst afterwards and
// no other byte is written; res: kScatterResFields u64 {bad records: written
// nowhere, read nowhere}, zeroed here, all on `s`.  src 16-byte aligned.  No
// launch when there is neither a unit nor a record.  Unchecked: nruns <=
// scatter::kMaxRuns, nunits <= scatter::kMaxUnits.
constexpr int kScatterResFields = 1;
hipError_t launch_scatter_runs(const uint8_t* src, uint64_t src_bytes, const uint64_t* runs,
                               uint64_t nruns, uint64_t nunits, uint64_t* res, hipStream_t s);

// Bytes anywhere in device memory copied into the packed runs of a staging
// slot (gather.hip; cir_gather_runs_dev, cir_store_blocks; the rule is
// gather.hpp): for every sound record {unit_first, dst_pos, src, bytes} of
// `runs` (gather::kRunWords u64 each) the bytes at src stand at dst[dst_pos,
// dst_pos + bytes) afterwards, zeros behind them up to the next multiple of 16,
// and no other byte is written; res: kGatherResFields u64 {bad records: written
// nowhere, read nowhere}, zeroed here, all on `s`.  dst 16-byte aligned and not
// overlapping any source.  No launch when there is neither a unit nor a record.
// Unchecked: nruns <= gather::kMaxRuns, nunits <= gather::kMaxUnits.
constexpr int kGatherResFields = 1;
hipError_t launch_gather_runs(uint8_t* dst, uint64_t dst_bytes, const uint64_t* runs,
                              uint64_t nruns, uint64_t nunits, uint64_t* res, hipStream_t s);

// Runs of bytes copied between buffers of any alignment inside device memory
// (copyblk.hip; cir_copy_runs_dev, cir_reload_blocks; the rule is copyblk.hpp):
// for every sound record {unit_first, src, dst, bytes} of `runs`
// (copyblk::kRunWords u64 each) the bytes at src stand at dst afterwards and no
// other byte is written; res: kCopyResFields u64 {bad records: written nowhere,
// read nowhere}, zeroed here, all on `s`.  Sources and destinations of one table
// must not overlap.  No launch when there is neither a unit nor a record.
// Unchecked: nruns <= copyblk::kMaxRuns, nunits <= copyblk::kMaxUnits.
constexpr int kCopyResFields = 1;
hipError_t launch_copy_runs(const uint64_t* runs, uint64_t nruns, uint64_t nunits, uint64_t* res,
                            hipStream_t s);
// The copy table of the blocks taken from resident buffers (copyblk.hip;
// cir_reload_blocks; the rule is copyblk::take_of): have (ceil(n_need / 64) u64,
// every word written) = the taken blocks, runs = their records in block order
// (none at or past cap_runs is written), res: copyblk::kPlanResFields u64
// {records, units, bytes, matches dropped for their length}, all written here,
// all on `s`.  work: copy_plan_work_bytes(n_need) bytes of scratch.  Unchecked:
// bs != 0, n_need < 2^32.
inline uint64_t copy_plan_tiles(uint64_t n_need) { return (n_need + 63) / 64; }
inline uint64_t copy_plan_work_bytes(uint64_t n_need) { return 16 * copy_plan_tiles(n_need) + 16; }
hipError_t launch_copy_plan(const copyblk::Plan& p, uint64_t* have, uint64_t* runs,
                            uint64_t cap_runs, uint64_t* work, uint64_t* res, hipStream_t s);

// The two copy tables and the bitmap of an image updated in the buffers that
// hold it (update.hip; cir_update_blocks; the rule is update.hpp), in two steps
// with the host's look at the counts between them.  launch_update_count:
// k_update_plan and k_update_scan; res: update::kResFields u64, zeroed here,
// of which the totals {A records, A units, B records, B units} and the
// candidates' totals are final afterwards; work: update_plan_work_bytes(n_need)
// bytes of scratch that launch_update_emit reads.  launch_update_emit
// (p.scratch set, at least 16 res[kBUnits] bytes): have (ceil(n_need / 64) u64,
// every word written) = the kept, direct and staged blocks, runs_a and runs_b =
// the records of phase 1 and phase 2 in block order (none at or past cap_runs
// is written), and the class counts added to res.  All on `s`.  Unchecked: bs
// != 0, n_need < 2^32, the resident table sorted by address and disjoint.
inline uint64_t update_plan_tiles(uint64_t n_need) { return (n_need + 63) / 64; }
inline uint64_t update_plan_work_bytes(uint64_t n_need) { return 32 * update_plan_tiles(n_need) + 32; }
hipError_t launch_update_count(const update::Plan& p, uint64_t* work, uint64_t* res, hipStream_t s);
hipError_t launch_update_emit(const update::Plan& p, const uint64_t* work, uint64_t cap_runs,
                              uint64_t* have, uint64_t* runs_a, uint64_t* runs_b, uint64_t* res,
                              hipStream_t s);

// nlanes x `lines` register-only compressions (diagnostic VALU ceiling).
hipError_t launch_compress_only(uint64_t nlanes, uint32_t lines, uint8_t* out, hipStream_t s);

// one wave reads the device's wall clock and shader clock counters around a
// spin of `spin` wall-clock ticks: out[0..3] = rt0, rt1, c0, c1 (device memory)
hipError_t launch_clock_probe(uint64_t* out, uint64_t spin, hipStream_t s);
hipError_t launch_fill_splitmix64(uint64_t* p, uint64_t nwords, uint64_t seed,
                                  uint64_t block_words, uint64_t first_block, hipStream_t s);

}  // namespace dev
}  // namespace cir
