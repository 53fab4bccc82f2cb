/*
 * ciruela_blockhash.h — C ABI of the MI355X (gfx950) block-indexing path.
 *
 * Drop-in boundary for ciruela's indexing loop.  Every entry
 * point names the reference interface it replaces (paths are relative to the
 * tailhook/ciruela v0.6.12 tree).  Every block digest is computed on the GPU
 * (hand-written HIP kernels for gfx950); the host side stages bytes and
 * bookkeeps, and by default hashes the one serial footer chain of a scanned
 * index (cir_set_footer_mode).  There is no CPU fallback for block hashes:
 * without a usable GPU every hashing call returns CIR_ENODEV.
 *
 * Conventions
 *   - return 0 (CIR_OK) on success, a negative CIR_E* code on failure; the
 *     detail of the last failure is in cir_last_error().  No call aborts the
 *     process on bad input it can check (the reference panics only on
 *     impossible states, e.g. src/block_id.rs:38,41 "length is ok").  The
 *     caller's own buffers are trusted, as a slice is in the reference: the
 *     descriptor batches (cir_hash_blocks[_dev][_ht], cir_verify_blocks[_dev])
 *     read arena + off[b] .. + len[b] as given (an out-of-range descriptor is
 *     a memory fault, on the GPU or the host), so descriptors derived from
 *     untrusted data go through the *_bounded entry points, which check
 *     every one against the arena's size (on the device for *_dev_bounded).
 *   - digests are 32 raw bytes (BlockHash([u8; 32]), src/block_id.rs:19),
 *     printed as lowercase hex (src/hexlify.rs:9-13).
 *   - `stream` arguments are hipStream_t passed as void* (NULL = the null
 *     stream of the calling thread's current device).  *_dev calls are
 *     asynchronous on that stream and never synchronise the device (with a
 *     context, a descriptor batch larger than any before grows the device's
 *     ordering or bounds scratch, waiting once for that scratch's previous
 *     user).
 *   - no call changes the calling thread's current HIP device: entry points
 *     that work on other devices restore it before returning.
 *   - buffers returned through `uint8_t**` are released with cir_free().
 *   - environment (read by the library; none is needed):
 *       CIR_STAGE_COPY=direct  host threads fill the pinned staging slots with
 *                              plain pread()/memcpy() instead of streaming
 *                              (non-temporal) stores;
 *       CIR_STAGE_RAMP=0       staged host paths start with whole-slot batches
 *                              (default: the first three batches ramp up from
 *                              1/8 of a slot, so the first upload starts
 *                              sooner);
 *       CIR_FOOTER=gpu         cir_init's contexts start with CIR_FOOTER_GPU;
 *       CIR_TRACE=1            per-batch timings on stderr;
 *       CIR_SOURCES_PARSE=host cir_block_sources with a context parses the index
 *                              texts on the host, as before the device parse
 *                              (cir_index_digests_dev) existed (A/B measurement);
 *       CIR_SOURCES_MAP=host   cir_block_sources / cir_block_extents with a context
 *                              map the join's matches back to files on a host
 *                              thread; =device: with cir_match_extents_dev's
 *                              kernels.  Unset: cir_block_extents on the device,
 *                              cir_block_sources on the device from 16,384
 *                              needed blocks on;
 *       CIR_LINKS_MATCH=host   cir_file_sources with a context answers with the host
 *                              rule of cir_link_candidates, and cir_file_copies with
 *                              its own host rule (A/B measurement; read per call);
 *       CIR_PLAN=host          cir_fetch_plan with a context answers with the host
 *                              composition of the four calls it is defined by (A/B
 *                              measurement; read per call);
 *       CIR_SKETCH=host        cir_index_sketch with a context answers with the host
 *                              rule (A/B measurement; read per call);
 *       CIR_DEBUG_SPLIT=k      (tests) every opened GPU appears k times.
 *       CIR_DEBUG_STRIPE_BLOCKS=n  (tests) a scan over several devices deals
 *                              stripes of n blocks (default: one staging
 *                              slot of whole blocks) round-robin to them.
 */
#ifndef CIRUELA_BLOCKHASH_H
#define CIRUELA_BLOCKHASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIR_DIGEST_BYTES 32
#define CIR_DEFAULT_BLOCK_SIZE 32768 /* src/daemon/disk/public.rs:154 */

/* Every int-returning call returns one of these (the text of the last
 * failure on this thread: cir_last_error).  No C++ exception leaves the
 * library: an allocation that fails inside it is CIR_ENOMEM. */
enum cir_status {
  CIR_OK = 0,
  CIR_EIO = -1,        /* filesystem error: scan's io::Error (src/client/sync/uploads.rs:57) */
  CIR_EINVAL = -2,     /* bad argument, length or shape */
  CIR_EHIP = -3,       /* HIP runtime error (hipError_t text in cir_last_error) */
  CIR_ENOMEM = -4,     /* host or device allocation failed */
  CIR_EPARSE = -5,     /* IndexError::ParseError (src/index.rs:64) / DirError::ParseError (src/blocks.rs:117) */
  CIR_ENOTFOUND = -6,  /* ReadError::NotFound (src/index.rs:78, src/blocks.rs:101) */
  CIR_EHASHSIZE = -7,  /* DirError::HashSize (src/blocks.rs:123) */
  CIR_ENODEV = -8,     /* no usable gfx950 device */
  CIR_EUNSUPPORTED = -9, /* reserved (every dir-signature hash type is implemented) */
  CIR_EAGAIN = -10       /* cir_verify_submit, non-blocking: the verify queue is full */
};

/* dir-signature HashType (external crate 0.2.9; header tokens in the index) */
enum cir_hash_type {
  CIR_HASH_BLAKE2B_256 = 1, /* HashType::blake2b_256()  "blake2b/256" */
  CIR_HASH_SHA512_256 = 2   /* HashType::sha512_256()   "sha512/256" */
};

typedef struct cir_ctx cir_ctx;

/* ---- context --------------------------------------------------------- */

/* Open the devices in device_mask (bit i = HIP device i; 0 = every visible
 * device; the devices are opened in parallel, one host thread each).
 * staging_bytes sizes each device's host->device staging slots for the
 * host-memory entry points (0 = 256 MiB).  What cir_init creates per device:
 * its streams (compute, copy, quad part, footer chain), the relay scratch,
 * the ordering scratch for one full staging batch and -- unless staging_bytes
 * is CIR_STAGING_LAZY -- three staging slots (pinned host + device memory of
 * staging_bytes each, plus descriptor and digest buffers).  A tiny warm-up
 * hash loads the kernels and the first copies on the staging and chain
 * streams are paid here.  Allocated later, on first use: the footer-chain
 * text buffers (cir_scan_v1 with CIR_FOOTER_GPU), the single-launch buffers
 * of cir_blake2b256, timing events, and -- with CIR_STAGING_LAZY -- the
 * staging slots (256 MiB each), so a context used only through the *_dev
 * entry points pins no staging memory.
 *
 * Cost per opened device, staging S (blocks per slot B = max(S / 512, 4096)):
 *   pinned host memory  3 x (S + 44 B)            = 834 MiB at the default
 *   device memory       3 x (S + 44 B) + 8 B + 4 MiB (ordering, relay)
 *                                                 = 842 MiB at the default
 *   with CIR_STAGING_LAZY: ~4.2 MiB of device memory and no pinned memory
 *   until a host path runs; plus, either way, the HIP runtime's own context
 *   on that device and cir_init's 0.1-0.3 s of start-up. */
#define CIR_STAGING_LAZY ((uint64_t)-1)
int cir_init(cir_ctx** ctx, uint32_t device_mask, uint64_t staging_bytes);
/* cir_init with a device-count hint: opens at most max_devices of the
 * devices device_mask selects, the lowest-numbered first (0 = no cap, as
 * cir_init).  With cir_devices_for_bytes a caller that knows how much input
 * it will stage opens only the devices that input can use.  flags: 0 or
 * CIR_INIT_ONE_SHOT. */
int cir_init_n(cir_ctx** ctx, uint32_t device_mask, uint64_t staging_bytes, uint32_t max_devices,
               uint32_t flags);
/* A context for one short job (the CLI's sync of an input that fits one
 * staging slot): each device gets ONE stream for its uploads and kernels and
 * one staging slot.  A HIP stream on a hardware queue of its own costs 8-10
 * ms to create in a fresh process (the first 19 ms; profiles/r05/
 * start_env.log), and the copy, footer-chain and quad-part streams were
 * ~25 ms of a 55 ms cir_init.  Every entry point still works: the other
 * slots are allocated and the footer-chain stream created if a call needs
 * them, uploads wait for the previous batch's kernels, and an ordered
 * batch's quad part runs behind its lane part instead of beside it (config
 * 3's mixed batch takes the sum of the two parts, not the longer). */
#define CIR_INIT_ONE_SHOT 1u
/* The devices worth opening for work_bytes of host-path input (a scan's
 * tree, a hash_file / hash_memory input): ceil(work_bytes / (2 x staging))
 * -- each device gets at least two staging batches, so its start-up and
 * pinned slots are not spent on a fraction of one -- capped at `visible`,
 * at least 1; work_bytes == 0 (unknown) gives `visible`.  staging_bytes as
 * cir_init's (0 / CIR_STAGING_LAZY = 256 MiB).  Pure: no HIP call. */
uint32_t cir_devices_for_bytes(uint64_t work_bytes, uint64_t staging_bytes, uint32_t visible);
void cir_destroy(cir_ctx* ctx);
int cir_device_count(void);
/* devices opened by ctx; ids[i] receives the HIP ordinal of the i-th. */
int cir_ctx_devices(const cir_ctx* ctx, int* ids, int max_ids);
const char* cir_strerror(int status);
const char* cir_last_error(void); /* thread-local detail of the last failure */
void cir_free(void* p);

/* ---- block hashes ---------------------------------------------------- */

/* BlockHash::hash_bytes(&[u8]) -> BlockHash   (src/block_id.rs:37-43).
 * Single host buffer, hashed on the process-default device context. */
int cir_blake2b256(const uint8_t* p, size_t n, uint8_t out[CIR_DIGEST_BYTES]);

/* Device-resident Hashes::hash_file: the bytes [d_data, d_data + nbytes) of
 * one file already in HBM, split into ceil(nbytes / block_size) blocks (the
 * last one short; none when nbytes == 0), digest i -> d_out + 32 i (d_out
 * 16-byte aligned, as hipMalloc returns it).  This is the metric path
 * (BASELINE.json configs 2 and 4).  With a context (ctx != NULL) parts of
 * the file may also run on the device's own quad-part stream (the short last
 * block; the blocks past a whole number of waves per SIMD), forked from and
 * joined back into `stream`, so the call is ordered on `stream` as one
 * launch would be; ctx == NULL: one launch on `stream`, no side streams. */
int cir_hash_chunks_dev(cir_ctx* ctx, const void* d_data, uint64_t nbytes, uint64_t block_size,
                        uint8_t* d_out, void* stream);

/* Device-resident batch of independent blocks: block b = d_arena[d_off[b] ..
 * d_off[b] + d_len[b]) -> d_out + 32 b (d_out 16-byte aligned).  Any order,
 * any mix of lengths (config 3); zero-length blocks hash as the empty input. */
int cir_hash_blocks_dev(cir_ctx* ctx, const void* d_arena, const uint64_t* d_off,
                        const uint32_t* d_len, size_t nblk, uint8_t* d_out, void* stream);

/* cir_hash_blocks_dev_ht for descriptors the caller cannot vouch for (the
 * daemon's received blocks, src/daemon/tracking/fetch_blocks.rs:77,91-103):
 * the arena is [d_arena, d_arena + arena_bytes), and block b is out of range
 * when d_off[b] + d_len[b] wraps around 2^64 or passes arena_bytes.  An
 * out-of-range block is not read (no kernel touches memory outside the
 * arena); its digest is 32 zero bytes and *d_nrange (device u32, may be
 * NULL) = the number of such blocks.  The other blocks' digests are exactly
 * cir_hash_blocks_dev_ht's.  Asynchronous on `stream` like the other *_dev
 * calls: the caller reads *d_nrange after its own synchronisation and treats
 * a non-zero count as CIR_EINVAL for those blocks.  Costs one extra pass
 * over the descriptors (12 B read, 5 B written per block) and, with a
 * context, a device scratch of ~5 B per block kept for the next call. */
int cir_hash_blocks_dev_bounded(cir_ctx* ctx, int hash_type, const void* d_arena,
                                uint64_t arena_bytes, const uint64_t* d_off, const uint32_t* d_len,
                                size_t nblk, uint8_t* d_out, uint32_t* d_nrange, void* stream);

/* Host-memory batch (same meaning as cir_hash_blocks_dev, host pointers);
 * staged through pinned buffers, split across the context's devices. */
int cir_hash_blocks(cir_ctx* ctx, const uint8_t* h_arena, const uint64_t* off,
                    const uint32_t* len, size_t nblk, uint8_t* h_out);

/* cir_hash_blocks_ht over host descriptors the caller cannot vouch for: the
 * arena is [h_arena, h_arena + arena_bytes); block b is out of range when
 * off[b] + len[b] wraps around 2^64 or passes arena_bytes.  Such a block is
 * never read; its digest is 32 zero bytes and *nrange_out (may be NULL) =
 * their number.  The other digests are exactly cir_hash_blocks_ht's; with
 * every block in range nothing is copied (one pass over the descriptors). */
int cir_hash_blocks_bounded(cir_ctx* ctx, int hash_type, const uint8_t* h_arena,
                            uint64_t arena_bytes, const uint64_t* off, const uint32_t* len,
                            size_t nblk, uint8_t* h_out, size_t* nrange_out);

/* dir_signature::v1::Hashes::hash_file(HashType::blake2b_256(), block_size,
 * reader)  (external; call sites src/blocks.rs:193,
 * src/cluster/download.rs:257).  Reads fd from its current offset to EOF.
 * *hashes_out = ceil(size / block_size) x 32 bytes (NULL when size == 0). */
int cir_hash_file(cir_ctx* ctx, int fd, uint64_t block_size, uint64_t* size_out,
                  uint8_t** hashes_out, size_t* nhash_out);

/* Hashes::hash_file over an in-memory reader (register_memory_blocks,
 * src/blocks.rs:187-204). */
int cir_hash_memory(cir_ctx* ctx, const uint8_t* data, uint64_t size, uint64_t block_size,
                    uint8_t** hashes_out, size_t* nhash_out);

/* ---- other hash types (dir-signature HashType) ------------------------ */

/* The entry points above with an explicit HashType (enum cir_hash_type):
 * Hashes::hash_file(hash_type, ...) is generic over the index's hash type
 * (src/cluster/download.rs:257 passes self.hash_type). */
int cir_sha512_256(const uint8_t* p, size_t n, uint8_t out[CIR_DIGEST_BYTES]);
int cir_hash_blocks_dev_ht(cir_ctx* ctx, int hash_type, const void* d_arena,
                           const uint64_t* d_off, const uint32_t* d_len, size_t nblk,
                           uint8_t* d_out, void* stream);
int cir_hash_blocks_ht(cir_ctx* ctx, int hash_type, const uint8_t* h_arena, const uint64_t* off,
                       const uint32_t* len, size_t nblk, uint8_t* h_out);
int cir_hash_file_ht(cir_ctx* ctx, int hash_type, int fd, uint64_t block_size,
                     uint64_t* size_out, uint8_t** hashes_out, size_t* nhash_out);
int cir_hash_memory_ht(cir_ctx* ctx, int hash_type, const uint8_t* data, uint64_t size,
                       uint64_t block_size, uint8_t** hashes_out, size_t* nhash_out);

/* ---- verification (the daemon side of the same hash) ------------------ */

/* FetchBlock::poll's `BlockHash::hash_bytes(&data.data) == blk.hash`
 * (src/daemon/tracking/fetch_blocks.rs:77) over a device-resident batch of
 * received blocks: the blocks are hashed (as cir_hash_blocks_dev_ht) into
 * d_digests (32 x nblk bytes of scratch) and compared with d_expected on the
 * same stream.  d_ok[b] = 1 when block b matches, 0 when it does not (the
 * reference then retries the block elsewhere, :91-103); *d_nbad (device
 * u32) = number of mismatches.  d_ok / d_nbad may be NULL.  d_expected and
 * d_digests must be 16-byte aligned. */
int cir_verify_blocks_dev(cir_ctx* ctx, int hash_type, const void* d_arena, const uint64_t* d_off,
                          const uint32_t* d_len, size_t nblk, const uint8_t* d_expected,
                          uint8_t* d_digests, uint8_t* d_ok, uint32_t* d_nbad, void* stream);

/* cir_verify_blocks_dev over untrusted descriptors, as
 * cir_hash_blocks_dev_bounded checks them: an out-of-range block (d_off[b] +
 * d_len[b] wraps or passes arena_bytes) is never read and counts as a
 * mismatch -- d_ok[b] = 0, included in *d_nbad -- so the caller re-fetches
 * it as it would a corrupted block (fetch_blocks.rs:91-103); its
 * d_digests entry is 32 zero bytes. */
int cir_verify_blocks_dev_bounded(cir_ctx* ctx, int hash_type, const void* d_arena,
                                  uint64_t arena_bytes, const uint64_t* d_off,
                                  const uint32_t* d_len, size_t nblk, const uint8_t* d_expected,
                                  uint8_t* d_digests, uint8_t* d_ok, uint32_t* d_nbad,
                                  void* stream);

/* cir_verify_blocks_dev, answering only "which block first": *d_first (device u64) = smallest b
 * whose digest differs from d_expected (or is out of range: pass arena_bytes = UINT64_MAX for
 * trusted descriptors), UINT64_MAX when none; *d_nbad (device u32, may be NULL) = how many.
 * Both are written on `stream` by the call itself (the caller initialises nothing; nblk == 0
 * writes UINT64_MAX and 0), no per-block result is stored, and a batch without a mismatch
 * issues no atomic.  Alignment and CIR_EINVAL cases as cir_verify_blocks_dev_bounded; d_first
 * must not be NULL. */
int cir_verify_first_dev(cir_ctx* ctx, int hash_type, const void* d_arena, uint64_t arena_bytes,
                         const uint64_t* d_off, const uint32_t* d_len, size_t nblk,
                         const uint8_t* d_expected, uint8_t* d_digests,
                         uint64_t* d_first, uint32_t* d_nbad, void* stream);

/* cir_verify_first_dev with one verdict per segment instead of "which block first": the
 * compare behind cir_check_links (try_hardlink, src/daemon/disk/public.rs:285-346, where a bad
 * candidate never affects another, :303).  Segment s is the blocks [d_seg_end[s-1],
 * d_seg_end[s]) with d_seg_end[-1] = 0; d_seg_end (device u32 x nseg) is non-decreasing, empty
 * segments are allowed and d_seg_end[nseg-1] == nblk.  d_seg_bad[s] (device bytes x nseg) = 1
 * when any block of s mismatches d_expected or is out of range (arena_bytes = UINT64_MAX:
 * trusted descriptors), else 0; *d_nbad_seg (device u32, may be NULL) = the number of bad
 * segments.  Every flag and the count are written on `stream` by the call itself (the caller
 * initialises nothing; nblk == 0 writes zeros and 0), no digest travels back, a wave without a
 * mismatch issues no store, and a mismatching block's segment index is clamped to [0, nseg), so
 * nothing outside d_seg_bad[0 .. nseg) is written whatever d_seg_end holds.  CIR_EINVAL: a
 * NULL d_seg_end or d_seg_bad, nseg == 0 with nblk > 0, and the alignment and argument cases
 * of cir_verify_first_dev (d_seg_end and d_nbad_seg 4-byte aligned). */
int cir_verify_segments_dev(cir_ctx* ctx, int hash_type, const void* d_arena, uint64_t arena_bytes,
                            const uint64_t* d_off, const uint32_t* d_len, size_t nblk,
                            const uint8_t* d_expected, uint8_t* d_digests,
                            const uint32_t* d_seg_end, size_t nseg,
                            uint8_t* d_seg_bad, uint32_t* d_nbad_seg, void* stream);

/* cir_verify_first_dev with one bit per block instead of "which block first": the compare
 * behind cir_check_blocks.  Bit (b & 63) of d_have[b >> 6] (device u64 x ceil(nblk / 64),
 * 8-byte aligned, never NULL) = 1 when block b hashes to d_expected[32 b ..) and is in range
 * (arena_bytes = UINT64_MAX: trusted descriptors); an out-of-range block is never read and its
 * bit is 0.  Every word of [0, ceil(nblk / 64)) is written on `stream` by the call itself, the
 * bits of the last word at positions >= nblk as 0, and nothing past that word is written; the
 * caller initialises nothing and no atomic touches the bitmap.  *d_nbad (device u32, may be
 * NULL) = the number of blocks whose bit is 0, written by the call (nblk == 0 writes only
 * *d_nbad = 0).  CIR_EINVAL: a NULL or misaligned d_have and the alignment and argument cases
 * of cir_verify_first_dev. */
int cir_verify_bitmap_dev(cir_ctx* ctx, int hash_type, const void* d_arena, uint64_t arena_bytes,
                          const uint64_t* d_off, const uint32_t* d_len, size_t nblk,
                          const uint8_t* d_expected, uint8_t* d_digests, uint64_t* d_have,
                          uint32_t* d_nbad, void* stream);

/* Host-memory batch of the same check; ok_out (nblk bytes) may be NULL. */
int cir_verify_blocks(cir_ctx* ctx, int hash_type, const uint8_t* h_arena, const uint64_t* off,
                      const uint32_t* len, size_t nblk, const uint8_t* expected, uint8_t* ok_out,
                      size_t* nbad_out);

/* cir_verify_blocks over untrusted host descriptors (checked as
 * cir_hash_blocks_bounded checks them): an out-of-range block is never read
 * and is a mismatch (ok_out[b] = 0, counted in *nbad_out). */
int cir_verify_blocks_bounded(cir_ctx* ctx, int hash_type, const uint8_t* h_arena,
                              uint64_t arena_bytes, const uint64_t* off, const uint32_t* len,
                              size_t nblk, const uint8_t* expected, uint8_t* ok_out,
                              size_t* nbad_out);

/* The same check one block at a time, asynchronously, for a caller that
 * receives blocks one by one (FetchBlock::poll, fetch_blocks.rs:77):
 * cir_verify_submit copies the block (once, into the arena of the batch
 * being formed) with its expected digest and returns a ticket; a worker
 * thread of the context verifies each batch as one host batch once it is full
 * or a short window after its first block (default 200 us, at most 4096
 * blocks, one hash type per batch).  cir_verify_poll: *state = 0 pending,
 * 1 match, 2 mismatch (the outcome is consumed when reported).
 * cir_verify_wait blocks: *ok = 1 match, 0 mismatch.  A failed batch returns
 * its error for each of its tickets.  An unknown, consumed, forgotten or
 * expired ticket is CIR_ENOTFOUND.  cir_verify_window sets the window
 * (microseconds) and the batch cap.
 *
 * Bounds (cir_verify_limits; 0 = the default):
 *   max_bytes    block bytes accepted and not yet verified (default 256 MiB).
 *                It bounds admission only: a batch's arena holds min(half of
 *                it, 128 MiB), so a large bound allocates nothing up front.  A submit that
 *                would pass it waits until the worker has verified enough,
 *                or with flags = CIR_VERIFY_NONBLOCK returns CIR_EAGAIN (the
 *                block is not taken: retry later or elsewhere).  A block
 *                larger than max_bytes is taken once nothing else is held.
 *   max_results  finished outcomes held for tickets not yet polled, waited
 *                or forgotten (default 2^20); beyond it the oldest tickets'
 *                outcomes are dropped (they become CIR_ENOTFOUND, counted as
 *                expired).
 * cir_verify_forget drops a ticket the caller no longer wants (a block the
 * reference would re-fetch elsewhere, :91-103): a pending one is still
 * hashed with its batch but its outcome is never held; a finished one's
 * outcome is released.
 * cir_verify_stats: out[0] bytes held (accepted, not yet verified), [1] the
 * peak of [0], [2] pending tickets, [3] outcomes held, [4] outcomes
 * expired, [5] tickets forgotten, [6] submits refused with CIR_EAGAIN,
 * [7] batches verified. */
#define CIR_VERIFY_NONBLOCK 1
#define CIR_VERIFY_STATS_FIELDS 8
int cir_verify_submit(cir_ctx* ctx, int hash_type, const uint8_t* data, size_t n,
                      const uint8_t expected[CIR_DIGEST_BYTES], uint64_t* ticket);
int cir_verify_poll(cir_ctx* ctx, uint64_t ticket, int* state);
int cir_verify_wait(cir_ctx* ctx, uint64_t ticket, int* ok);
int cir_verify_forget(cir_ctx* ctx, uint64_t ticket);
int cir_verify_window(cir_ctx* ctx, uint32_t window_us, uint32_t max_batch);
int cir_verify_limits(cir_ctx* ctx, uint64_t max_bytes, uint64_t max_results, int flags);
int cir_verify_stats(cir_ctx* ctx, uint64_t out[CIR_VERIFY_STATS_FIELDS]);

/* Hashes::check_file(&mut file) at image commit (src/daemon/disk/commit.rs:
 * 104; false -> Error::Checksum, :110): re-hash fd from its current offset to
 * EOF in block_size blocks; *ok_out = 1 iff the file has exactly nhash
 * blocks and every digest equals expected[32 i .. 32 i + 32]. */
int cir_check_file(cir_ctx* ctx, int hash_type, int fd, uint64_t block_size,
                   const uint8_t* expected, size_t nhash, int* ok_out);

/* The re-hash loop of commit_image (src/daemon/disk/commit.rs:51-117) over a whole image in
 * one call: every file the index lists is read through the scan's staging pipeline, hashed and
 * compared with the index's digests on the device, and only "which block first" comes back.
 * The image root is `dir`, opened relative to dirfd (AT_FDCWD allowed; dir == NULL: dirfd
 * itself); hash type and block size come from the index header; threads as in cir_scan_v1.
 *
 * Returns CIR_OK whenever the check ran to a verdict, "a file is bad" included: *kind_out =
 * CIR_CHECK_OK (*path_out = NULL), CIR_CHECK_CHECKSUM (Error::Checksum, :81 / :110) or
 * CIR_CHECK_READ (Error::ReadFile, :74-78 / :98-106) for the first failing entry in index
 * order, as the reference's serial loop would meet it, with its path (the index's, unescaped
 * raw bytes, no terminator) in *path_out / *path_len (malloc'd: cir_free).  CIR_EINVAL: null
 * arguments; CIR_EPARSE / CIR_EHASHSIZE: the index does not parse; CIR_EIO: the root cannot
 * be opened.
 *
 * Read-only: nothing is created, no mode or timestamp changes (those parts of commit_image
 * stay the caller's).  Directories are opened one component at a time (O_DIRECTORY |
 * O_NOFOLLOW) below the root fd and files with openat(O_NOFOLLOW) in theirs, so no entry is
 * reached through a symlink.  Symlink entries, files the index does not list and the index's
 * footer are not examined.  A size-0 entry passes when it does not exist (the caller creates
 * it, :63) and is CHECKSUM when it is anything but an empty regular file; a file that cannot
 * be opened, is not regular, fails to read or shrinks while read is READ (errno in stats[6]);
 * one whose length differs from the index's is CHECKSUM without being read.
 *
 * stats ([0]-[4] defined for CIR_CHECK_OK only): [0] non-empty files hashed, [1] blocks
 * hashed, [2] bytes read, [3] batches, [4] size-0 entries examined, [5] peak of the file
 * descriptors the check held at once (O(reader threads), whatever the batch holds), [6]
 * errno of a READ verdict else 0, [7] global index (in index order) of the first bad block,
 * or UINT64_MAX. */
enum cir_check_kind { CIR_CHECK_OK = 0, CIR_CHECK_CHECKSUM = 1, CIR_CHECK_READ = 2 };
#define CIR_CHECK_STATS_FIELDS 8
int cir_check_index(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                    uint32_t threads, int* kind_out, uint8_t** path_out, size_t* path_len,
                    uint64_t stats[CIR_CHECK_STATS_FIELDS]);

/* scan_links (src/daemon/metadata/hardlink_sources.rs:107-153): which files of a new image
 * may be hardlinked from older images of the same base directory.  `index` is the new image's
 * index, src_index[j] / src_len[j] (j < nsrc) the older images' in the order the caller ranks
 * them (the reference: newest first, :66-72).  Every file entry of `index` is visited in index
 * order -- file ordinals count the file entries only, from 0 -- and for each the sources in the
 * order given: a source matches when it lists a file at the same path with equal exe flag, size
 * and digests (:131-133; a symlink or a directory at that path does not match), and the first
 * match makes the candidate (file ordinal, source ordinal) and ends the entry's search (the
 * break at :143).  So there is at most one candidate per file and file_out is strictly
 * increasing.  *file_out / *src_out hold *n_out values each (malloc'd: cir_free; NULL when
 * *n_out == 0).  A source that does not parse (the reference skips it with a warning, :95-101)
 * or whose hash type or block size is not the new index's takes no part and is counted in
 * *nskipped_out (may be NULL).  CIR_EPARSE / CIR_EHASHSIZE: `index` does not parse;
 * CIR_EINVAL: null arguments.  Host only.  (The reference walks the sources through the
 * MergedSignatures iterator of the external dir-signature crate, which is not in its tree:
 * the matching rule above is what :121-146 show of it.) */
int cir_link_candidates(const uint8_t* index, size_t len,
                        const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                        uint64_t** file_out, uint32_t** src_out, size_t* n_out,
                        size_t* nskipped_out);

/* check_and_hardlink's verify (try_hardlink, src/daemon/disk/public.rs:285-346) over every
 * candidate in one call: candidate i is file entry link_file[i] of `index` (an ordinal as in
 * cir_link_candidates; need not be sorted or unique), looked for at the entry's path under
 * source root link_src[i] -- src_dir[j] opened relative to src_dirfd[j] (AT_FDCWD allowed;
 * src_dir[j] == NULL: src_dirfd[j] itself).  The candidates go through cir_check_index's
 * staging pipeline without its stop at the first failure: a batch carries a segment table (one
 * segment = one candidate's run of blocks in the batch), cir_verify_segments_dev's compare
 * answers per segment and only one flag byte per segment and a count come back.  Hash type and
 * block size come from the index header; threads as in cir_scan_v1.
 *
 * Each candidate gets its verdict in isolation, in kind_out[i] (a cir_check_kind), with the
 * errno of a READ in errno_out[i] (may be NULL; else 0):
 *   CIR_CHECK_READ      the source root or a directory component cannot be opened (:315-319;
 *                       components one at a time, O_DIRECTORY | O_NOFOLLOW), the file cannot
 *                       be opened with openat(O_NOFOLLOW) in its directory (:322), is not
 *                       regular, fails to read (:324), or changes identity (st_dev, st_ino,
 *                       st_size) between the packer's look and the read.  A root that does not
 *                       open makes READ of its candidates, not a failed call.
 *   CIR_CHECK_CHECKSUM  (when not READ) the length is not the index's (the file is not read),
 *                       a block digest differs (:326), or st_mode & 0777 is not 0755 for an
 *                       exe entry, 0644 otherwise (:331-338; found by the packer's fstat, and
 *                       such a file is not read either).
 *   CIR_CHECK_OK        otherwise.
 * A size-0 candidate is examined on the host alone: it must exist as an empty regular file of
 * the right mode (a missing one is READ: there is nothing to link, unlike cir_check_index's
 * "absent passes").
 *
 * Read-only: nothing is linked, created or chmod'ed (link(2) and ensure_path, :340-342, stay
 * the caller's).  File descriptors held at once: the roots, one directory and one file per
 * packer and per reader thread.  Several devices take stripes of the candidates' block order;
 * every candidate is independent, so the verdicts do not depend on timing.
 *
 * Returns CIR_OK whenever every candidate got a verdict.  CIR_EINVAL (before any I/O): null
 * arguments, link_file[i] past the last file entry, link_src[i] >= nsrc; CIR_EPARSE /
 * CIR_EHASHSIZE as cir_check_index.
 *
 * stats: [0] candidates OK, [1] CHECKSUM, [2] READ, [3] blocks hashed, [4] bytes read, [5]
 * batches, [6] peak of the file descriptors held at once, [7] size-0 candidates examined. */
#define CIR_LINKS_STATS_FIELDS 8
int cir_check_links(cir_ctx* ctx, const uint8_t* index, size_t len,
                    const int* src_dirfd, const char* const* src_dir, size_t nsrc,
                    const uint64_t* link_file, const uint32_t* link_src, size_t nlinks,
                    uint32_t threads, uint8_t* kind_out, int32_t* errno_out,
                    uint64_t stats[CIR_LINKS_STATS_FIELDS]);

/* cir_check_links with a place per candidate: candidate i is still file entry link_file[i] of
 * `index` -- the size, the exe mode bits and the digests expected are that entry's -- but it is
 * looked for under source root link_src[i] at the path link_paths[link_path_off[i] ..
 * link_path_off[i + 1]) (raw bytes, nlinks + 1 offsets, no terminators): exactly what
 * cir_file_copies returns in paths_out / path_off_out, so a file an older image holds unchanged
 * below a renamed directory is verified where it actually lies.  An empty path means the entry's
 * own path; link_path_off == NULL makes the call cir_check_links.  The pipeline, the verdicts,
 * the stats, the bound on file descriptors and the striping over devices are cir_check_links';
 * the work order is by root, then by directory, then by index order, so neighbours still share a
 * directory fd.
 *
 * The paths come from another party's index and are validated before any I/O: a path is split at
 * '/', a leading '/' is allowed and empty components are dropped; a "." or ".." component, or a
 * non-empty path without any component, makes the whole call CIR_EINVAL with no file opened; a
 * component that holds a NUL byte makes CIR_CHECK_READ with EINVAL of that candidate alone.  Every
 * component is opened with O_DIRECTORY | O_NOFOLLOW below the root fd and the file with
 * O_NOFOLLOW, as in cir_check_links: a symlink in any component's place is READ.
 *
 * CIR_EINVAL additionally: link_path_off that decreases, a null link_paths with a non-empty
 * path. */
int cir_check_links_at(cir_ctx* ctx, const uint8_t* index, size_t len,
                       const int* src_dirfd, const char* const* src_dir, size_t nsrc,
                       const uint64_t* link_file, const uint32_t* link_src,
                       const uint64_t* link_path_off, const uint8_t* link_paths, size_t nlinks,
                       uint32_t threads, uint8_t* kind_out, int32_t* errno_out,
                       uint64_t stats[CIR_LINKS_STATS_FIELDS]);

/* Which blocks of an index a partial image directory already holds, for resume and repair.
 * The reference resumes by starting over: "Resuming download" (src/daemon/tracking/mod.rs:
 * 561-585) goes through start_image, which removes the partial .tmp directory
 * (src/daemon/disk/public.rs:91-93), and fill_blocks queues every block of every file again
 * (src/daemon/tracking/progress.rs:129-170).  Here the directory stays and the caller queues
 * only the blocks whose bit is 0.
 *
 * Root, hash type, block size and threads as in cir_check_index.  Blocks are numbered globally
 * in index order over the file entries (the numbering of cir_check_index's stats[7]), files by
 * file ordinal as in cir_link_candidates.  *have_out: one bit per block (bit (g & 63) of word
 * g >> 6; ceil(*nblk_out / 64) words); *state_out: one cir_file_state per file entry
 * (*nfiles_out of them), with CIR_FILE_LONG or'ed in; *errno_out (errno_out may be NULL): the
 * errno of a BLOCKED file, else 0.  All malloc'd (cir_free), NULL when their count is 0.
 *
 * Bit g is 1 exactly when the entry's path -- every directory component opened with
 * openat(O_DIRECTORY | O_NOFOLLOW) below the root, the file with openat(O_NOFOLLOW) -- is a
 * regular file, block j's bytes [j bs, min((j + 1) bs, size)) lie wholly inside the file's
 * current length, and their digest is the index's.  A block that reaches past EOF is not read;
 * a hole reads as zeros and is judged like any other bytes.
 *
 *   CIR_FILE_ABSENT    ENOENT on the file or on a directory component.
 *   CIR_FILE_BLOCKED   anything else keeps the file from being opened, something that is not a
 *                      regular file is in its place, a read fails, or the file changes
 *                      identity (st_dev, st_ino) or shrinks (ESTALE / ENODATA) between the
 *                      packer's look and the read.  None of the file's bits is set (the caller
 *                      removes the object and fetches the whole file); other files are
 *                      unaffected.
 *   CIR_FILE_COMPLETE  every block has its bit and the length is the entry's.
 *   CIR_FILE_PARTIAL   otherwise.
 *   CIR_FILE_LONG      or'ed into PARTIAL when the file is longer than the entry: the caller
 *                      truncates it before commit; its blocks up to the entry's size are
 *                      judged all the same (all of them may have their bits).
 * A size-0 entry is judged by the host alone: COMPLETE when an empty regular file is there,
 * ABSENT when nothing is, PARTIAL | LONG when it is regular and not empty, else BLOCKED.  Mode
 * bits are not examined (commit sets them).  cir_check_index gives CIR_CHECK_OK on the same
 * directory exactly when every non-empty file is COMPLETE and every size-0 file COMPLETE or
 * ABSENT.
 *
 * The pipeline is cir_check_links': the blocks inside each file's length are packed into the
 * staging slots, hashed, compared by cir_verify_bitmap_dev's kernel, and 16 + 8 ceil(n / 64)
 * bytes come back per batch of n blocks.  Read-only: nothing is created, truncated or
 * chmod'ed.  File descriptors held at once: the root, one directory and one file per packer
 * and per reader thread.  Several devices take stripes of the global block order; every block
 * has one owner, so the result does not depend on timing.
 *
 * Returns CIR_OK whenever every block and file got a verdict.  CIR_EINVAL / CIR_EPARSE /
 * CIR_EHASHSIZE (before any I/O) as cir_check_index; CIR_EIO only when the root cannot be
 * opened.
 *
 * stats: [0] blocks have, [1] blocks not have, [2] files COMPLETE, [3] ABSENT, [4] PARTIAL,
 * [5] BLOCKED, [6] bytes read, [7] batches, [8] peak of the file descriptors held at once,
 * [9] blocks not read because the file is absent or blocked or the block lies past EOF. */
enum cir_file_state {
  CIR_FILE_COMPLETE = 0,
  CIR_FILE_ABSENT = 1,
  CIR_FILE_PARTIAL = 2,
  CIR_FILE_BLOCKED = 3
};
#define CIR_FILE_LONG 0x80 /* or'ed in: on-disk length exceeds the entry's */
#define CIR_FILE_SKIPPED 4 /* cir_load_blocks only: a non-empty entry without a destination */
#define CIR_BLOCKS_STATS_FIELDS 10
int cir_check_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                     uint32_t threads, uint64_t** have_out, uint64_t* nblk_out,
                     uint8_t** state_out, int32_t** errno_out, size_t* nfiles_out,
                     uint64_t stats[CIR_BLOCKS_STATS_FIELDS]);

/* The scatter of cir_load_blocks on its own: packed runs of one source buffer copied to their
 * places.  The reference has no counterpart.  The rule is ciruela_amd/csrc/scatter.hpp.
 *
 * Table: nruns records of CIR_SCATTER_RUN_WORDS u64 {unit_first, src_pos, dst, bytes}: `bytes`
 * (> 0) bytes at byte src_pos of the source (a multiple of 16) go to the address dst (any
 * alignment).  A record has ceil(bytes / 16) units of 16 bytes; unit_first is the unit count of
 * all earlier records and nunits that of the whole table.  For every sound record the bytes
 * src[src_pos, src_pos + bytes) stand at dst afterwards, and no other byte is written: a unit
 * stores only its own bytes, so the destinations of different records must not overlap and need
 * no padding.
 *
 * res[0] = the bad records: src_pos not a multiple of 16, bytes 0, a source range outside [0,
 * src_bytes), or a unit_first that is not the previous record's plus its units (0 for the first
 * record; the last record must end at nunits).  A bad record is written nowhere and read nowhere;
 * the count is exact whatever the table holds.
 *
 * cir_scatter_runs is the host form (dst: host addresses; pure, host-only).  CIR_EINVAL: a null
 * pointer with a non-zero count, a null res, nruns or nunits above 2^32 - 1. */
#define CIR_SCATTER_RUN_WORDS 4
#define CIR_SCATTER_RES_FIELDS 1
int cir_scatter_runs(const uint8_t* src, uint64_t src_bytes, const uint64_t* runs, uint64_t nruns,
                     uint64_t nunits, uint64_t res[CIR_SCATTER_RES_FIELDS]);

/* The same on the device: source, table and destinations in device memory (d_src 16-byte
 * aligned, d_runs and d_res 8-byte aligned).  One lane per unit: one 16-byte load from the source
 * (a unit that reaches past src_bytes loads its bytes singly), one 16-byte store where the unit
 * is whole and its destination 16-byte aligned, narrower stores otherwise; no atomic touches a
 * destination.  Every word of d_res[CIR_SCATTER_RES_FIELDS] is written (a memset and one launch;
 * no launch for an empty table).  Like every *_dev call it allocates nothing, synchronises
 * nothing and runs on `stream` alone; ctx may be NULL and is not used.  CIR_EINVAL, decided
 * before any HIP call: as cir_scatter_runs, or a misaligned pointer. */
int cir_scatter_runs_dev(cir_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes,
                         const uint64_t* d_runs, uint64_t nruns, uint64_t nunits, uint64_t* d_res,
                         void* stream);

/* cir_check_blocks that keeps what it read: an image directory read into device memory,
 * verified.  The way back from cir_index_memory_dev; the reference has no counterpart (its
 * consumers read committed files from disk unchecked: commit_image, src/daemon/disk/commit.rs:
 * 51-117, is the last look at the bytes).
 *
 * Root, hash type, block size, threads, block numbering, file ordinals, *have_out, *state_out and
 * *errno_out are exactly cir_check_blocks'.
 *
 * Destinations: d_data[i] belongs to file ordinal i; ndata must be the index's file entries,
 * else CIR_EINVAL after the parse and before any I/O.  Each is at least the entry's size, of any
 * alignment, on the device of `stream`, which must be one of ctx's.  For a size-0 entry d_data[i]
 * is ignored (the host judges the entry as in cir_check_blocks).  A non-empty entry with
 * d_data[i] == NULL is not looked at, not opened and not read: its bits are 0 and its state is
 * CIR_FILE_SKIPPED (each rank of a job loads its own shard files).
 *
 * Afterwards the bytes of every block that was read -- exactly the blocks cir_check_blocks would
 * have read -- stand at d_data[file] + j * block_size, and the block's bit says whether those
 * bytes are the index's: a COMPLETE file's buffer is the file.  Bytes of blocks that were not
 * read are untouched; a file that is not COMPLETE has unspecified content in the positions of
 * the blocks that were read.  Nothing is written outside [d_data[i], d_data[i] + size_i).
 *
 * Stream order: before the first batch the device's compute stream waits for an event recorded
 * on `stream`, so whatever the caller queued there before the call -- a producer or an earlier
 * user of the buffers -- is finished before the first byte lands.  The call returns after all
 * its batches are done: the caller needs no synchronise afterwards.  The caller's current device
 * is restored.
 *
 * One device: the whole image goes through the device state that owns `stream`'s device (no
 * striping: the destinations live on one device).  The pipeline is cir_check_blocks' with one
 * scatter record per packed run added to each batch: the packed slot stays the unit of upload,
 * and behind the compare cir_scatter_runs_dev's kernel moves the batch's runs from the slot's
 * device twin to the destinations, inside device memory, while the next batch uploads.
 * CIR_TRACE=1 prints cir_check_blocks' laps and the scatter records per batch.
 *
 * CIR_EINVAL / CIR_EPARSE / CIR_EHASHSIZE / CIR_EIO as cir_check_blocks, and CIR_EINVAL for a
 * wrong ndata, a null d_data, a device that is not ctx's; CIR_EIO when the scatter counted a bad
 * record (the table is the call's own: a defect).
 *
 * stats: [0..9] as cir_check_blocks (SKIPPED files are in none of [2..5], their blocks count as
 * not have and not in [9]), [10] bytes scattered, [11] files SKIPPED. */
#define CIR_LOAD_STATS_FIELDS 12
int cir_load_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                    uint32_t threads, void* const* d_data, size_t ndata, void* stream,
                    uint64_t** have_out, uint64_t* nblk_out, uint8_t** state_out,
                    int32_t** errno_out, size_t* nfiles_out,
                    uint64_t stats[CIR_LOAD_STATS_FIELDS]);

/* The gather of cir_store_blocks on its own: bytes that lie anywhere copied into the packed runs
 * of one destination buffer.  cir_scatter_runs turned round; the reference has no counterpart.
 * The rule is ciruela_amd/csrc/gather.hpp.
 *
 * Table: nruns records of CIR_GATHER_RUN_WORDS u64 {unit_first, dst_pos, src, bytes}: `bytes`
 * (> 0) bytes at the address src (any alignment) go to byte dst_pos of the destination (a
 * multiple of 16).  A record has ceil(bytes / 16) units of 16 bytes; unit_first is the unit count
 * of all earlier records and nunits that of the whole table.  A unit owns its 16 aligned
 * destination bytes and writes all of them: for every sound record the bytes at src stand at
 * dst[dst_pos, dst_pos + bytes) afterwards, zeros behind them up to the next multiple of 16, and
 * no other byte is written.  Nothing is read outside [src, src + bytes).  The sources must not
 * overlap the destination.
 *
 * res[0] = the bad records: dst_pos not a multiple of 16, bytes 0, a range [dst_pos, dst_pos +
 * 16 * ceil(bytes / 16)) that does not lie inside [0, dst_bytes], or a unit_first that is not the
 * previous record's plus its units (0 for the first record; the last record must end at nunits).
 * A bad record is written nowhere and read nowhere; the count is exact whatever the table holds.
 *
 * cir_gather_runs is the host form (src: host addresses; pure, host-only).  CIR_EINVAL: a null
 * pointer with a non-zero count, a null res, nruns or nunits above 2^32 - 1. */
#define CIR_GATHER_RUN_WORDS 4
#define CIR_GATHER_RES_FIELDS 1
int cir_gather_runs(uint8_t* dst, uint64_t dst_bytes, const uint64_t* runs, uint64_t nruns,
                    uint64_t nunits, uint64_t res[CIR_GATHER_RES_FIELDS]);

/* The same on the device: destination, table and sources in device memory (d_dst 16-byte
 * aligned, d_runs and d_res 8-byte aligned).  One lane per unit: always one 16-byte store; a whole
 * unit is loaded with one 16-byte load where its source is 16-byte aligned and with the widest
 * loads the source's alignment allows otherwise, a short last unit byte by byte.  Every word of
 * d_res[CIR_GATHER_RES_FIELDS] is written (a memset and one launch; no launch for an empty
 * table).  Like every *_dev call it allocates nothing, synchronises nothing and runs on `stream`
 * alone; ctx may be NULL and is not used.  CIR_EINVAL, decided before any HIP call: as
 * cir_gather_runs, or a misaligned pointer. */
int cir_gather_runs_dev(cir_ctx* ctx, uint8_t* d_dst, uint64_t dst_bytes, const uint64_t* d_runs,
                        uint64_t nruns, uint64_t nunits, uint64_t* d_res, void* stream);

/* cir_load_blocks mirrored: files held in device memory written out as an image directory, and
 * the directory's index.  The reference has no counterpart (an image directory is filled block by
 * block from the network, src/daemon/disk/public.rs write_block; its index comes from a scan).
 *
 * The file list -- paths, path_off, sizes, exe, nfiles, d_data --, the path rules and every
 * CIR_EINVAL case are cir_index_memory_dev's (a null ctx, a device that is not ctx's, a null
 * pointer of a non-empty file, an invalid path or a path conflict, a bad block size or hash
 * type); all of them are decided before anything is created on disk and before any device work.
 * The root is dirfd + dir as in cir_check_blocks and must exist.
 *
 * The tree: the directories the paths imply are made with mkdirat below their parent's fd (an
 * existing directory is accepted) and opened with O_DIRECTORY | O_NOFOLLOW; every file is created
 * with openat(O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW) and fchmod'ed to exactly 0644, or 0755
 * where exe is set; a size-0 file is created empty.  Nothing is fsync'ed, and renaming a
 * temporary root into place stays the caller's.  CIR_EIO with the path and errno in
 * cir_last_error: a root that cannot be opened, a file that exists, a symlink at any component, a
 * write error.  The first such failure ends the call; what was written is left for the caller to
 * remove.  Nothing is ever written through a symlink or outside the root.
 *
 * Pipeline: cir_load_blocks' the other way, on the device of `stream`.  The files' runs are laid
 * out in a staging slot in the caller's file order, one gather record per run; cir_gather_runs_dev's
 * kernel fills the slot's device twin from d_data, the slot is hashed there, and its bytes and
 * digests come down as one copy each per batch; `threads` writers (0: chosen by the library)
 * pwrite the runs from the pinned slot while the next slots gather and download.  Before the
 * first batch the device's compute stream waits for an event recorded on `stream`, so whatever the
 * caller queued there to produce the data is finished before the first byte is read.  The call
 * returns after its last write; the caller's current device is restored.  CIR_TRACE=1 prints one
 * `cir store_blocks:` line with the laps.
 *
 * The index: made by cir_index_emit's emitter from the digests of the slots' bytes, the bytes
 * that were written.  *index_out (cir_free) and image_id are byte-identical to
 * cir_index_memory_dev's of the same list and so to cir_scan_v1's of the written tree:
 * cir_check_index(root, *index_out) passes by construction.
 *
 * CIR_EIO also when the gather counted a bad record (the table is the call's own: a defect).
 *
 * stats (all written as 0 first): [0] blocks, [1] files written, [2] directories made, [3] bytes
 * written, [4] batches, [5] body bytes. */
#define CIR_STORE_STATS_FIELDS 6
int cir_store_blocks(cir_ctx* ctx, int dirfd, const char* dir, int hash_type, uint64_t block_size,
                     const uint8_t* paths, const uint64_t* path_off, const uint64_t* sizes,
                     const uint8_t* exe, size_t nfiles, const void* const* d_data, void* stream,
                     uint32_t threads, uint8_t** index_out, size_t* len_out,
                     uint8_t image_id[CIR_DIGEST_BYTES], uint64_t stats[CIR_STORE_STATS_FIELDS]);

/* The copy of cir_reload_blocks on its own: runs of bytes copied between buffers of any
 * alignment.  The reference has no counterpart.  The rule is ciruela_amd/csrc/copyblk.hpp.
 *
 * Table: nruns records of CIR_COPY_RUN_WORDS u64 {unit_first, src, dst, bytes}: `bytes` (> 0)
 * bytes at the address src go to the address dst, both of any alignment.  A record has
 * ceil(bytes / 16) units of 16 bytes; unit_first is the unit count of all earlier records and
 * nunits that of the whole table.  Unit k of a record is the bytes [16 k, 16 k + n), n = min(16,
 * bytes - 16 k), on both sides: it reads only its own n source bytes and stores only its own n
 * destination bytes.  For every sound record the bytes at src stand at dst afterwards, and no
 * other byte is written.  Sources and destinations of one table must not overlap, and neither
 * may the destinations of different records.
 *
 * res[0] = the bad records: bytes 0, or a unit_first that is not the previous record's plus its
 * units (0 for the first record; the last record must end at nunits).  A bad record is written
 * nowhere and read nowhere; the count is exact whatever the table holds.
 *
 * cir_copy_runs is the host form (src, dst: host addresses; pure, host-only).  CIR_EINVAL: a null
 * runs with a non-zero count, a null res, nruns above 2^32 - 1 or nunits above 2^60. */
#define CIR_COPY_RUN_WORDS 4
#define CIR_COPY_RES_FIELDS 1
int cir_copy_runs(const uint64_t* runs, uint64_t nruns, uint64_t nunits,
                  uint64_t res[CIR_COPY_RES_FIELDS]);

/* The same on the device: table, sources and destinations in device memory (d_runs and d_res
 * 8-byte aligned).  One lane per unit, striding when the table has more units than one grid
 * holds: one 16-byte load and one 16-byte store where the unit is whole and both addresses are
 * 16-byte aligned, otherwise the widest loads the source's and the widest stores the
 * destination's alignment allow, down to single bytes; no atomic touches a destination.  Every
 * word of d_res[CIR_COPY_RES_FIELDS] is written (a memset and one launch; no launch for an empty
 * table).  Like every *_dev call it allocates nothing, synchronises nothing and runs on `stream`
 * alone; ctx may be NULL and is not used.  CIR_EINVAL, decided before any HIP call: as
 * cir_copy_runs, or a misaligned pointer. */
int cir_copy_runs_dev(cir_ctx* ctx, const uint64_t* d_runs, uint64_t nruns, uint64_t nunits,
                      uint64_t* d_res, void* stream);

/* cir_load_blocks for a process that holds the previous version of the image in device memory:
 * the blocks the resident buffers already hold are copied inside device memory, and only the
 * rest is read from the image directory.  The reference has no counterpart (it holds no image in
 * device memory); the observation is the one behind cir_block_sources: most blocks of version
 * N + 1 are already present in version N.
 *
 * The root, index, d_data / ndata, threads, the block numbering, the file ordinals, the outputs
 * and the stream contract are cir_load_blocks'.  d_have[i] / have_bytes[i] (nhave of them) is a
 * flat list of resident buffers on the same device: the tensors of the previous version, in any
 * order and of any alignment.  No path, no index and no claim about their content comes with
 * them: each is cut into blocks of the new index's block size from its own offset 0, and those
 * blocks are hashed where they lie, in this call, with the index's hash type.  An entry that is
 * NULL or empty is ignored.
 *
 * Bit g is 1 exactly when d_data[file] + j * block_size now holds bytes whose digest is the
 * index's: they were copied from a resident block with that digest and length (min(block_size,
 * size - j * block_size) on either side), or read from the root and verified as in
 * cir_load_blocks.  Bytes of blocks with neither are untouched.  Blocks taken from memory are
 * not read, and a file none of whose blocks is left to read is not looked at: a non-empty file
 * all of whose blocks came from memory is never opened, and its state is CIR_FILE_COMPLETE |
 * CIR_FILE_RESIDENT whatever is on disk.  Every other file's state is cir_load_blocks', judged
 * over the combined bitmap; of an ABSENT or BLOCKED file the bits that memory gave stay.  Size-0
 * entries and CIR_FILE_SKIPPED are as in cir_load_blocks.
 *
 * Steps, on the device of `stream`: the memory half is queued on `stream` itself, behind
 * whatever the caller queued there, and waited for: descriptors of the resident blocks
 * (cir_index_memory_dev's kernel), their digests, the new index's digests uploaded (the host
 * parser's: the load pipeline needs the parsed index anyway), cir_match_digests_dev's join with
 * a seed drawn per call, a plan kernel that turns the matches into a copy table in block order
 * and a bitmap, cir_copy_runs_dev's kernel.  Then cir_load_blocks' pipeline runs over the blocks
 * the bitmap lacks.  Device scratch is allocated for the call and freed after it: 44 bytes per
 * resident block plus the join's table (4 bytes per slot, cir_match_table_slots), 48 bytes per
 * resident buffer (its record in two tables), 68.4 bytes per block of the new index, and 40 bytes
 * per file entry of the new index (a run record and a destination).
 *
 * Updating an image in the buffers that hold it is cir_update_blocks' (below), not this call's:
 * a block being overwritten may be another block's source.  CIR_EINVAL, decided before any I/O and any device work: whatever
 * cir_load_blocks rejects; a null d_have or have_bytes with nhave > 0; more than 2^31 - 1
 * resident blocks; any destination range [d_data[i], d_data[i] + size_i) that overlaps any
 * resident range.
 *
 * CIR_RELOAD=disk (read per call) ignores the resident list: the call is then cir_load_blocks
 * (A/B measurement).  CIR_TRACE=1 prints one `cir reload_blocks:` line with the tables, resident
 * hash, digest upload, join, plan + copy, pipeline and whole-call laps and the blocks taken from
 * memory, besides cir_load_blocks' own lines.
 *
 * stats: [0..11] as cir_load_blocks (blocks from memory count as have and are not in [9]; a
 * RESIDENT file is in [2]), [12] blocks copied from memory, [13] bytes copied, [14] resident
 * blocks hashed, [15] files RESIDENT, [16] matches dropped because the lengths differ. */
#define CIR_FILE_RESIDENT 0x40 /* or'ed in: cir_reload_blocks took every block from memory */
#define CIR_RELOAD_STATS_FIELDS 17
int cir_reload_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                      uint32_t threads, void* const* d_data, size_t ndata,
                      const void* const* d_have, const uint64_t* have_bytes, size_t nhave,
                      void* stream, uint64_t** have_out, uint64_t* nblk_out, uint8_t** state_out,
                      int32_t** errno_out, size_t* nfiles_out,
                      uint64_t stats[CIR_RELOAD_STATS_FIELDS]);

/* cir_reload_blocks without the overlap restriction: the next version of an image loaded in the
 * buffers that hold the previous one.  The destinations d_data[i] may be the resident buffers
 * themselves or overlap them in any way -- identical, shifted by whole blocks or by odd bytes,
 * partly inside and partly outside -- or be fresh memory.  The reference has no counterpart.  The
 * rule is ciruela_amd/csrc/update.hpp.
 *
 * Everything not said here is cir_reload_blocks': the root, index, d_data / ndata, the resident
 * list, the outputs, the stream contract and the guarantee: bit g is 1 exactly when d_data[file]
 * + j * block_size now holds bytes whose digest is the index's.  cir_index_memory_dev of a
 * complete result is the new index.
 *
 * Every block g of the index whose file has a destination gets one class (dst = d_data[file] + j
 * * block_size, len = min(block_size, size - j * block_size)).  KEPT: dst lies in a resident
 * buffer at a multiple of block_size from its start, and that resident block has length len and
 * g's digest; nothing is read or written.  This test comes first: a file full of equal blocks is
 * kept, not moved onto itself.  Otherwise a block with a resident block of its digest and length
 * is taken as in cir_reload_blocks: DIRECT when [dst, dst + len) overlaps no resident buffer,
 * copied in phase 1; STAGED otherwise, copied to a scratch in phase 1 and from it to dst in phase
 * 2.  Phase 1 is the last read of the resident buffers; phase 2 and the reads from the root write
 * afterwards, in stream order, so swaps, cycles and shifts need no ordering of single copies.
 *
 * scratch_bytes caps the staging scratch: UINT64_MAX means whatever the staged blocks need, 0
 * stages nothing.  STAGED candidates take ceil(len / 16) units of 16 bytes each, in block order;
 * one is staged while the units of all candidates up to and including it fit in scratch_bytes /
 * 16, and DEMOTED otherwise: not taken, bit 0 unless the root gives the block, read from the root
 * like any missing block.  The cut is a prefix in block order, whatever the timing.
 *
 * Until the scratch is allocated -- min(scratch_bytes, 16 bytes per staged unit), after the plan
 * -- no byte of any caller buffer has been written: CIR_ENOMEM from that allocation or any error
 * before it leaves version N as it was.  After that the old version is gone as an image, and on a
 * later error the bitmap, where one is returned, is the only truth about the buffers.  Bytes of
 * blocks that were neither taken nor read are untouched, as in cir_reload_blocks.
 *
 * A non-empty file all of whose blocks are KEPT, DIRECT or STAGED is never opened: its state is
 * CIR_FILE_COMPLETE | CIR_FILE_RESIDENT.
 *
 * Steps, on `stream`: cir_reload_blocks' descriptors, resident hash, digest upload and join; two
 * plan kernels (classes and counts, their prefixes and the cut); one synchronise for the counts;
 * the scratch; a third plan kernel (the bitmap and the two copy tables, in block order) and
 * cir_copy_runs_dev's kernel twice.  Then cir_load_blocks' pipeline over the blocks the bitmap
 * lacks.  Device scratch besides the staging scratch: cir_reload_blocks' plus 32.5 bytes per block
 * of the new index (a second table, two more words per tile).
 *
 * CIR_EINVAL, decided before any I/O and any device work: whatever cir_reload_blocks rejects
 * except a destination that overlaps a resident buffer; two resident buffers that overlap one
 * another (the call writes into them); two destinations of non-empty entries that overlap one
 * another.
 *
 * CIR_UPDATE=disk (read per call) ignores the resident list: the call is then cir_load_blocks
 * into the same buffers (A/B measurement).  CIR_TRACE=1 prints one `cir update_blocks:` line with
 * cir_reload_blocks' laps and the kept, copied, staged and demoted blocks.
 *
 * stats: [0..16] as cir_reload_blocks, [12] and [13] the DIRECT and staged blocks and their
 * bytes; [17] blocks kept, [18] bytes kept, [19] blocks staged, [20] bytes of staging scratch
 * allocated, [21] blocks demoted by the cap. */
#define CIR_UPDATE_STATS_FIELDS 22
int cir_update_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                      uint32_t threads, void* const* d_data, size_t ndata,
                      const void* const* d_have, const uint64_t* have_bytes, size_t nhave,
                      uint64_t scratch_bytes, void* stream, uint64_t** have_out,
                      uint64_t* nblk_out, uint8_t** state_out, int32_t** errno_out,
                      size_t* nfiles_out, uint64_t stats[CIR_UPDATE_STATS_FIELDS]);

/* Slots the table of cir_match_digests_dev needs for n_pool digests: the smallest power of two
 * >= max(64, 2 * n_pool), so the table is never more than half full (0 when no u64 holds it:
 * n_pool > 2^62).  Pure: no HIP call. */
uint64_t cir_match_table_slots(uint64_t n_pool);

/* The join behind cir_block_sources, device-resident: which of n_need digests (d_need, 32 bytes
 * each) occur among n_pool digests (d_pool), and where first.  The reference has no counterpart:
 * fill_blocks queues every block of every file that was not hardlinked whole (src/daemon/
 * tracking/progress.rs:129-170), and scan_links matches whole files only (src/daemon/metadata/
 * hardlink_sources.rs:131-133, the break at :143).
 *
 * d_match[i] (device u32 x n_need) = the smallest j < n_pool with pool[j] == need[i] over all 32
 * bytes, or UINT32_MAX; *d_nmatch (device u32, may be NULL) = the number of entries that
 * matched.  d_table is table_slots u32 of device scratch that the call initialises itself
 * (table_slots a power of two >= cir_match_table_slots(n_pool)).  Like every *_dev call it
 * allocates nothing, synchronises nothing and runs on `stream` alone; there are no side
 * streams, so ctx may be NULL and is not used for scratch.  Every d_match[0 .. n_need) and the
 * count are written by the call, nothing past them and nothing past d_table[table_slots);
 * n_pool == 0 writes all UINT32_MAX and 0, n_need == 0 writes only the count.
 *
 * The table is open addressing with linear probing (wrapping) over pool ordinals, and the home
 * slot is part of the contract: x = seed; for the digest's four little-endian u64 words w in
 * order, x = (x ^ w) * 0x9E3779B97F4A7C15, x ^= x >> 32; home = x & (table_slots - 1).  It
 * folds all 32 bytes under the caller's seed because pool digests come from other parties'
 * indexes: digests crafted to share a prefix do not share a home slot, and a caller that joins
 * untrusted digests passes an unpredictable seed (cir_block_sources draws one per call), so
 * nobody can craft a pool that chains through one run of slots.  The result does not depend
 * on the seed.
 *
 * CIR_EINVAL: a NULL or non-16-byte-aligned d_need or d_pool when its count is not 0; a NULL
 * d_match with n_need > 0; a NULL d_table; table_slots not a power of two or below
 * cir_match_table_slots(n_pool); n_pool > 2^31 - 1; n_need > 2^32 - 1 (the count is a u32);
 * d_match, d_table or d_nmatch not 4-byte aligned. */
int cir_match_digests_dev(cir_ctx* ctx, const uint8_t* d_need, size_t n_need,
                          const uint8_t* d_pool, size_t n_pool,
                          uint32_t* d_table, uint64_t table_slots, uint64_t seed,
                          uint32_t* d_match, uint32_t* d_nmatch, void* stream);

/* Which blocks of a new image older local images already hold, and where: what fill_blocks
 * (src/daemon/tracking/progress.rs:129-170) would need in order not to put every block of a
 * changed, appended-to or moved file on the wire.  scan_links matches whole files only -- same
 * path, same size, all digests equal (src/daemon/metadata/hardlink_sources.rs:131-133) -- so
 * one changed block sends its whole file, although the other blocks sit in an older image of
 * the same base directory.  The indexes say where; no file is read, and nothing is copied (the
 * copy stays the caller's, and cir_check_blocks afterwards re-hashes what was copied).
 *
 * The rule.  Need list: the file entries of `index` in index order, blocks ascending -- the
 * global block numbering of cir_check_index's stats[7] and of cir_check_blocks.  Pool: the
 * sources src_index[s] / src_len[s] (s < nsrc) in the order given (the reference ranks newest
 * first, hardlink_sources.rs:66-72), within a source the file entries in index order, blocks
 * ascending; pool ordinal j counts across all sources.  A source that does not parse, or whose
 * hash type or block size is not the new index's, takes no part and is counted in
 * *nskipped_out (may be NULL), as in cir_link_candidates; source ordinals in the result still
 * refer to the order given.  Block g matches the smallest pool ordinal j whose 32-byte digest
 * equals its own: the first source in the caller's ranking, then the first place in index
 * order (the flavour of scan_links' break at :143).  Then the two blocks' lengths, min(bs,
 * size - block * bs) on either side, are compared: if they differ the source index lies or a
 * digest collided, the block is reported as not found and counted in stats[5], and no second
 * candidate is looked for.  Matches inside `index` itself are cir_block_repeats' (below).
 *
 * want (may be NULL = every block): a bitmap over the global blocks, bit (g & 63) of word
 * g >> 6, ceil(nblk / 64) words; bits at and past nblk are ignored.  The caller clears the
 * blocks of hardlinked files and the 1-bits of a cir_check_blocks bitmap.
 *
 * For every global block g: src_out[g] = the source ordinal, or UINT32_MAX for "not found" and
 * for "not wanted"; src_file_out[g] = the file ordinal inside that source's index, counting
 * file entries only as in cir_link_candidates; src_block_out[g] = the block number inside that
 * file (byte offset block x block_size; the length is the new block's own).  Unmatched entries
 * of the last two are UINT64_MAX.  The arrays are malloc'd (cir_free), *nblk_out long, and
 * NULL when *nblk_out == 0.
 *
 * With ctx == NULL the rule is applied on the host with a hash map in which the first entry
 * wins, and no GPU is needed.
 *
 * With a context the join runs on the context's first device (cir_match_digests_dev's kernels;
 * device buffers are allocated for the call and freed after it, the seed is drawn per call, the
 * current device is restored).  So does the parse of the texts: every text is framed on the
 * host (cir_index_frame's rules), uploaded, and its body decoded by cir_index_digests_dev's
 * kernels straight into the join's buffers; only the run tables (32 bytes per non-empty file)
 * come back.  A text the device declines takes the host parser, that text alone, and a call
 * that ends before any join (a new index without blocks, a list past its limit) is decided by
 * the host parser altogether.  Which sources are skipped, the stats, and the error code and
 * text of a new index that does not parse are therefore the host parser's.  The device's lock
 * is not held while a text is parsed on the host.  CIR_SOURCES_PARSE=host keeps every text on
 * the host.  From 16,384 needed blocks on, the matches are mapped back to (source, file, block)
 * on the device as well (cir_match_extents_dev's k_map_matches behind the join, on the same
 * stream; the combined run tables go up, the three arrays come down); smaller calls, and every
 * call under CIR_SOURCES_MAP=host, keep that loop on a host thread.
 *
 * Both give identical arrays, skip counts and stats ([6] and [7] aside).
 *
 * CIR_EINVAL: null arguments, or more than 2^31 - 1 pool blocks in total (pass fewer sources);
 * CIR_EPARSE / CIR_EHASHSIZE: `index` does not parse; CIR_ENOMEM.  All are decided before any
 * join.
 *
 * stats: [0] blocks wanted, [1] blocks found, [2] bytes found locally, [3] pool blocks, [4]
 * sources used, [5] matches dropped because the lengths differ, [6] table slots (0 on the
 * host), [7] 1 if joined on the device (a context was given), 0 if on the host. */
#define CIR_SOURCES_STATS_FIELDS 8
int cir_block_sources(cir_ctx* ctx, const uint8_t* index, size_t len,
                      const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                      const uint64_t* want,
                      uint32_t** src_out, uint64_t** src_file_out, uint64_t** src_block_out,
                      uint64_t* nblk_out, size_t* nskipped_out,
                      uint64_t stats[CIR_SOURCES_STATS_FIELDS]);

/* ---- local copies as extents ------------------------------------------ */

/* Bytes of device scratch cir_match_extents_dev needs for n_need blocks (two bitmaps and one
 * u64 per tile).  Pure. */
uint64_t cir_extents_work_bytes(uint64_t n_need);

/* Need blocks per workgroup of cir_match_extents_dev's map and emit passes (2048: tests place
 * extent heads and tails across this boundary).  Pure. */
uint64_t cir_debug_extent_tile_blocks(void);

/* The matches of cir_match_digests_dev mapped back to files and merged into extents, device-
 * resident: what a caller copies with one copy_file_range per extent instead of walking 20 bytes
 * per block.  The reference has no counterpart (fill_blocks queues every block, src/daemon/
 * tracking/progress.rs:129-170).  The rule is ciruela_amd/csrc/extents.hpp, one text for the
 * kernels, the host path and its fuzz.
 *
 * Inputs: d_match[g] for g < n_need as cir_match_digests_dev leaves it; a need run table and a
 * pool run table of four u64 per non-empty file {first, size, file, x}, `first` ascending.  In
 * the need table x is ignored, so the table cir_index_digests_dev writes fits as it is.  In the
 * pool table `first` is a pool ordinal across all sources and x (its low 32 bits) the source
 * ordinal.  n_pool, block_size, and d_want (may be NULL = every block; the bitmap layout of
 * cir_block_sources' want, ceil(n_need / 64) words).
 *
 * Per block g: its need run is the last one with first <= g; if there is none, or g - first >=
 * ceil(size / block_size), the block lies in no file and is neither wanted nor found.  Otherwise
 * it is wanted iff its want bit is set.  A wanted block with d_match[g] = j < n_pool whose pool
 * run covers j is found iff the two blocks' lengths min(bs, size - block x bs) are equal; unequal
 * lengths count as dropped and no second candidate is looked for (cir_block_sources' rule).
 * Block g continues block g - 1 iff both are found, lie in the same need run, have the same src
 * and src_file, and src_block(g) == src_block(g - 1) + 1.  An extent is a maximal stretch of
 * blocks so joined: a need-file boundary breaks it, and so does a source-file or source boundary
 * (even where the pool ordinals are consecutive), an unwanted or dropped block, and two need
 * blocks that match the same pool block.
 *
 * Outputs.  d_src / d_file / d_block (device, n_need entries each; all three or all NULL): as
 * cir_block_sources' arrays.  d_fetch (device u64 x ceil(n_need / 64), may be NULL): bit (g & 63)
 * of word g >> 6 = 1 iff block g is wanted and not found; every word is written, bits at and
 * past n_need as 0 -- the layout of cir_check_blocks' bitmap and of `want`.  d_extents (device,
 * eight u64 per record, cap_extents records): {first, count, need_file, need_block, src,
 * src_file, src_block, bytes} in ascending `first`; first = the global number of the extent's
 * first block, need_block and src_block = block numbers inside their files, bytes = min(size,
 * (need_block + count) x bs) - need_block x bs.  d_res (device u64 x CIR_EXTENTS_RES_FIELDS):
 * [0] CIR_EXTENTS_OK or CIR_EXTENTS_CAPACITY, [1] wanted, [2] found, [3] bytes found, [4]
 * dropped, [5] extents; every word is written by the call.  On CIR_EXTENTS_CAPACITY ([5] >
 * cap_extents) the counts, the per-block arrays and the bitmap are exact and written, and no
 * extent record is.  d_work: work_bytes >= cir_extents_work_bytes(n_need) of device scratch.
 *
 * Like every *_dev call it allocates nothing, synchronises nothing and runs on `stream` alone
 * (four launches: map, scan, emit, finish; no workgroup waits for another; every loop is bounded
 * by an argument); ctx may be NULL and is not used.  Whatever the run tables and d_match hold
 * (unsorted, overlapping, `first` past n_need, sizes of 2^64 - 1, ordinals >= n_pool), nothing
 * is read or written outside the arrays as sized by the arguments, and no record at or past
 * cap_extents is written: such input gives an unspecified answer, not a fault.
 *
 * CIR_EINVAL: a NULL d_match (with n_need > 0), run table (with its count > 0), d_extents (with
 * cap_extents > 0), d_work or d_res; per-block arrays given in part; d_match or d_src not 4-byte
 * aligned, any other pointer not 8-byte aligned; block_size == 0; n_need > 2^32 - 1; n_pool >
 * 2^31 - 1; cap_extents > 2^57; work_bytes < cir_extents_work_bytes(n_need). */
#define CIR_EXTENT_WORDS 8
#define CIR_EXTENTS_RES_FIELDS 6
#define CIR_EXTENTS_OK 0
#define CIR_EXTENTS_CAPACITY 1
int cir_match_extents_dev(cir_ctx* ctx, const uint32_t* d_match, uint64_t n_need,
                          const uint64_t* d_need_runs, uint64_t n_need_runs,
                          const uint64_t* d_pool_runs, uint64_t n_pool_runs, uint64_t n_pool,
                          uint64_t block_size, const uint64_t* d_want,
                          uint32_t* d_src, uint64_t* d_file, uint64_t* d_block, uint64_t* d_fetch,
                          uint64_t* d_extents, uint64_t cap_extents,
                          void* d_work, uint64_t work_bytes, uint64_t* d_res, void* stream);

/* cir_block_sources' question answered as extents: the inputs, the skip rules and the errors are
 * cir_block_sources'.  *extents_out = malloc'd records of CIR_EXTENT_WORDS u64 as above
 * (cir_free; NULL when *nextents_out == 0); *fetch_out = the malloc'd bitmap of the wanted blocks
 * without a local copy, ceil(*nblk_out / 64) words (cir_free; NULL when *nblk_out == 0): what is
 * left to fetch, and the `want` of a later call.
 *
 * With a context the device flow of cir_block_sources runs up to the join; then the combined run
 * tables go up (32 bytes per non-empty file) and cir_match_extents_dev's kernels run behind the
 * join on the same stream.  One synchronise learns the extent count, the records are allocated
 * exactly, emitted and downloaded with the bitmap; the per-block arrays never leave the device
 * (they are not even made).  With ctx == NULL the host applies the same rule (map_matches and
 * extents_of in ciruela_amd/csrc/sources.hpp), and no GPU is needed.  Both give identical
 * output.  CIR_SOURCES_MAP=host, read per call, keeps the mapping on a host thread behind the
 * device join.
 *
 * stats: cir_block_sources' eight fields, [8] extents, [9] blocks left to fetch. */
#define CIR_EXTENTS_STATS_FIELDS 10
int cir_block_extents(cir_ctx* ctx, const uint8_t* index, size_t len,
                      const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                      const uint64_t* want,
                      uint64_t** extents_out, size_t* nextents_out, uint64_t** fetch_out,
                      uint64_t* nblk_out, size_t* nskipped_out,
                      uint64_t stats[CIR_EXTENTS_STATS_FIELDS]);

/* ---- blocks repeated inside one image --------------------------------- */

/* The join behind cir_block_repeats, device-resident: which of the n blocks of one index
 * (d_digests, 32 bytes each, in the global block numbering of cir_check_blocks -- what
 * cir_index_digests_dev writes) carry a digest that another participating block of the same
 * index carries, and which block stands for it.  The reference has no counterpart: fill_blocks
 * queues one Block per (path, offset) (src/daemon/tracking/progress.rs:129-170), so a digest
 * that occurs twice inside the image is fetched twice.  The rule is ciruela_amd/csrc/
 * repeats.hpp, one text for the kernels, the host path and its fuzz.
 *
 * d_want / d_present (device u64 x ceil(n / 64), each may be NULL): bitmaps, bit (g & 63) of word
 * g >> 6, bits at and past n ignored.  Block g is wanted when d_want is NULL or its bit is set;
 * present when it is not wanted, d_present is not NULL and its bit is set (a bit in both means
 * wanted); a block that is neither takes no part, neither as a source nor as a destination.  A
 * present block's key is g, a wanted block's 2^31 + g, and the leader of a digest is the block
 * with the smallest key among the participating blocks with that digest over all 32 bytes: a
 * present holder beats any wanted one, and among equals the first in index order wins.
 *
 * d_match[g] (device u32 x n) = UINT32_MAX when g is not wanted or is its own leader; otherwise
 * the leader L as an ordinal of a pool of 2n: L when the leader is present, n + L when it is a
 * wanted block (which will be fetched).  *d_nmatch (device u32, may be NULL) = the number of
 * entries that are not UINT32_MAX.  So d_match feeds cir_match_extents_dev as it is, with the
 * need run table twice as the pool's -- the first copy with x = 0, the second with every `first`
 * raised by n and x = 1, n_pool = 2n: an extent's src is then 0 for a present source and 1 for a
 * fetched one, and src_file a file ordinal of the same index.
 *
 * d_table is table_slots u32 of device scratch that the call initialises itself (table_slots a
 * power of two >= cir_match_table_slots(n): the table holds at most n entries); the home slot
 * and the seed are cir_match_digests_dev's, and the result does not depend on the seed.  Like
 * every *_dev call it allocates nothing, synchronises nothing and runs on `stream` alone (one
 * memset and two launches, build and probe; no lane waits for another's write and every loop is
 * bounded by table_slots); ctx may be NULL and is not used.  Every d_match[0 .. n) and the count
 * are written by the call, nothing past them and nothing past d_table[table_slots); n == 0
 * writes only the count.
 *
 * CIR_EINVAL, decided before any HIP call: a NULL d_digests or d_match with n > 0; a NULL
 * d_table; d_digests not 16-byte aligned; a bitmap not 8-byte aligned; d_match, d_table or
 * d_nmatch not 4-byte aligned; table_slots not a power of two or below
 * cir_match_table_slots(n); n > CIR_REPEATS_MAX_BLOCKS (2n must stay within
 * cir_match_extents_dev's 2^31 - 1, and 2^31 + g clear of UINT32_MAX). */
#define CIR_REPEATS_MAX_BLOCKS 0x3FFFFFFF /* 2^30 - 1 */
int cir_match_repeats_dev(cir_ctx* ctx, const uint8_t* d_digests, size_t n,
                          const uint64_t* d_want, const uint64_t* d_present,
                          uint32_t* d_table, uint64_t table_slots, uint64_t seed,
                          uint32_t* d_match, uint32_t* d_nmatch, void* stream);

/* Which blocks of a new image need not be fetched because the same image holds, or will fetch,
 * a block with the same digest: a vendored copy of a directory, one shared object under two
 * paths, a zero-filled file, a file kept under an old and a new name.  The last digest join of
 * the download path: cir_check_links covers whole files, cir_check_blocks what a partial
 * directory holds, cir_block_extents the copies in older images; what they leave in the fetch
 * bitmap is still queued by position.  No file is read and nothing is copied.
 *
 * want / present (each may be NULL): the bitmaps of cir_match_repeats_dev over the global blocks
 * of `index`, ceil(nblk / 64) words.  want: the blocks still to be obtained, for example
 * cir_block_extents' fetch_out.  present: blocks that are in the new directory, or will be
 * before any copy below is made -- hardlinked files, cir_check_blocks' 1-bits, blocks covered by
 * cir_block_extents' extents.
 *
 * A wanted block whose digest's leader (above) is another block L is a repeat: it is obtained by
 * copying block L of the same image.  The two blocks' lengths min(bs, size - block x bs) are
 * compared first: if they differ the index lies or a digest collided, the block is counted in
 * stats[5], stays in the fetch bitmap, and no second candidate is looked for (cir_block_sources'
 * rule).  Repeats are merged into extents exactly as cir_match_extents_dev merges copies: a
 * stretch continues while the blocks are consecutive repeats inside one file whose leaders are
 * consecutive blocks of one file and of one class, all present or all fetched; two repeats of
 * the same leader break it, so a zero-filled file of k blocks gives one fetched block and k - 1
 * one-block extents.  A leader is never a repeat, so no block is both a source and a
 * destination: extents of one class can be applied in any order, and a copy inside one file
 * never overlaps.  With nothing dropped, the blocks left to fetch have pairwise distinct
 * digests, none of them a present block's.
 *
 * *extents_out = malloc'd records of CIR_EXTENT_WORDS u64 as cir_block_extents', ascending
 * `first` (cir_free; NULL when *nextents_out == 0): src = 0 when the source block is present
 * (copy at once, after the local copies), 1 when it is fetched (copy after the fetch); src_file
 * = a file ordinal of `index`.  *fetch_out = the malloc'd bitmap of the wanted blocks that are
 * not repeats, ceil(*nblk_out / 64) words (cir_free; NULL when *nblk_out == 0): a valid `want`
 * for any sibling call.
 *
 * With ctx == NULL the host parser and a hash map in which the smaller key wins apply the rule,
 * then map_matches and extents_of of ciruela_amd/csrc/sources.hpp; no GPU is needed.  With a
 * context the call runs on the context's first device under that device's lock (buffers are
 * allocated for the call and freed after it, the seed is drawn per call, the current device is
 * restored): the text is framed on the host and uploaded once, cir_index_digests_dev's kernels
 * leave the digests and the run table in device memory, the run table comes back (32 bytes per
 * non-empty file) and goes up doubled with the bitmaps, cir_match_repeats_dev's and
 * cir_match_extents_dev's kernels run on one stream, one synchronise learns the extent count,
 * and the records and the bitmap come down; the per-block arrays are not made.  A text the
 * device declines, and every text under CIR_SOURCES_PARSE=host, takes the host parser and its
 * digests are uploaded instead.  Both paths give identical output, stats [6] and [7] aside.
 *
 * CIR_EINVAL: null index, outputs or stats, or more than CIR_REPEATS_MAX_BLOCKS blocks;
 * CIR_EPARSE / CIR_EHASHSIZE: `index` does not parse; CIR_ENOMEM.  All are decided before any
 * join; on error the outputs are NULL / 0 and the stats zero.
 *
 * stats: [0] blocks wanted, [1] repeats found, [2] their bytes, [3] blocks that took part, [4] of
 * those present, [5] dropped because the lengths differ, [6] table slots (0 on the host), [7] 1
 * if joined on the device, [8] extents, [9] blocks left to fetch = [0] - [1]. */
#define CIR_REPEATS_STATS_FIELDS 10
int cir_block_repeats(cir_ctx* ctx, const uint8_t* index, size_t len,
                      const uint64_t* want, const uint64_t* present,
                      uint64_t** extents_out, size_t* nextents_out, uint64_t** fetch_out,
                      uint64_t* nblk_out, uint64_t stats[CIR_REPEATS_STATS_FIELDS]);

/* ---- an index's digests as an array ----------------------------------- */

/* The frame of a DIRSIGNATURE.v1 index without its body.  Pure host code, no HIP call: the
 * index parser's rules for the line structure (the text ends in '\n' and has at least two
 * lines), the header line ("DIRSIGNATURE.v1", the hash type, an optional block_size=N, default
 * 32768) and the footer line (non-empty hex), with that parser's error texts.  *hash_type =
 * CIR_HASH_*, *block_size, and the body as the bytes [*body_off, *body_end) of `index`: behind
 * the header line, before the footer line; empty, or ending in '\n'.  CIR_EINVAL: a null
 * pointer; CIR_EPARSE as the parser would. */
int cir_index_frame(const uint8_t* index, size_t len, int* hash_type, uint64_t* block_size,
                    uint64_t* body_off, uint64_t* body_end);

/* Bytes of device scratch cir_index_digests_dev needs for a text of len bytes.  Pure. */
uint64_t cir_index_work_bytes(uint64_t len);

/* Bytes of text per workgroup of cir_index_digests_dev's count and emit passes (4096: tests
 * place line starts, heads and tokens across this boundary). */
uint64_t cir_debug_index_tile_bytes(void);

/* The block digests of an index, parsed on the device: index text in (d_text, len bytes, the
 * body at [body_off, body_end) as cir_index_frame gives it), the digests of its file entries out
 * as one flat list -- d_digests, 32 bytes per block, in index order, blocks ascending: the global
 * block numbering of cir_check_blocks and the need list of cir_block_sources, ready for
 * cir_match_digests_dev -- and one run record of four u64 per non-empty file in d_runs:
 * {first, size, file, hash_off} = the global block number of its block 0, the entry's size, its
 * file ordinal (file entries only, as in cir_link_candidates) and the offset in the text of its
 * first hash token's leading space.  The reference has no counterpart: every consumer there
 * parses the text on a host thread.
 *
 * The device takes a canonical subset of what the host parser accepts (ciruela_amd/csrc/
 * idxscan.hpp states it: one space between tokens, no raw byte outside 0x21..0x7e, \xNN escapes
 * that form no ".", ".." or "/", directory lines and entry heads of at most 4096 bytes, exactly
 * ceil(size / block_size) tokens of one space and 64 hex digits) and declines everything else;
 * it never guesses.  Status CIR_INDEX_OK means the host parser accepts the same bytes and gives
 * the same file count, runs and digests.  A declined text goes to the host parser (cir_index_digests
 * does that), which alone decides between success, CIR_EPARSE and CIR_EHASHSIZE.
 *
 * d_res (device, CIR_INDEX_RES_FIELDS u64): [0] CIR_INDEX_OK, CIR_INDEX_CAPACITY or
 * CIR_INDEX_DECLINED, [1] file entries, [2] runs, [3] blocks, [4] the offset of the first
 * declined line's start, or UINT64_MAX.  On CIR_INDEX_OK d_digests[0 .. 32 x [3]) and d_runs[0 ..
 * 4 x [2]) are written.  On CIR_INDEX_CAPACITY ([3] > cap_blocks or [2] > cap_runs) the counts are
 * exact and neither array is written; on CIR_INDEX_DECLINED the counts and the arrays mean
 * nothing.  cap_blocks = len / 65 and cap_runs = len / 73 always suffice for a text the host
 * parser accepts (a token is 65 bytes, the shortest line with a token 73), so a caller can
 * allocate without a round trip; with those caps CIR_INDEX_CAPACITY is a text the host parser
 * rejects.  Nothing is written past cap_blocks digests, cap_runs records, d_work[work_bytes) or
 * d_res[5), and every d_res word is written by the call.
 *
 * Like every *_dev call it allocates nothing, synchronises nothing and runs on `stream` alone
 * (four launches: count, scan, emit, decode; no workgroup waits for another, and no atomic is
 * issued unless a line is declined); ctx may be NULL and is not used.
 *
 * CIR_EINVAL: a null d_text (with len > 0), d_digests (with cap_blocks > 0), d_runs (with cap_runs
 * > 0), d_work or d_res; d_digests not 16-byte aligned; d_text, d_runs, d_work or d_res not
 * 8-byte aligned; body_off > body_end; body_end > len; block_size == 0; work_bytes <
 * cir_index_work_bytes(len); cap_blocks > 2^32 - 1; len > 2^36. */
#define CIR_INDEX_RES_FIELDS 5
#define CIR_INDEX_OK 0
#define CIR_INDEX_CAPACITY 1
#define CIR_INDEX_DECLINED 2
int cir_index_digests_dev(cir_ctx* ctx, const uint8_t* d_text, uint64_t len, uint64_t body_off,
                          uint64_t body_end, uint64_t block_size, uint8_t* d_digests,
                          uint64_t cap_blocks, uint64_t* d_runs, uint64_t cap_runs, void* d_work,
                          uint64_t work_bytes, uint64_t* d_res, void* stream);

/* The host form: `index` in host memory to malloc'd arrays (cir_free; NULL when empty):
 * *digests_out = 32 x *nblk_out bytes, *runs_out = 4 x *nruns_out u64 as above, *nfiles_out =
 * the file entries; *hash_type = CIR_HASH_* and *block_size from the header.  With a context:
 * cir_index_frame, one upload, cir_index_digests_dev's kernels on the context's first device,
 * one download; a text the device declines (or whose frame does not parse) takes the host parser
 * instead; the current device is restored.  With ctx == NULL: the host parser alone, and no GPU
 * is needed.  Both give identical arrays and identical error codes (CIR_EPARSE, CIR_EHASHSIZE:
 * the index does not parse; CIR_EINVAL: a null pointer; CIR_ENOMEM).
 *
 * stats: [0] 1 if the device parsed it, [1] 1 if the device declined and the host parsed, [2] the
 * declined line's offset (UINT64_MAX when none was reported), [3] text bytes uploaded. */
#define CIR_INDEX_STATS_FIELDS 4
int cir_index_digests(cir_ctx* ctx, const uint8_t* index, size_t len, int* hash_type,
                      uint64_t* block_size, uint8_t** digests_out, uint64_t* nblk_out,
                      uint64_t** runs_out, size_t* nruns_out, size_t* nfiles_out,
                      uint64_t stats[CIR_INDEX_STATS_FIELDS]);

/* ---- hardlink candidates matched on the device ------------------------ */

/* Bytes of device scratch cir_index_files_dev needs for a text of len bytes.  Pure.  (Its text
 * tile is cir_debug_index_tile_bytes.) */
uint64_t cir_index_files_work_bytes(uint64_t len);

/* The file entries of an index, parsed on the device: the sibling of cir_index_digests_dev over
 * the same text and frame (d_text, len, body_off, body_end, block_size as there).  One record of
 * CIR_FILE_WORDS u64 per file entry, size-0 entries included, at the entry's file ordinal (file
 * entries only, as in cir_link_candidates): {name_off, dir_off, size, first | exe << 63} = the
 * text offset of the name's first byte, the offset of the '/' that starts the entry's directory
 * line, the entry's size, and the global block number of its block 0 (for an empty file the
 * number the next block would get) with the exe flag in bit 63.  off_bias is added to both
 * offsets as written and block_bias to `first`, so that the records of several texts that sit in
 * one device arena address that arena and one digest list.  The reference has no counterpart.
 *
 * The lines the device takes are cir_index_digests_dev's (ciruela_amd/csrc/idxscan.hpp, the same
 * parse of every line's head), and the statuses are its CIR_INDEX_*.  d_res (device,
 * CIR_FILES_RES_FIELDS u64): [0] the status, [1] file entries, [2] blocks, [3] the offset of the
 * first declined line's start, or UINT64_MAX.  On CIR_INDEX_OK d_files[0 .. 4 x [1]) is written;
 * on CIR_INDEX_CAPACITY ([1] > cap_files) the counts are exact and no record is written; on
 * CIR_INDEX_DECLINED the counts mean nothing.  cap_files = len / 8 always suffices (the shortest
 * file line is "  a f 0\n").  A last pass reads every hash token's digits, so the two calls never
 * disagree about a text: a bad hex digit declines its line here as it does there.  Nothing is
 * written past cap_files records, d_work[work_bytes) or d_res[4), and every d_res word is written
 * by the call.
 *
 * Like every *_dev call it allocates nothing, synchronises nothing and runs on `stream` alone
 * (one memset of d_res and four launches: count, scan, emit, token check; each tile reports the last
 * directory line it owns, the scan carries a running maximum across the tiles, and an entry takes
 * the last directory line at or before it; no workgroup waits for another); ctx may be NULL and
 * is not used.
 *
 * CIR_EINVAL, decided before any HIP call: a null d_text (with len > 0), d_files (with cap_files
 * > 0), d_work or d_res; any of them not 8-byte aligned; body_off > body_end; body_end > len;
 * block_size == 0; work_bytes < cir_index_files_work_bytes(len); len > 2^36; cap_files > 2^58. */
#define CIR_FILE_WORDS 4
#define CIR_FILES_RES_FIELDS 4
int cir_index_files_dev(cir_ctx* ctx, const uint8_t* d_text, uint64_t len, uint64_t body_off,
                        uint64_t body_end, uint64_t block_size, uint64_t off_bias,
                        uint64_t block_bias, uint64_t* d_files, uint64_t cap_files, void* d_work,
                        uint64_t work_bytes, uint64_t* d_res, void* stream);

/* Bytes of device scratch cir_match_files_dev needs: 16 per file of either side and 4 per table
 * slot (cir_match_table_slots(n_pool_files)).  Pure; 0 when a count passes the call's limits. */
uint64_t cir_match_files_work_bytes(uint64_t n_need_files, uint64_t n_pool_files);

/* The join behind cir_file_sources, device-resident: cir_link_candidates' rule over file records.
 * Each side is a text arena (d_*_text, *_text_len bytes), the file records over it (d_*_files,
 * CIR_FILE_WORDS u64 each, what cir_index_files_dev wrote with its biases) and the flat digests
 * the records' `first` count into (d_*_digests, 32 bytes per block, what cir_index_digests_dev
 * wrote); the two sides may share an arena.  Pool files are ordered by source, then in index
 * order; d_src_first (device u64 x (nsrc + 1)) holds the first pool file ordinal of each source
 * and the pool's file count last.  block_size is the indexes' (a file holds ceil(size /
 * block_size) blocks).
 *
 * For need file i the sources 0 .. nsrc-1 in order: a source matches when the first file entry it
 * lists at the same path has equal exe flag, size and digests, and the first matching source
 * makes the candidate: d_cand_src[i] (device u32; UINT32_MAX: none) and d_cand_file[i] (device
 * u64, the file ordinal inside that source; UINT64_MAX: none).  Two paths are equal when their
 * decoded directories and their decoded names are equal byte by byte (\x41 equals A); they are
 * compared over the arenas, never copied.  d_res (device, CIR_FILES_RES_FIELDS u64): [0]
 * CIR_FILES_OK or CIR_FILES_COLLISION, [1] candidates, [2] the sum of their sizes, [3] need files.
 *
 * All on `stream` behind one memset of d_work: fold (each file's 128-bit fold is the sum mod 2^64,
 * per word, of a term mixed under `seed` from a block's position in its file and its digest;
 * summed inside the wave over the lanes that share a file, one integer atomic add per wave, file
 * and word, so the result does not depend on arrival order), build (one lane per pool file into a
 * table of pool ordinals on cir_match_digests_dev's discipline, keyed by source and decoded path:
 * the slot of (source, path) ends holding the source's first entry), probe (one lane per need
 * file; equal exe flag, size and fold stop the search) and verify (one lane per need block of a
 * file with a candidate: its digest must equal the candidate's at the same position, read from
 * d_pool_verify -- NULL: d_pool_digests; tests pass another array to reach the status).  A
 * difference is CIR_FILES_COLLISION and the arrays mean nothing; with CIR_FILES_OK the answer is
 * exactly the host rule's, whatever the seed.  No lane waits for another and every loop is
 * bounded by an argument; a path walk reads at most 4096 bytes of each token.  Whatever the
 * records hold, nothing outside the arrays as sized by the arguments is read or written: records
 * that do not describe the arrays give an unspecified answer, not a fault.  ctx may be NULL and
 * is not used.
 *
 * CIR_EINVAL, decided before any HIP call: a null array with a non-zero count, a null
 * d_src_first, d_work or d_res; a digest array not 16-byte aligned; records, d_src_first, d_work,
 * d_cand_file or d_res not 8-byte aligned; d_cand_src not 4-byte aligned; block_size == 0; more
 * than 2^31 - 1 pool files, 2^32 - 1 need files or 2^32 - 1 blocks on a side; work_bytes <
 * cir_match_files_work_bytes(n_need_files, n_pool_files). */
#define CIR_FILES_OK 0
#define CIR_FILES_COLLISION 1
int cir_match_files_dev(cir_ctx* ctx, const uint8_t* d_need_text, uint64_t need_text_len,
                        const uint64_t* d_need_files, uint64_t n_need_files,
                        const uint8_t* d_need_digests, uint64_t n_need_blocks,
                        const uint8_t* d_pool_text, uint64_t pool_text_len,
                        const uint64_t* d_pool_files, uint64_t n_pool_files,
                        const uint8_t* d_pool_digests, uint64_t n_pool_blocks,
                        const uint64_t* d_src_first, uint64_t nsrc, uint64_t block_size,
                        const uint8_t* d_pool_verify, uint64_t seed, void* d_work,
                        uint64_t work_bytes, uint32_t* d_cand_src, uint64_t* d_cand_file,
                        uint64_t* d_res, void* stream);

/* cir_link_candidates with a context: the same arguments, outputs, rule and error codes, and
 * stats.  With ctx == NULL the host rule runs as in cir_link_candidates and no GPU is needed.
 * With a context the call runs on the context's first device under that device's lock (buffers
 * are allocated for the call and freed after it, the seed is drawn per call, the current device
 * is restored): every text is framed on the host (cir_index_frame's rules); a source whose frame
 * fails or whose hash type or block size differs is skipped and counted without being uploaded;
 * the other texts go up once into one arena; cir_index_digests_dev's count pass gives every
 * text's counts (first synchronise), its emit and decode passes and cir_index_files_dev's
 * kernels fill shared digest and record buffers with the biases set, cir_match_files_dev's
 * kernels run behind them, and d_cand_src (4 bytes per file) comes down with the verdicts (second
 * synchronise) and is compacted into file_out / src_out on the host, a loop per file.
 *
 * The whole call is answered by the host rule instead -- outputs, error codes and error texts are
 * then the host's, and this is never an error -- when the device declines any uploaded text, the
 * status is CIR_FILES_COLLISION, a count passes a device limit (more than 2^31 - 1 pool files,
 * 2^32 - 1 need files or pool blocks, a text of more than 2^36 bytes), or CIR_LINKS_MATCH=host is
 * set.  Both paths give identical output, stats [5] to [7] aside.
 *
 * stats: [0] file entries of `index`, [1] candidates, [2] their bytes, [3] pool files, [4] sources
 * used, [5] table slots (0 on the host), [6] 1 if matched on the device, [7] why not: 0, or a
 * CIR_FILE_WHY_*. */
#define CIR_FILE_SOURCES_STATS_FIELDS 8
#define CIR_FILE_WHY_DECLINED 1  /* the device declined a text */
#define CIR_FILE_WHY_COLLISION 2 /* two folds collided */
#define CIR_FILE_WHY_LIMIT 3     /* a count passes a device limit */
#define CIR_FILE_WHY_ENV 4       /* CIR_LINKS_MATCH=host */
int cir_file_sources(cir_ctx* ctx, const uint8_t* index, size_t len,
                     const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                     uint64_t** file_out, uint32_t** src_out, size_t* n_out,
                     size_t* nskipped_out, uint64_t stats[CIR_FILE_SOURCES_STATS_FIELDS]);

/* Bytes of device scratch cir_match_copies_dev needs: 16 per file of either side and 4 per table
 * slot (cir_match_table_slots(n_pool_files)).  Pure; 0 when a count passes the call's limits. */
uint64_t cir_match_copies_work_bytes(uint64_t n_need_files, uint64_t n_pool_files);

/* The join behind cir_file_copies, device-resident: hardlink candidates matched by content, at
 * any path.  The record arrays (CIR_FILE_WORDS u64 each), the flat digest lists, d_src_first
 * (device u64 x (nsrc + 1)) and block_size are cir_match_files_dev's; no text arena is read, paths
 * play no part.  Pool files are ordered by source in the order given, then in index order.
 *
 * The rule (ciruela_amd/csrc/copies.hpp): need file i has a candidate only if its size is greater
 * than 0 and its bit in d_skip (device u64 x ceil(n_need_files / 64), bit i & 63 of word i / 64;
 * NULL: nothing is skipped) is 0; empty files take part on neither side.  The candidate is the
 * pool file with the smallest pool ordinal that has equal exe flag, equal size and an equal digest
 * list: the first source that holds such a file and, inside it, its first place.  One candidate at
 * most per need file; several need files may name one pool file.  d_cand_src[i] (device u32;
 * UINT32_MAX: none), d_cand_file[i] (device u64, the file ordinal inside that source; UINT64_MAX:
 * none) and d_cand_place[2 i .. 2 i + 2) (device u64: the name_off and dir_off of the candidate's
 * pool record, so that its path can be decoded without the pool records; UINT64_MAX: none) are
 * written for every need file.  d_res (device, CIR_FILES_RES_FIELDS u64): [0] CIR_FILES_OK or
 * CIR_FILES_COLLISION, [1] candidates, [2] the sum of their sizes, [3] need files.
 *
 * All on `stream` behind one memset of d_work: cir_match_files_dev's fold of both sides, build
 * (one lane per non-empty pool file into a table of pool ordinals keyed by {size, exe, the 128-bit
 * fold}: claimed by compare-and-swap when empty, lowered by an atomic minimum when the occupant's
 * key is equal, so that every occupant a slot ever has carries one key and the slot ends holding
 * the smallest ordinal with it), probe (one lane per need file, from the key's home slot to an
 * equal key or an empty slot) and cir_match_files_dev's verify, digest by digest, against
 * d_pool_verify (NULL: d_pool_digests; tests pass another array to reach the status).  Files of
 * equal content have equal keys, so once every candidate has passed the verify each is the
 * smallest ordinal among the files equal to its need file: with CIR_FILES_OK the answer is exactly
 * the rule's, whatever the seed and the timing.  A collided fold can only make a slot's minimum a
 * file that fails the verify: CIR_FILES_COLLISION, and the arrays mean nothing.  No lane waits for
 * another and every loop is bounded by an argument.  Whatever the records hold, nothing outside the
 * arrays as sized by the arguments is read or written.  Like every *_dev call it allocates
 * nothing and synchronises nothing; ctx may be NULL and is not used.
 *
 * CIR_EINVAL, decided before any HIP call: a null array with a non-zero count, a null
 * d_src_first, d_work or d_res; a digest array not 16-byte aligned; records, d_src_first, d_skip,
 * d_work, d_cand_file, d_cand_place or d_res not 8-byte aligned; d_cand_src not 4-byte aligned;
 * block_size == 0; more than 2^31 - 1 pool files, 2^32 - 1 need files or 2^32 - 1 blocks on a
 * side; work_bytes < cir_match_copies_work_bytes(n_need_files, n_pool_files). */
int cir_match_copies_dev(cir_ctx* ctx, const uint64_t* d_need_files, uint64_t n_need_files,
                         const uint8_t* d_need_digests, uint64_t n_need_blocks,
                         const uint64_t* d_pool_files, uint64_t n_pool_files,
                         const uint8_t* d_pool_digests, uint64_t n_pool_blocks,
                         const uint64_t* d_src_first, uint64_t nsrc, uint64_t block_size,
                         const uint64_t* d_skip, const uint8_t* d_pool_verify, uint64_t seed,
                         void* d_work, uint64_t work_bytes, uint32_t* d_cand_src,
                         uint64_t* d_cand_file, uint64_t* d_cand_place, uint64_t* d_res,
                         void* stream);

/* Hardlink candidates matched by content: for every file entry of `index` that is not empty and
 * whose bit in `skip` (u64 words over file ordinals; NULL: nothing is skipped) is 0, the first
 * source, in the order given, that holds a file with equal exe flag, size and digests at any
 * path, and inside that source the first such file in index order (cir_match_copies_dev's rule).
 * cir_file_sources finds a file only at its own path: below a renamed directory (/app-1.2.3
 * becomes /app-1.2.4) or for a moved file it finds nothing, and the bytes are copied
 * (cir_block_extents) where a link would do.  Run after it with skip = the files it linked, this
 * call is a pure addition.  The reference has no counterpart
 * (src/daemon/metadata/hardlink_sources.rs:121-146 matches by path).
 *
 * Candidate k: file_out[k] (file ordinal in `index`, strictly increasing), src_out[k] (source
 * ordinal as the caller counts), src_file_out[k] (file ordinal inside that source) and its path in
 * the source, decoded, in the form the index parser gives an entry's path ("/dir/name", raw
 * bytes): paths_out[path_off_out[k] .. path_off_out[k + 1]); n + 1 offsets, no terminators.  All
 * five arrays are malloc'd (cir_free) and NULL when *n_out == 0.  Sources are skipped and counted
 * in *nskipped_out (nullable) exactly as in cir_file_sources.
 *
 * With ctx == NULL the host rule runs and no GPU is needed.  With a context the flow is
 * cir_file_sources': texts framed on the host and uploaded once, the count pass (first
 * synchronise), the emit and decode passes with cir_index_files_dev's kernels and biases, the skip
 * bitmap, cir_match_copies_dev's kernels, and d_cand_src, d_cand_file, d_cand_place and the need
 * records down with the verdicts (second synchronise); the host compacts them and decodes every
 * candidate's path from the source text it holds.  The whole call is answered by the host rule
 * instead, which is never an error, in the cases named at cir_file_sources (a declined text, a
 * collision, a limit, CIR_LINKS_MATCH=host).  Both paths give identical output, stats [5] to [7]
 * aside.
 *
 * stats: [0] file entries of `index`, [1] candidates, [2] their bytes, [3] pool files, [4] sources
 * used, [5] table slots (0 on the host), [6] 1 if matched on the device, [7] why not: 0, or a
 * CIR_FILE_WHY_*, [8] need files left out by `skip`, [9] candidates whose source path equals the
 * entry's own path. */
#define CIR_FILE_COPIES_STATS_FIELDS 10
int cir_file_copies(cir_ctx* ctx, const uint8_t* index, size_t len,
                    const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                    const uint64_t* skip, uint64_t** file_out, uint32_t** src_out,
                    uint64_t** src_file_out, uint64_t** path_off_out, uint8_t** paths_out,
                    size_t* n_out, size_t* nskipped_out,
                    uint64_t stats[CIR_FILE_COPIES_STATS_FIELDS]);

/* ---- the download plan ------------------------------------------------ */

/* The glue between cir_match_files_dev and cir_match_copies_dev, device-resident
 * (ciruela_amd/csrc/plan.hpp, plan.hip): behind cir_match_files_dev's candidates, one lane per need
 * file i.  If d_deny (device u64 x ceil(n_files / 64), bit i & 63 of word i / 64; NULL: nothing is
 * denied) has bit i and d_cand_src[i] != UINT32_MAX, the candidate is withdrawn: d_cand_src[i] =
 * UINT32_MAX, d_cand_file[i] = UINT64_MAX.  d_skip (device u64 x ceil(n_files / 64)) = deny | a
 * candidate kept: the `d_skip` of cir_match_copies_dev.  Every word of d_skip is written by the
 * call, the bits at and past n_files as 0, with one aligned 64-bit store per wave; no atomic
 * touches it.  d_res (device, CIR_PLAN_LINKS_RES_FIELDS u64): [0] candidates kept, [1] withdrawn;
 * zeroed on `stream` in front of the kernel (also when n_files == 0), then one atomic add per wave
 * that has something to add.  Like every *_dev call it allocates nothing and synchronises
 * nothing; ctx may be NULL and is not used.
 *
 * CIR_EINVAL, decided before any HIP call: a null d_res; a null d_cand_src, d_cand_file or d_skip
 * with n_files > 0; d_deny, d_cand_file, d_skip or d_res not 8-byte aligned; d_cand_src not 4-byte
 * aligned; more than 2^32 - 1 files. */
#define CIR_PLAN_LINKS_RES_FIELDS 2
int cir_plan_links_dev(cir_ctx* ctx, const uint64_t* d_deny, uint64_t n_files,
                       uint32_t* d_cand_src, uint64_t* d_cand_file, uint64_t* d_skip,
                       uint64_t* d_res, void* stream);

/* The glue between cir_match_copies_dev and cir_match_extents_dev, device-resident: the `d_want`
 * of the latter, one lane per global block g < n_blocks.  d_need_runs is the new index's run table
 * (cir_index_digests_dev's, or the packed form cir_match_extents_dev takes: four u64 per non-empty
 * file {first, size, file, x}, `first` ascending; x is not read).  The table is bisected for the
 * last run with first <= g; block g is in a file iff there is one and g - first < size /
 * block_size + (size % block_size != 0).  The file is linked iff its ordinal f is below n_files
 * and d_cand_a[f] != UINT32_MAX or d_cand_b[f] != UINT32_MAX (device u32 x n_files each, either
 * may be NULL: the candidates after cir_plan_links_dev and after cir_match_copies_dev); f is
 * checked before either array is read.  The want bit is set iff the block is in a file that is not
 * linked and d_have (device u64 x ceil(n_blocks / 64), NULL: none) does not hold it.  Every word
 * of d_want [0, ceil(n_blocks / 64)) is written, the bits at and past n_blocks as 0, as in
 * cir_plan_links_dev.  d_res (device, CIR_PLAN_WANT_RES_FIELDS u64, zeroed on `stream` first): [0]
 * blocks wanted, [1] blocks of linked files, [2] blocks left out by d_have.
 *
 * A table that is sorted but lies gets the answer these words define (an ordinal >= n_files is not
 * linked; a `first` >= n_blocks covers nothing; a size of 2^64 - 1 covers every block from its
 * `first` to the next run's); an unsorted table gets an unspecified answer.  In neither case is
 * anything read or written outside the arrays as sized by the arguments.  No lane waits for
 * another and the only loop, the bisection, is bounded by n_need_runs.
 *
 * CIR_EINVAL, decided before any HIP call: a null d_res; a null d_need_runs with n_need_runs > 0
 * or d_want with n_blocks > 0; the run table, a bitmap or d_res not 8-byte aligned; a candidate
 * array not 4-byte aligned; block_size == 0; more than 2^32 - 1 blocks, runs or files. */
#define CIR_PLAN_WANT_RES_FIELDS 3
int cir_plan_want_dev(cir_ctx* ctx, const uint64_t* d_need_runs, uint64_t n_need_runs,
                      uint64_t n_blocks, uint64_t block_size, uint64_t n_files,
                      const uint32_t* d_cand_a, const uint32_t* d_cand_b, const uint64_t* d_have,
                      uint64_t* d_want, uint64_t* d_res, void* stream);

/* The whole download plan of a new image in one call: what to hardlink, what to copy from older
 * images, what to copy inside the image and what to fetch.  It is defined as this composition of
 * the four calls above (ciruela_amd/csrc/plan.hpp), none of which changes:
 *   1. L1 = cir_file_sources' candidates, minus the files in `deny`;
 *   2. L2 = cir_file_copies with skip = deny | files(L1);
 *   3. linked = files(L1) | files(L2); want1 = every block of a file entry that is not linked,
 *      minus the 1-bits of `have`;
 *   4. (E1, fetch1) = cir_block_extents with want = want1;
 *   5. (E2, fetch2) = cir_block_repeats with want = fetch1 and present = every block not in
 *      fetch1 (the linked files' blocks, the `have` blocks and the blocks E1 covers are all in
 *      place before any copy inside the image).
 * deny (u64 words over file ordinals, NULL: none): files for which no whole-file link may be
 * proposed -- a candidate failed cir_check_links on an earlier pass, or the partial directory
 * already holds an object at that path.  have (u64 words over global blocks, NULL: none): blocks
 * already present and correct (cir_check_blocks' bitmap).  Bits past the counts are ignored.
 *
 * Outputs: L1 as cir_file_sources returns its pairs (link_file_out, link_src_out); L2 as
 * cir_file_copies returns its five arrays; E1 (extents_out) and E2 (repeat_extents_out) as
 * CIR_EXTENT_WORDS-u64 extent records; fetch2 (fetch_out, ceil(*nblk_out / 64) words).  All
 * malloc'd (cir_free) and NULL when their count is 0.  Skipped sources are counted once
 * (*nskipped_out, nullable).  Errors are whatever the composition would meet first; they are
 * decided before any output is made: on error every output is NULL / 0 and the stats are zero.
 *
 * With a context every text is uploaded and parsed once (the four calls each do it again) and the
 * four joins run back to back in device memory with cir_plan_links_dev and cir_plan_want_dev
 * between them: five synchronises (the counts, the verdicts with the run tables and the
 * candidates, the two extent counts, each extent tail).  The whole call is answered by the host
 * composition -- the four calls with ctx = NULL -- when ctx == NULL, with CIR_PLAN=host, for a text
 * the device declines, a collided fold, a count past a device limit, or a new index without
 * blocks.  None of these is an error, and both paths give identical output (the stats that name
 * the path aside).
 *
 * stats: [0..8) cir_file_sources' (taken before `deny` is applied), [8..18) cir_file_copies',
 * [18..28) cir_block_extents', [28..38) cir_block_repeats', [38] same-path candidates withdrawn by
 * `deny`, [39] files linked, [40] blocks of linked files, [41] blocks left out by `have`, [42] 1
 * if planned on the device, [43] why not: 0, a CIR_FILE_WHY_* value (CIR_FILE_WHY_ENV:
 * CIR_PLAN=host), or CIR_PLAN_WHY_EMPTY. */
#define CIR_PLAN_STATS_FIELDS 44
#define CIR_PLAN_WHY_EMPTY 5 /* the new index has no block */
int cir_fetch_plan(cir_ctx* ctx, const uint8_t* index, size_t len,
                   const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                   const uint64_t* deny, const uint64_t* have, uint64_t** link_file_out,
                   uint32_t** link_src_out, size_t* nlinks_out, uint64_t** copy_file_out,
                   uint32_t** copy_src_out, uint64_t** copy_src_file_out,
                   uint64_t** copy_path_off_out, uint8_t** copy_paths_out, size_t* ncopies_out,
                   uint64_t** extents_out, size_t* nextents_out, uint64_t** repeat_extents_out,
                   size_t* nrepeats_out, uint64_t** fetch_out, uint64_t* nblk_out,
                   size_t* nskipped_out, uint64_t stats[CIR_PLAN_STATS_FIELDS]);

/* ---- content sketches: which older images are worth a plan ------------- */

/* Every planning call above takes the older images' full index texts, and those texts are its
 * cost (cir_fetch_plan with 16 sources uploads 1.77 GB).  The reference chooses its sources by
 * timestamp, the 37 most recent images of the base directory whatever they hold
 * (src/daemon/metadata/hardlink_sources.rs:66-90, "TODO make tweakable", "TODO look in cache").
 * A sketch is a fixed-size summary of an index's block digests, made once when the index is
 * registered and kept beside it (at most 40 + 8 k bytes); cir_sketch_rank orders any number of
 * candidate sources by how much of the new image each one holds, from sketches alone, so no text
 * is uploaded for an image that will not be used.  The plan stays exact: the ranking only
 * decides which texts it is given.  Nothing lives on the device between calls.
 *
 * The rule (ciruela_amd/csrc/sketch.hpp).  Key of a digest: x = 0x243F6A8885A308D3; for the four
 * little-endian u64 words w of the 32 bytes, in order: x = (x ^ w) * 0x9E3779B97F4A7C15, x ^= x >>
 * 32; the key is the full x.  Sketch of size k (1 <= k <= CIR_SKETCH_MAX_K): the k smallest
 * distinct keys of the digests of all blocks of all file entries (cir_index_digests' block list),
 * ascending; all of them when there are fewer.  The seed is fixed because sketches are stored
 * and compared across calls, and every step of the mix is invertible: an index's author can
 * choose the keys of their own digests.  That can only mislead the ranking, never the plan.
 *
 * Blob, little-endian: 8 bytes "CIRSKv1\0", u32 hash_type, u32 k, u64 block_size, u64 n_blocks,
 * u64 count, count u64 keys.  Valid iff the magic matches, 1 <= k <= 4096, count <= k, count <=
 * n_blocks, the length is exactly 40 + 8 count and the keys are strictly ascending; everything
 * that reads a blob validates it first. */
#define CIR_SKETCH_MAX_K 4096
#define CIR_SKETCH_DEFAULT_K 1024

/* The key of one 32-byte digest (0 for a null pointer).  Pure, host-only. */
uint64_t cir_sketch_key(const uint8_t* digest);

/* Ranks nsrc source sketches against the sketch of a new image.  Overlap of the need sketch N
 * and a source sketch S: t(X) = X's last key if X is full (count == k), else 2^64 - 1; tau =
 * min(t(N), t(S)); both sketches are complete below tau, so examined = the number of N's keys <=
 * tau and shared = how many of those S holds are exact over that range, and shared / examined
 * estimates the fraction of the new image's distinct blocks the source holds (it is that
 * fraction when neither sketch is full).  Sources are ordered by shared / examined descending
 * (compared by cross-multiplying in integers; examined == 0 counts as 0), ties to the lower
 * ordinal: the caller's order is kept.  order_out[0 .. *nranked_out) = the ranked source
 * ordinals, shared_out and examined_out indexed like order_out; all three hold nsrc entries.  A
 * source that is NULL, not a valid blob, or of another hash type or block size than the need is
 * left out and counted in *nskipped_out (may be NULL), as cir_link_candidates treats its
 * sources.  The sketches' k may differ.  Pure, host-only, no GPU.
 * CIR_EINVAL: a null need, nranked_out, or (with nsrc > 0) array; CIR_EPARSE: the need blob is
 * not valid. */
int cir_sketch_rank(const uint8_t* need, size_t need_len, const uint8_t* const* src,
                    const size_t* src_len, size_t nsrc, uint64_t* order_out, uint64_t* shared_out,
                    uint64_t* examined_out, size_t* nranked_out, size_t* nskipped_out);

/* Bytes of device scratch cir_sketch_digests_dev needs for n digests.  Pure. */
uint64_t cir_sketch_work_bytes(uint64_t n, uint32_t k);

/* The sketch of a digest list in device memory: d_digests = n digests of 32 bytes as
 * cir_index_digests_dev leaves them, d_keys = room for k u64.
 *
 * d_res (device, CIR_SKETCH_RES_FIELDS u64, every word written by the call): [0] CIR_SKETCH_OK
 * or CIR_SKETCH_DECLINED, [1] keys written = min(k, distinct keys), [2] n, [3] candidates the
 * selection sorted (diagnostic).  On CIR_SKETCH_OK d_keys[0 .. [1]) holds exactly the rule's
 * keys, ascending.  CIR_SKETCH_DECLINED: the device could not answer exactly inside its scratch
 * -- more than 8192 distinct keys share the k-th key's top bits (for uniformly spread keys a
 * histogram bin holds about 64), or a key's probe walk in the set passed 1024 slots; both take a
 * crafted index -- and the keys then mean nothing; the host rule answers (cir_index_sketch does
 * that).  The device never returns a wrong or short sketch with CIR_SKETCH_OK.  The keys 0 and
 * 2^64 - 1 are ordinary keys.  n == 0 is CIR_SKETCH_OK with no key.  Nothing is written past
 * d_keys[k), d_work[work_bytes) or d_res[4).
 *
 * Like every *_dev call it allocates nothing, synchronises nothing and runs on `stream` alone
 * (two memsets and four launches: insert into a set of keys with a histogram of their top bits,
 * scan the histogram, compact the candidates, sort them in LDS; no workgroup waits for another
 * and every probe walk is bounded); ctx may be NULL and is not used.
 *
 * CIR_EINVAL, decided before any HIP call: a null d_digests (with n > 0), d_keys, d_work or
 * d_res; d_digests not 16-byte aligned; d_keys, d_work or d_res not 8-byte aligned; k outside
 * [1, 4096]; n > 2^32 - 1; work_bytes < cir_sketch_work_bytes(n, k). */
#define CIR_SKETCH_RES_FIELDS 4
#define CIR_SKETCH_OK 0
#define CIR_SKETCH_DECLINED 1
int cir_sketch_digests_dev(cir_ctx* ctx, const uint8_t* d_digests, uint64_t n, uint32_t k,
                           uint64_t* d_keys, void* d_work, uint64_t work_bytes, uint64_t* d_res,
                           void* stream);

/* The sketch of an index in host memory: *blob_out = the malloc'd blob (cir_free), *blob_len its
 * length (40 bytes for an index without blocks).  With a context: cir_index_frame, one upload,
 * cir_index_digests_dev's kernels and cir_sketch_digests_dev's behind them on the context's first
 * device, and a download of the result words and at most 8 k bytes of keys -- the digests never
 * come down (cir_index_digests with a context downloads 32 bytes per block); the current device
 * is restored.  The host rule alone (the host parser, the keys, a partial sort) answers when ctx
 * == NULL, with CIR_SKETCH=host, for a text the device declines, for a declined sketch and for a
 * length the device parse does not take.  None of these is an error, and the blob is
 * byte-identical on both paths.  Error codes are cir_index_digests' (CIR_EPARSE, CIR_EHASHSIZE,
 * CIR_EINVAL -- also k outside [1, 4096] --, CIR_ENOMEM); on error *blob_out is NULL, *blob_len 0
 * and the stats are zero.
 *
 * stats: [0] 1 if the device answered, [1] why not: 0 (it did, or ctx == NULL) or a
 * CIR_SKETCH_WHY_* value, [2] blocks, [3] keys in the blob, [4] text bytes uploaded, [5] bytes
 * downloaded. */
#define CIR_SKETCH_STATS_FIELDS 6
#define CIR_SKETCH_WHY_ENV 1      /* CIR_SKETCH=host */
#define CIR_SKETCH_WHY_TEXT 2     /* the device parse declined the text */
#define CIR_SKETCH_WHY_DECLINED 3 /* CIR_SKETCH_DECLINED */
#define CIR_SKETCH_WHY_SIZE 4     /* a text longer than the device parse takes */
int cir_index_sketch(cir_ctx* ctx, const uint8_t* index, size_t len, uint32_t k,
                     uint8_t** blob_out, size_t* blob_len,
                     uint64_t stats[CIR_SKETCH_STATS_FIELDS]);

/* ---- index (DIRSIGNATURE.v1) ----------------------------------------- */

/* dir_signature::v1::scan(&ScannerConfig, &mut Vec<u8>)
 * (src/client/sync/uploads.rs:49-59; examples/custom_uploader.rs:59-65):
 * ScannerConfig{threads, hash, add_dir(dirs[i], prefixes[i])}.  threads =
 * host reader threads (gopt.threads, default 4, src/client/global_options.rs:13;
 * 0 = auto_threads).  *index_out receives the index bytes. */
int cir_scan_v1(cir_ctx* ctx, const char* const* dirs, const char* const* prefixes, size_t ndirs,
                uint64_t block_size, int hash_type, uint32_t threads, uint8_t** index_out,
                size_t* len_out);

/* The same scan writing the index out as it goes, as v1::scan writes into
 * the caller's `&mut Vec<u8>` / io::Write (src/client/sync/uploads.rs:55-57):
 * write(user, data, n) receives the index bytes in order -- the header line
 * first, then each stretch of the body as the batches complete files, the
 * footer line last -- from library threads, one call at a time.  The
 * library keeps only the unwritten tail (no whole-index buffer, no copy
 * after the scan).  A non-zero return from write stops the scan with
 * CIR_EIO (the reference's io::Error from the writer); on any error the
 * writer may have received part of an index.  *len_out (may be NULL) = the
 * bytes written. */
typedef int (*cir_write_fn)(void* user, const uint8_t* data, size_t n);
int cir_scan_v1_write(cir_ctx* ctx, const char* const* dirs, const char* const* prefixes,
                      size_t ndirs, uint64_t block_size, int hash_type, uint32_t threads,
                      cir_write_fn write, void* user, size_t* len_out);

/* dir_signature::get_hash via InMemoryIndexes::register_index
 * (src/index.rs:98-105): the image id printed on the index's last line.
 * id_out must hold 64 bytes; *id_len = decoded length (32 for v1 hashes). */
int cir_index_get_hash(const uint8_t* index, size_t len, uint8_t* id_out, size_t* id_len);

/* RawIndex::into_mut + MutableIndex::to_raw_data (src/cluster/download.rs:
 * 171-188, 266-319): parse, rebuild the directory tree and re-emit it in the
 * reference's order (files and links by name, then subdirectories; empty
 * directories dropped) with the footer recomputed in the index's hash type
 * where cir_set_footer_mode says: CIR_FOOTER_HOST (the default, as in
 * cir_scan_v1) hashes it on the calling thread, blake2b/256 and sha512/256
 * alike; CIR_FOOTER_GPU as one descriptor on the GPU. */
int cir_index_rewrite(cir_ctx* ctx, const uint8_t* in, size_t len, uint8_t** out, size_t* out_len);

/* ---- an index of files that are not in a file system ------------------- */

/* The index of a flat list of regular files, for bytes that no directory holds: tensors,
 * checkpoints, generated data.  The reference has no counterpart: its indexes come from a
 * directory scan (src/client/sync/uploads.rs:49-59) or from a parsed index re-emitted
 * (src/cluster/download.rs:266-319).  The rule is ciruela_amd/csrc/emit.hpp.
 *
 * Input, as parallel arrays in the caller's order: file i's path is paths[path_off[i] ..
 * path_off[i + 1]) (raw bytes, nfiles + 1 offsets, no terminators), its size sizes[i], its
 * executable flag exe[i] != 0 (exe == NULL: none).  Digests are one flat list of 32 bytes each,
 * file i's behind file i - 1's in that same order -- not in emission order --, sizes[i] /
 * block_size + (sizes[i] % block_size != 0) per file.
 *
 * Tree: a path is '/' followed by components separated by single '/'; no component is empty, "."
 * or ".."; no NUL byte; no path twice; no path that is both a file and a directory (the checks of
 * cir_index_rewrite's tree: InvalidPath, PathConflict).  The directories are those the paths
 * imply, plus "/".  A violation is CIR_EINVAL with the path in cir_last_error, decided before
 * anything is allocated on or sent to a device.
 *
 * Text: exactly what cir_scan_v1 emits for a directory that holds these files: the header line;
 * per directory its line, its files in bytewise name order, then its subdirectories in bytewise
 * name order, recursively; a size-0 file carries no token; the footer line is H(body).  No file
 * at all gives the body "/\n".  Symlinks and empty directories cannot be expressed.
 *
 * Layout: the body is a sequence of pieces, one per file in emission order (one piece with the
 * literal "/" when there is no file).  A piece is CIR_EMIT_PIECE_WORDS u64 {out_off, lit_off,
 * lit_len, first_block, nblk}: at body offset out_off stand lit_len bytes of the literal arena
 * from lit_off (the directory lines since the previous file, then the file line's head through
 * the size digits), then nblk tokens (' ' + 64 lower-case hex digits) of the digests first_block
 * .. first_block + nblk - 1, then '\n'. */
#define CIR_EMIT_PIECE_WORDS 5
#define CIR_EMIT_RES_FIELDS 1

/* The layout of a file list: *pieces_out (malloc'd, cir_free; *npieces pieces), *lits_out
 * (malloc'd; *lits_len bytes), first_block_out (nullable; nfiles u64: where file i's digests
 * start in the flat list), *nblocks and *body_len.  What a caller of cir_index_emit_dev uploads.
 * Pure, host-only.  CIR_EINVAL: as above, a block_size outside 1 .. 2^32-1, more than 2^31-1
 * blocks. */
int cir_index_emit_layout(uint64_t block_size, const uint8_t* paths, const uint64_t* path_off,
                          const uint64_t* sizes, const uint8_t* exe, size_t nfiles,
                          uint64_t** pieces_out, size_t* npieces, uint8_t** lits_out,
                          size_t* lits_len, uint64_t* first_block_out, uint64_t* nblocks,
                          uint64_t* body_len);

/* The body from its tables on the host: the function the kernel of cir_index_emit_dev runs, 16
 * bytes at a time, with the same guards.  body holds body_len rounded up to 16 bytes; every one
 * of them is written, the padding as 0.  res[0] = pieces whose literal range lies outside [0,
 * lits_len) or whose block range lies outside [0, ndigests): every byte of such a piece is 0 and
 * nothing is read through it (exact for tables whose out_off strictly ascends); bytes that no
 * piece covers are 0.  Pure, host-only.  CIR_EINVAL: a null array of non-zero length, npieces >
 * 2^32-1, body_len or ndigests > 2^40. */
int cir_index_emit_tables(const uint8_t* digests, uint64_t ndigests, const uint64_t* pieces,
                          uint64_t npieces, const uint8_t* lits, uint64_t lits_len, uint8_t* body,
                          uint64_t body_len, uint64_t res[CIR_EMIT_RES_FIELDS]);

/* The host form: *index_out = the malloc'd index (cir_free), *len_out its length, image_id
 * (nullable, 32 bytes) = the footer digest.  Needs no context and no device.  CIR_EINVAL: as
 * above, an unknown hash type, ndigests other than the sizes ask for. */
int cir_index_emit(int hash_type, uint64_t block_size, const uint8_t* paths,
                   const uint64_t* path_off, const uint64_t* sizes, const uint8_t* exe,
                   size_t nfiles, const uint8_t* digests, size_t ndigests, uint8_t** index_out,
                   size_t* len_out, uint8_t image_id[CIR_DIGEST_BYTES]);

/* cir_index_emit_tables on the device: digests, pieces and literals in device memory to the body
 * in device memory (d_body: 16-byte aligned, body_len rounded up to 16 bytes; d_pieces and d_res
 * 8-byte aligned).  One lane owns 16 aligned bytes of the body and stores only those, so the
 * call writes every byte of d_body[0, round_up(body_len, 16)) and d_res[0], and nothing else,
 * whatever the tables hold; d_res[0] as res[0] above (a memset and one launch).  Like every *_dev
 * call it allocates nothing, synchronises nothing and runs on `stream` alone; ctx may be NULL and
 * is not used.  CIR_EINVAL, decided before any HIP call: as cir_index_emit_tables, or a
 * misaligned pointer. */
int cir_index_emit_dev(cir_ctx* ctx, const uint8_t* d_digests, uint64_t ndigests,
                       const uint64_t* d_pieces, uint64_t npieces, const uint8_t* d_lits,
                       uint64_t lits_len, uint8_t* d_body, uint64_t body_len, uint64_t* d_res,
                       void* stream);

/* The index of files held in device memory: file i's bytes are d_data[i][0 .. sizes[i]) on the
 * device of `stream` (any alignment; ignored for a size-0 file), which must be one of ctx's.
 * The host validates the list and lays the body out; the file table (24 bytes per non-empty
 * file), the pieces and the literals go up; on `stream` a kernel writes one descriptor per block,
 * the blocks are hashed as one batch by cir_hash_blocks_dev_ht's routing over the lowest pointer
 * as the arena, and cir_index_emit_dev's kernel writes the body, which comes down; the footer is
 * hashed on the calling thread.  All of it is queued behind whatever the caller queued on
 * `stream` before: data still being produced there needs no synchronise first.  The call
 * returns after its own synchronise; its device buffers are allocated and freed inside the call
 * and nothing stays on the device; the caller's current device is restored.
 *
 * CIR_EMIT=host (read per call) hashes on the device, downloads the digests and emits with
 * cir_index_emit's code; the index is byte-identical.  CIR_TRACE=1: one "cir index_memory:" line
 * with the laps hash, emit, download, footer.
 *
 * CIR_EINVAL: as cir_index_emit, a null ctx, a device that is not ctx's, a null pointer of a
 * non-empty file, more than 2^31-1 blocks (one descriptor batch).  CIR_EIO: the emit kernel
 * counted a piece outside its arrays (the tables are the call's own: a defect).
 *
 * stats: [0] blocks, [1] 1 if the device emitted the text, 0 if the host did, [2] files, [3]
 * body bytes, [4] bytes uploaded, [5] bytes downloaded. */
#define CIR_MEMINDEX_STATS_FIELDS 6
int cir_index_memory_dev(cir_ctx* ctx, int hash_type, uint64_t block_size, const uint8_t* paths,
                         const uint64_t* path_off, const uint64_t* sizes, const uint8_t* exe,
                         size_t nfiles, const void* const* d_data, void* stream,
                         uint8_t** index_out, size_t* len_out,
                         uint8_t image_id[CIR_DIGEST_BYTES],
                         uint64_t stats[CIR_MEMINDEX_STATS_FIELDS]);

/* ---- consumers of the index (host bookkeeping) ------------------------ */

/* InMemoryIndexes (src/index.rs:53-124): ImageId -> index bytes. */
typedef struct cir_indexes cir_indexes;
cir_indexes* cir_indexes_new(void); /* NULL if out of memory */
void cir_indexes_free(cir_indexes* h);
/* register_index (src/index.rs:98-105); id_out holds 64 bytes. */
int cir_indexes_register(cir_indexes* h, const uint8_t* data, size_t len, uint8_t* id_out,
                         size_t* id_len);
/* GetIndex::read_index (src/index.rs:106-123); CIR_ENOTFOUND if absent. */
int cir_indexes_read(cir_indexes* h, const uint8_t* id, size_t id_len, uint8_t** data_out,
                     size_t* len_out);

/* ThreadedBlockReader (src/blocks.rs:85-240): BlockHash -> block bytes. */
typedef struct cir_blocks cir_blocks;
cir_blocks* cir_blocks_new(void); /* NULL if out of memory */
void cir_blocks_free(cir_blocks* h);
size_t cir_blocks_len(cir_blocks* h);
/* register_dir (src/blocks.rs:145-183): CIR_EPARSE / CIR_EHASHSIZE. */
int cir_blocks_register_dir(cir_blocks* h, const char* dir, const uint8_t* index, size_t len);
/* register_memory_blocks(HashType::blake2b_256(), ..) (src/blocks.rs:187-204),
 * hashed on the GPU. */
int cir_blocks_register_memory(cir_ctx* ctx, cir_blocks* h, const uint8_t* data, size_t len,
                               uint64_t block_size);
/* register_memory_blocks(hash_type, block_size, data) with the index's own
 * hash type (put-file, src/client/put_file/network.rs:56). */
int cir_blocks_register_memory_ht(cir_ctx* ctx, cir_blocks* h, int hash_type, const uint8_t* data,
                                  size_t len, uint64_t block_size);
/* GetBlock::read_block (src/blocks.rs:207-240); CIR_ENOTFOUND if absent. */
int cir_blocks_read(cir_blocks* h, const uint8_t hash[CIR_DIGEST_BYTES], uint8_t** data_out,
                    size_t* len_out);

/* ---- test data -------------------------------------------------------- */

/* Fill d_ptr with splitmix64 words (bench/tests only).  block_bytes == 0:
 * word k = splitmix64 output k of `seed`; otherwise block i (block_bytes
 * each, a multiple of 8) is its own stream seeded seed ^ (first_block + i). */
int cir_fill_splitmix64_dev(void* d_ptr, uint64_t nbytes, uint64_t seed, uint64_t block_bytes,
                            uint64_t first_block, void* stream);

/* ---- diagnostics (not part of the reference interface) ---------------- */

/* One launch of a uniform-block kernel variant, for A/B measurement:
 * loader 0 = LDS-DMA coalesced lines (the production loader), 1 = per-lane
 * direct loads.  nblk % 256 == 0, block_size % 128 == 0, d_data 16-B aligned. */
int cir_debug_hash_uniform_dev(int loader, const void* d_data, uint64_t block_size, uint64_t nblk,
                               uint8_t* d_out, void* stream);

/* nlanes (% 256 == 0) independent chains of `lines` BLAKE2b compressions on
 * register-resident messages, digest per lane -> d_out + 32 lane: the same
 * compression count as hashing nlanes blocks of 128 x lines bytes, with no
 * memory traffic.  bench.py times it as the measured VALU ceiling. */
int cir_debug_compress_only_dev(uint64_t nlanes, uint32_t lines, uint8_t* d_out, void* stream);

/* Per-part kernel timing of the ordered descriptor batches of ctx's first
 * device (cir_hash_blocks_dev with a context): enable != 0 starts recording
 * HIP events around the ordering, the quad part and the lane part of each
 * batch (at most 256 batches per enable; enabling again restarts), 0 stops.
 * cir_debug_desc_times waits for the recorded events and returns
 * out[0] = batches, out[1..3] = summed ordering / quad-part / lane-part
 * milliseconds, out[4] = summed ordering start -> last part end. */
int cir_debug_desc_timing(cir_ctx* ctx, int enable);
int cir_debug_desc_times(cir_ctx* ctx, double out[5]);

/* Where cir_scan_v1 and cir_index_rewrite hash an index's footer (the
 * ImageId, H(every byte after the header line), src/index.rs:98-105): one
 * serial chain over the index text, ~65 B per 32 KiB block.  CIR_FOOTER_HOST
 * (the default): a host thread hashes the text as the scan emits it
 * (blake2b/256 and sha512/256).  CIR_FOOTER_GPU: the resumable single-chain
 * kernel (quad mode) on device 0's chain stream for blake2b/256, one lane at
 * the end for sha512/256.  Block digests are always computed on the GPU. */
enum cir_footer_mode { CIR_FOOTER_HOST = 0, CIR_FOOTER_GPU = 1 };
int cir_set_footer_mode(cir_ctx* ctx, int mode);

/* Staged-scan timing of ctx (cir_scan_v1): enable != 0 clears the record and
 * starts recording, 0 stops.  While on, every staged batch adds one row of
 * CIR_SCAN_BATCH_FIELDS doubles:
 *   [0] device index in ctx  [1] bytes  [2] blocks
 *   [3] host wait for the slot (ms)
 *   [4] reads start  [5] reads end            (ms since the scan started)
 *   [6] H2D start    [7] H2D end              (HIP events on the copy stream)
 *   [8] hash start   [9] digests back on host (HIP events, compute stream)
 * and every scan sets CIR_SCAN_PHASE_FIELDS doubles:
 *   [0] walk ms  [1] hash loop ms  [2] last emit ms
 *   [3] footer tail ms (hash loop end -> footer digest)  [4] output ms
 *   [5] footer busy ms (host thread hashing, or summed chain-kernel time)
 *   [6] footer mode  [7] batches  [8] index bytes  [9] footer feeds.
 * cir_debug_scan_batches copies at most max_rows rows and sets *nrows to the
 * number recorded. */
#define CIR_SCAN_BATCH_FIELDS 10
#define CIR_SCAN_PHASE_FIELDS 10
int cir_debug_scan_timing(cir_ctx* ctx, int enable);
int cir_debug_scan_batches(cir_ctx* ctx, double* rows, size_t max_rows, size_t* nrows);
int cir_debug_scan_phases(cir_ctx* ctx, double out[CIR_SCAN_PHASE_FIELDS]);

/* The footer's host BLAKE2b-256 / SHA-512/256 fed in `piece`-byte updates
 * (0 = one update): no device involved; the CPU tests check them against
 * the oracle. */
int cir_debug_host_blake2b256(const uint8_t* p, size_t n, size_t piece,
                              uint8_t out[CIR_DIGEST_BYTES]);
int cir_debug_host_sha512_256(const uint8_t* p, size_t n, size_t piece,
                              uint8_t out[CIR_DIGEST_BYTES]);

/* Identity of HIP device `device` as its driver and its own counters see it
 * (the multi-GPU bench puts every rank's into its line): the PCI bus id
 * (hipDeviceGetPCIBusId, into pci_bus_id, len >= 13), the UUID
 * (hipDeviceGetUuid), and one wave's reads of the device's wall clock and
 * shader clock counters ~100 us apart: clocks[0], [1] = wall clock before /
 * after, [2], [3] = shader clock counter before / after, [4] = the wall
 * clock's rate in kHz.  Synchronous; allocates and frees 32 bytes. */
int cir_debug_device_identity(int device, char* pci_bus_id, size_t len, uint8_t uuid[16],
                              uint64_t clocks[5]);

/* How many whole blocks of a file of nfull x block_size bytes (plus any short
 * last block) cir_hash_chunks_dev with a context relays on the calling
 * thread's current device (0: none).  Relayed blocks run in quad mode as
 * segmented chains beside k whole lane (or quad) waves per SIMD. */
uint64_t cir_debug_relay_blocks(uint64_t nfull, uint64_t block_size);

#ifdef __cplusplus
}
#endif

#endif /* CIRUELA_BLOCKHASH_H */
