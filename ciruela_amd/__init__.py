"""ciruela_amd — MI355X-native block-indexing path of tailhook/ciruela.

Python mirror of the reference's public interface for the indexing path,
over the C ABI in include/ciruela_blockhash.h (libciruela_amd.so).  Names,
argument meaning and error behaviour follow the reference:

=============================  ==============================================
this module                     reference (tailhook/ciruela v0.6.12)
=============================  ==============================================
BlockHash                       ciruela::blocks::BlockHash (src/block_id.rs:19)
BlockHash.hash_bytes            BlockHash::hash_bytes (src/block_id.rs:37-43)
ImageId                         ciruela::index::ImageId (src/id.rs:142)
HashType                        dir_signature::HashType (external 0.2.9)
Hashes.hash_file                dir_signature::v1::Hashes::hash_file
ScannerConfig, v1.scan          dir_signature::{ScannerConfig, v1::scan}
                                (src/client/sync/uploads.rs:49-59)
get_hash                        dir_signature::get_hash (src/index.rs:99)
InMemoryIndexes                 ciruela::index::InMemoryIndexes (src/index.rs:53)
ThreadedBlockReader             ciruela::blocks::ThreadedBlockReader
                                (src/blocks.rs:85)
Context.verify_blocks[_dev]     FetchBlock::poll's `hash_bytes(..) == blk.hash`
                                (src/daemon/tracking/fetch_blocks.rs:77), batched
Context.verify_submit / poll /  the same check per block, batched by the library,
  wait / forget / limits        bounded (CIR_EAGAIN backpressure, forgotten tickets)
Context.check_file              Hashes::check_file (src/daemon/disk/commit.rs:104)
Context.check_index,            commit_image's re-hash loop over a whole image, batched
  check_index                   (src/daemon/disk/commit.rs:51-117)
Context.verify_first_dev        the same compare on the device, answering only "which
                                block first" (src/daemon/disk/commit.rs:51-117)
link_candidates                 scan_links: which files of a new image older images
                                hold (src/daemon/metadata/hardlink_sources.rs:107-153)
Context.check_links,            check_and_hardlink's re-hash and mode test of every
  check_links                   candidate, batched, one verdict per candidate
                                (src/daemon/disk/public.rs:285-346)
Context.verify_segments_dev     the same compare on the device, one flag per segment
                                (src/daemon/disk/public.rs:285-346)
Context.check_blocks,           what "Resuming download" lacks: which blocks a partial
  check_blocks                  image already holds, one bit per block, so that
                                fill_blocks need not queue everything again
                                (src/daemon/tracking/mod.rs:561-585,
                                src/daemon/disk/public.rs:91-93,
                                src/daemon/tracking/progress.rs:129-170)
Context.verify_bitmap_dev       the same compare on the device, one bit per block
block_sources                   what fill_blocks lacks: which of the blocks it queues an
                                older local image already holds, and where
                                (src/daemon/tracking/progress.rs:129-170; scan_links
                                matches whole files only, src/daemon/metadata/
                                hardlink_sources.rs:131-133)
Context.match_digests_dev       the join behind it on the device: per needed digest the
                                smallest ordinal of an equal digest in a pool
block_extents                   the same answer merged into extents (one copy_file_range
                                each) with the bitmap of what is left to fetch; the
                                reference has no counterpart
                                (src/daemon/tracking/progress.rs:129-170)
Context.match_extents_dev       the mapping and the merge behind it on the device
block_repeats                   what is left after that: blocks whose digest another block
                                of the same image carries are copied inside the image
                                instead of fetched twice; the reference has no
                                counterpart (src/daemon/tracking/progress.rs:129-170)
Context.match_repeats_dev       the join behind it on the device: per wanted block the
                                leader of its digest among the image's own blocks
file_sources,                   link_candidates' rule with the texts parsed and the files
  Context.index_files_dev,      joined on the device: file records, a fold of each
  Context.match_files_dev       file's digests, a table keyed by (source, path)
                                (src/daemon/metadata/hardlink_sources.rs:107-153)
file_copies,                    the step behind it: candidates matched by content at any
  Context.match_copies_dev      path (a renamed directory, a moved file), the first
                                source and the first place inside it; a table keyed by
                                {size, exe, fold}; the reference has no counterpart
                                (src/daemon/metadata/hardlink_sources.rs:121-146)
check_links_at,                 check_links with a place per candidate: the verify of a
  Context.check_links_at        file_copies candidate at the path where the source
                                holds it (src/daemon/disk/public.rs:308-346 with
                                another path)
fetch_plan,                     the four answers above as one download plan: links at the
  Context.plan_links_dev,       same path, links by content, extents from older images,
  Context.plan_want_dev         extents inside the image and the bitmap left to fetch,
                                with every text uploaded and parsed once; the reference
                                plans nothing (src/daemon/metadata/
                                hardlink_sources.rs:107-153, src/daemon/tracking/
                                progress.rs:129-170)
index_digests,                  what every consumer of an index starts with: its block
  Context.index_digests_dev     digests as one array and a run record per non-empty
                                file, parsed on the device (the reference parses the
                                text on a host thread: src/blocks.rs:150-183)
index_sketch, sketch_rank,      the question before the plan: which older images are
  sketch_key,                   worth handing to it.  A fixed-size content sketch per
  Context.sketch_digests_dev    index (the k smallest distinct keys of its block
                                digests, made on the device behind the parse) and a
                                host-only ranking of candidate sources from sketches
                                alone; the reference takes the 37 most recent images
                                by timestamp (src/daemon/metadata/
                                hardlink_sources.rs:66-90)
index_memory, index_emit,       the index and ImageId of files that no directory holds:
  index_emit_layout,            bytes in device memory (tensors, checkpoints) hashed
  Context.index_emit_dev        where they lie and the text written by the device, the
                                inverse of index_digests; equal to v1.scan of a
                                directory holding the same files (the reference indexes
                                directories only: src/client/sync/uploads.rs:49-59)
load_image,                     the way back: an image directory read into device
  Context.load_blocks           buffers and verified there, check_blocks that keeps
                                what it read (the reference's consumers read committed
                                files unchecked: src/daemon/disk/commit.rs:51-117)
reload_image,                   load_image for a process that holds the previous
  Context.reload_blocks         version in device memory: the blocks its buffers
                                already hold are copied on the device, the rest read
update_image,                   the same in the tensors that hold the previous
  Context.update_blocks         version: blocks already in place are left alone, the
                                others move through a staging scratch where they must
=============================  ==============================================

All hashing runs on gfx950 through the library; there is no CPU fallback.
"""
import collections
import ctypes
import os
import threading

from . import _native as _n
from ._native import CiruelaError, NoDevice  # noqa: F401

__all__ = [
    "BlockHash", "ImageId", "HashType", "Hashes", "ScannerConfig", "v1", "get_hash",
    "InMemoryIndexes", "ThreadedBlockReader", "BlockHint", "Context", "default_context",
    "IndexError_", "DirError", "ReadError", "CiruelaError", "NoDevice", "sha512_256",
    "check_index", "CheckResult", "link_candidates", "check_links", "LinksResult",
    "check_blocks", "BlocksResult", "block_sources", "SourcesResult",
    "block_extents", "ExtentsResult", "Extent",
    "block_repeats", "RepeatsResult",
    "index_digests", "IndexDigests", "file_sources", "file_copies", "check_links_at",
    "fetch_plan", "PlanResult", "index_sketch", "sketch_rank", "sketch_key",
    "index_memory", "index_emit", "index_emit_layout", "index_emit_tables", "load_image",
    "reload_image", "update_image",
    "store_image",
]

DEFAULT_BLOCK_SIZE = 32768


def _buf(data):
    """(pointer, keepalive) for any contiguous buffer (bytes, bytearray,
    memoryview, numpy array, mmap), without copying it."""
    import numpy as np
    try:
        mv = memoryview(data)
    except TypeError:
        raise TypeError("expected a bytes-like object, got %r" % type(data)) from None
    if not mv.c_contiguous:
        raise ValueError("buffer must be C-contiguous")
    mv = mv.cast("B")
    if mv.nbytes == 0:
        return None, b""
    arr = np.frombuffer(mv, dtype=np.uint8)
    return ctypes.c_void_p(arr.ctypes.data), (arr, mv)


class Context:
    """A cir_ctx: the devices the host-memory entry points run on."""

    def __init__(self, device_mask=0, staging_bytes=0, max_devices=0, one_shot=False):
        """max_devices: open at most that many of the masked devices (0 = all;
        cir_init_n).  devices_for_bytes() gives the count an input can use.
        one_shot: CIR_INIT_ONE_SHOT -- one stream and one staging slot per
        device, for one short job (the CLI's small inputs)."""
        h = ctypes.c_void_p()
        _n.check(_n.lib.cir_init_n(ctypes.byref(h), device_mask, staging_bytes, max_devices,
                                   _n.CIR_INIT_ONE_SHOT if one_shot else 0))
        self._h = h

    @staticmethod
    def devices_for_bytes(work_bytes, staging_bytes=0, visible=None):
        """cir_devices_for_bytes: ceil(work / (2 x staging)) capped at the
        visible count (no HIP call when `visible` is given)."""
        if visible is None:
            visible = _n.lib.cir_device_count()
        return _n.lib.cir_devices_for_bytes(work_bytes, staging_bytes, visible)

    @property
    def handle(self):
        return self._h

    def devices(self):
        ids = (ctypes.c_int * 64)()
        n = _n.lib.cir_ctx_devices(self._h, ids, 64)
        return list(ids[:n])

    def close(self):
        if self._h:
            _n.lib.cir_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- device-resident entry points (pointers are device addresses) ----
    def hash_chunks_dev(self, d_data, nbytes, block_size, d_out, stream=0):
        _n.check(_n.lib.cir_hash_chunks_dev(self._h, d_data, nbytes, block_size, d_out, stream))

    def hash_blocks_dev(self, d_arena, d_off, d_len, nblk, d_out, stream=0, hash_type=None):
        ht = (hash_type or HashType.blake2b_256()).code
        _n.check(_n.lib.cir_hash_blocks_dev_ht(self._h, ht, d_arena, d_off, d_len, nblk, d_out,
                                               stream))

    def hash_blocks_dev_bounded(self, d_arena, arena_bytes, d_off, d_len, nblk, d_out,
                                d_nrange=0, stream=0, hash_type=None):
        """hash_blocks_dev over untrusted descriptors: a block past
        arena_bytes is not read, its digest is zeros, *d_nrange counts them."""
        ht = (hash_type or HashType.blake2b_256()).code
        _n.check(_n.lib.cir_hash_blocks_dev_bounded(self._h, ht, d_arena, arena_bytes, d_off,
                                                    d_len, nblk, d_out, d_nrange, stream))

    # ---- host-memory entry points ----------------------------------------
    def hash_blocks(self, arena, offsets, lengths, hash_type=None):
        """Digests (n x 32 bytes) of arena[off[i] : off[i] + len[i]]."""
        ht = (hash_type or HashType.blake2b_256()).code
        n = len(offsets)
        if len(lengths) != n:
            raise ValueError("offsets and lengths differ in length")
        for o, ln in zip(offsets, lengths):
            if o < 0 or ln < 0 or o + ln > len(arena):
                raise ValueError("block outside the arena")
            if ln > 0xFFFFFFFF:
                raise ValueError("block longer than 2^32 - 1 bytes")
        out = ctypes.create_string_buffer(32 * max(n, 1))
        if n == 0:
            return b""
        offs = (ctypes.c_uint64 * n)(*offsets)
        lens = (ctypes.c_uint32 * n)(*lengths)
        ptr, keep = _buf(arena) if len(arena) else (ctypes.c_void_p(0), None)
        if ptr is None:
            one = ctypes.create_string_buffer(1)
            ptr, keep = ctypes.cast(one, ctypes.c_void_p), one
        _n.check(_n.lib.cir_hash_blocks_ht(self._h, ht, ptr, offs, lens, n, out))
        del keep
        return out.raw[:32 * n]

    def hash_file(self, fd, block_size, hash_type=None):
        ht = (hash_type or HashType.blake2b_256()).code
        size = ctypes.c_uint64()
        hp = ctypes.c_void_p()
        nh = ctypes.c_size_t()
        _n.check(_n.lib.cir_hash_file_ht(self._h, ht, fd, block_size, ctypes.byref(size),
                                         ctypes.byref(hp), ctypes.byref(nh)))
        return size.value, _n.take_buffer(hp.value, 32 * nh.value)

    def hash_memory(self, data, block_size, hash_type=None):
        ht = (hash_type or HashType.blake2b_256()).code
        ptr, keep = _buf(data)
        hp = ctypes.c_void_p()
        nh = ctypes.c_size_t()
        _n.check(_n.lib.cir_hash_memory_ht(self._h, ht, ptr, len(data), block_size,
                                           ctypes.byref(hp), ctypes.byref(nh)))
        del keep
        return _n.take_buffer(hp.value, 32 * nh.value)

    # ---- verification (daemon side, fetch_blocks.rs:77 / commit.rs:104) --
    def verify_blocks(self, arena, offsets, lengths, expected, hash_type=None):
        """Per block: does H(arena[off:off+len]) equal expected[32 i:32 i+32]?"""
        ht = (hash_type or HashType.blake2b_256()).code
        n = len(offsets)
        if len(lengths) != n or len(expected) != 32 * n:
            raise ValueError("offsets, lengths and expected digests disagree in length")
        for o, ln in zip(offsets, lengths):
            if o < 0 or ln < 0 or o + ln > len(arena):
                raise ValueError("block outside the arena")
            if ln > 0xFFFFFFFF:
                raise ValueError("block longer than 2^32 - 1 bytes")
        if n == 0:
            return []
        offs = (ctypes.c_uint64 * n)(*offsets)
        lens = (ctypes.c_uint32 * n)(*lengths)
        ptr, keep = _buf(arena) if len(arena) else (None, None)
        if ptr is None:
            one = ctypes.create_string_buffer(1)
            ptr, keep = ctypes.cast(one, ctypes.c_void_p), one
        exp = ctypes.create_string_buffer(bytes(expected), 32 * n)
        ok = ctypes.create_string_buffer(n)
        nbad = ctypes.c_size_t()
        _n.check(_n.lib.cir_verify_blocks(self._h, ht, ptr, offs, lens, n, exp, ok,
                                          ctypes.byref(nbad)))
        del keep
        return [b == 1 for b in ok.raw]

    def verify_blocks_bounded(self, arena, offsets, lengths, expected, hash_type=None):
        """verify_blocks for descriptors from untrusted data: nothing is
        checked here; a block outside the arena is not read and is False."""
        ht = (hash_type or HashType.blake2b_256()).code
        n = len(offsets)
        if len(lengths) != n or len(expected) != 32 * n:
            raise ValueError("offsets, lengths and expected digests disagree in length")
        if n == 0:
            return []
        offs = (ctypes.c_uint64 * n)(*offsets)
        lens = (ctypes.c_uint32 * n)(*lengths)
        ptr, keep = _buf(arena) if len(arena) else (None, None)
        exp = ctypes.create_string_buffer(bytes(expected), 32 * n)
        ok = ctypes.create_string_buffer(n)
        nbad = ctypes.c_size_t()
        _n.check(_n.lib.cir_verify_blocks_bounded(self._h, ht, ptr, len(arena), offs, lens, n, exp,
                                                  ok, ctypes.byref(nbad)))
        del keep
        return [b == 1 for b in ok.raw]

    def verify_blocks_dev(self, d_arena, d_off, d_len, nblk, d_expected, d_digests, d_ok=0,
                          d_nbad=0, stream=0, hash_type=None):
        ht = (hash_type or HashType.blake2b_256()).code
        _n.check(_n.lib.cir_verify_blocks_dev(self._h, ht, d_arena, d_off, d_len, nblk,
                                              d_expected, d_digests, d_ok, d_nbad, stream))

    def verify_blocks_dev_bounded(self, d_arena, arena_bytes, d_off, d_len, nblk, d_expected,
                                  d_digests, d_ok=0, d_nbad=0, stream=0, hash_type=None):
        """verify_blocks_dev over untrusted descriptors: a block past
        arena_bytes is not read and counts as a mismatch."""
        ht = (hash_type or HashType.blake2b_256()).code
        _n.check(_n.lib.cir_verify_blocks_dev_bounded(self._h, ht, d_arena, arena_bytes, d_off,
                                                      d_len, nblk, d_expected, d_digests, d_ok,
                                                      d_nbad, stream))

    def verify_first_dev(self, d_arena, arena_bytes, d_off, d_len, nblk, d_expected, d_digests,
                         d_first, d_nbad=0, stream=0, hash_type=None):
        """verify_blocks_dev_bounded answering only "which block first":
        *d_first (device u64) = the smallest mismatching or out-of-range b,
        2^64-1 when none; *d_nbad (device u32, optional) = how many.  Both
        are written by the call.  arena_bytes = 2^64-1: trusted descriptors."""
        ht = (hash_type or HashType.blake2b_256()).code
        _n.check(_n.lib.cir_verify_first_dev(self._h, ht, d_arena, arena_bytes, d_off, d_len,
                                             nblk, d_expected, d_digests, d_first, d_nbad, stream))

    def verify_segments_dev(self, d_arena, arena_bytes, d_off, d_len, nblk, d_expected, d_digests,
                            d_seg_end, nseg, d_seg_bad, d_nbad_seg=0, stream=0, hash_type=None):
        """verify_first_dev with one verdict per segment: segment s is the
        blocks [d_seg_end[s-1], d_seg_end[s]) (device u32 x nseg, non-decreasing,
        the last one nblk); d_seg_bad[s] (device bytes) = 1 when any block of
        s mismatches or is out of range, else 0; *d_nbad_seg (device u32,
        optional) = how many segments are bad.  All written by the call."""
        ht = (hash_type or HashType.blake2b_256()).code
        _n.check(_n.lib.cir_verify_segments_dev(self._h, ht, d_arena, arena_bytes, d_off, d_len,
                                                nblk, d_expected, d_digests, d_seg_end, nseg,
                                                d_seg_bad, d_nbad_seg, stream))

    def verify_bitmap_dev(self, d_arena, arena_bytes, d_off, d_len, nblk, d_expected, d_digests,
                          d_have, d_nbad=0, stream=0, hash_type=None):
        """verify_first_dev with one bit per block: bit (b & 63) of
        d_have[b >> 6] (device u64 x ceil(nblk / 64)) = 1 when block b matches
        and is in range; the last word's bits past nblk are 0 and nothing past
        that word is written.  *d_nbad (device u32, optional) = how many bits
        are 0.  All written by the call."""
        ht = (hash_type or HashType.blake2b_256()).code
        _n.check(_n.lib.cir_verify_bitmap_dev(self._h, ht, d_arena, arena_bytes, d_off, d_len,
                                              nblk, d_expected, d_digests, d_have, d_nbad, stream))

    @staticmethod
    def match_table_slots(n_pool):
        """cir_match_table_slots: the u32 slots match_digests_dev's table needs."""
        return _n.lib.cir_match_table_slots(n_pool)

    def match_digests_dev(self, d_need, n_need, d_pool, n_pool, d_table, table_slots, seed,
                          d_match, d_nmatch=0, stream=0):
        """The join behind block_sources on device-resident digests:
        d_match[i] (device u32) = the smallest j < n_pool with pool[j] ==
        need[i] over all 32 bytes, or 2^32-1; *d_nmatch (device u32, optional)
        = how many matched.  d_table: table_slots u32 of scratch (a power of
        two >= match_table_slots(n_pool)) that the call initialises; a caller
        that joins untrusted digests passes an unpredictable seed.  All
        written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_match_digests_dev(self._h, d_need, n_need, d_pool, n_pool, d_table,
                                              table_slots, seed, d_match, d_nmatch, stream))

    @staticmethod
    def extents_work_bytes(n_need):
        """cir_extents_work_bytes: the scratch match_extents_dev needs."""
        return _n.lib.cir_extents_work_bytes(n_need)

    def match_extents_dev(self, d_match, n_need, d_need_runs, n_need_runs, d_pool_runs,
                          n_pool_runs, n_pool, block_size, d_work, work_bytes, d_res, d_want=0,
                          d_src=0, d_file=0, d_block=0, d_fetch=0, d_extents=0, cap_extents=0,
                          stream=0):
        """match_digests_dev's d_match mapped back to files and merged into
        extents on the device (cir_match_extents_dev): run tables of four u64
        per non-empty file {first, size, file, x} (x: the source ordinal in
        the pool's); d_res: 6 u64 {status, wanted, found, bytes, dropped,
        extents}; d_extents: eight u64 per record {first, count, need_file,
        need_block, src, src_file, src_block, bytes}, none written when there
        are more than cap_extents; d_fetch: the bitmap of the wanted blocks
        that were not found; d_src / d_file / d_block: block_sources' arrays,
        all three or none.  d_work: extents_work_bytes(n_need) bytes.  All
        written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_match_extents_dev(self._h, d_match, n_need, d_need_runs, n_need_runs,
                                              d_pool_runs, n_pool_runs, n_pool, block_size,
                                              d_want, d_src, d_file, d_block, d_fetch, d_extents,
                                              cap_extents, d_work, work_bytes, d_res, stream))

    def match_repeats_dev(self, d_digests, n, d_table, table_slots, seed, d_match, d_want=0,
                          d_present=0, d_nmatch=0, stream=0):
        """The join behind block_repeats on device-resident digests
        (cir_match_repeats_dev): d_match[g] (device u32) = 2^32-1 when block g
        is not wanted or leads its digest, else the leader L as an ordinal of
        a pool of 2n -- L when it is present, n + L when it is a wanted block;
        *d_nmatch (device u32, optional) = how many are repeats.  d_want /
        d_present: bitmaps (u64 words, optional).  d_table: table_slots u32 of
        scratch (a power of two >= match_table_slots(n)) that the call
        initialises.  All written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_match_repeats_dev(self._h, d_digests, n, d_want, d_present, d_table,
                                              table_slots, seed, d_match, d_nmatch, stream))

    def index_digests_dev(self, d_text, length, body_off, body_end, block_size, d_digests,
                          cap_blocks, d_runs, cap_runs, d_work, work_bytes, d_res, stream=0):
        """A device-resident index text to device-resident digests and run
        records (cir_index_digests_dev): the body [body_off, body_end) as
        index_frame gives it; d_res: 5 u64 {status, file entries, runs,
        blocks, first declined line}; d_work: index_work_bytes(length) bytes.
        cap_blocks = length // 65 and cap_runs = length // 73 always suffice.
        All written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_index_digests_dev(self._h, d_text, length, body_off, body_end,
                                              block_size, d_digests, cap_blocks, d_runs,
                                              cap_runs, d_work, work_bytes, d_res, stream))

    def sketch_digests_dev(self, d_digests, n, k, d_keys, d_work, work_bytes, d_res, stream=0):
        """The content sketch of n device-resident digests
        (cir_sketch_digests_dev): d_keys = room for k u64; d_res: 4 u64
        {CIR_SKETCH_OK or CIR_SKETCH_DECLINED, keys written, n, candidates
        sorted}; d_work: sketch_work_bytes(n, k) bytes.  All written by the
        call, on `stream` alone."""
        _n.check(_n.lib.cir_sketch_digests_dev(self._h, d_digests, n, k, d_keys, d_work,
                                               work_bytes, d_res, stream))

    @staticmethod
    def sketch_work_bytes(n, k=_n.CIR_SKETCH_DEFAULT_K):
        return _n.lib.cir_sketch_work_bytes(n, k)

    def index_emit_dev(self, d_digests, ndigests, d_pieces, npieces, d_lits, lits_len, d_body,
                       body_len, d_res, stream=0):
        """The body text of an index from device-resident digests, pieces and
        literals (cir_index_emit_dev; index_emit_layout gives the tables):
        every byte of d_body[0, body_len rounded up to 16) and d_res[0] (the
        count of pieces whose ranges lie outside the arrays; their bytes are 0)
        is written, nothing else, on `stream` alone."""
        _n.check(_n.lib.cir_index_emit_dev(self._h, d_digests, ndigests, d_pieces, npieces, d_lits,
                                           lits_len, d_body, body_len, d_res, stream))

    def index_files_dev(self, d_text, length, body_off, body_end, block_size, d_files,
                        cap_files, d_work, work_bytes, d_res, off_bias=0, block_bias=0,
                        stream=0):
        """A device-resident index text to one record of 4 u64 per file entry
        (cir_index_files_dev): {name_off + off_bias, dir_off + off_bias, size,
        (first + block_bias) | exe << 63}, size-0 entries included.  d_res: 4
        u64 {status, file entries, blocks, first declined line}; d_work:
        cir_index_files_work_bytes(length) bytes; cap_files = length // 8
        always suffices.  All written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_index_files_dev(self._h, d_text, length, body_off, body_end,
                                            block_size, off_bias, block_bias, d_files, cap_files,
                                            d_work, work_bytes, d_res, stream))

    def match_files_dev(self, need, pool, d_src_first, nsrc, block_size, seed, d_work,
                        work_bytes, d_cand_src, d_cand_file, d_res, d_pool_verify=0, stream=0):
        """The join behind file_sources on device-resident records
        (cir_match_files_dev).  need / pool: (d_text, text_len, d_files,
        n_files, d_digests, n_blocks); d_src_first: nsrc + 1 u64, the first pool
        file ordinal of each source.  d_cand_src[i] (u32; 2^32-1: none) and
        d_cand_file[i] (u64, the ordinal inside that source) per need file;
        d_res: 4 u64 {status, candidates, their bytes, need files}.  d_work:
        cir_match_files_work_bytes(n_need_files, n_pool_files) bytes that the
        call initialises.  All written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_match_files_dev(self._h, *need, *pool, d_src_first, nsrc, block_size,
                                            d_pool_verify, seed, d_work, work_bytes, d_cand_src,
                                            d_cand_file, d_res, stream))

    def match_copies_dev(self, need, pool, d_src_first, nsrc, block_size, seed, d_work,
                         work_bytes, d_cand_src, d_cand_file, d_cand_place, d_res, d_skip=0,
                         d_pool_verify=0, stream=0):
        """The join behind file_copies on device-resident records
        (cir_match_copies_dev).  need / pool: (d_files, n_files, d_digests,
        n_blocks); d_src_first: nsrc + 1 u64.  Per need file that is not empty
        and whose bit in d_skip (u64 words over file ordinals; 0: none) is
        clear, the pool file of the smallest ordinal with equal exe flag, size
        and digests, at any path: d_cand_src[i] (u32; 2^32-1: none),
        d_cand_file[i] (u64, the ordinal inside that source) and
        d_cand_place[2 i ..] (u64: that pool record's name_off and dir_off);
        d_res: 4 u64 {status, candidates, their bytes, need files}.  d_work:
        cir_match_copies_work_bytes(n_need_files, n_pool_files) bytes that the
        call initialises.  All written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_match_copies_dev(self._h, *need, *pool, d_src_first, nsrc, block_size,
                                             d_skip, d_pool_verify, seed, d_work, work_bytes,
                                             d_cand_src, d_cand_file, d_cand_place, d_res, stream))

    def plan_links_dev(self, d_cand_src, d_cand_file, n_files, d_skip, d_res, d_deny=0,
                       stream=0):
        """The glue between match_files_dev and match_copies_dev
        (cir_plan_links_dev): the candidates of the files whose bit in d_deny
        (u64 words over file ordinals; 0: none) is set are withdrawn
        (d_cand_src[i] = 2^32-1, d_cand_file[i] = 2^64-1), and d_skip
        (ceil(n_files / 64) u64, every word written) = deny | candidate kept,
        match_copies_dev's d_skip.  d_res: 2 u64 {kept, withdrawn}.  All
        written by the call, on `stream` alone."""
        _n.check(_n.lib.cir_plan_links_dev(self._h, d_deny, n_files, d_cand_src, d_cand_file,
                                           d_skip, d_res, stream))

    def plan_want_dev(self, d_need_runs, n_need_runs, n_blocks, block_size, n_files, d_want,
                      d_res, d_cand_a=0, d_cand_b=0, d_have=0, stream=0):
        """The glue between match_copies_dev and match_extents_dev
        (cir_plan_want_dev): d_want (ceil(n_blocks / 64) u64, every word
        written) = the blocks of the file entries of the run table d_need_runs
        (4 u64 per non-empty file, `first` ascending) whose file has a candidate
        in neither d_cand_a nor d_cand_b (u32 x n_files; 0: no array) and whose
        bit in d_have (0: none) is clear.  d_res: 3 u64 {wanted, blocks of
        linked files, left out by have}.  All written by the call, on `stream`
        alone."""
        _n.check(_n.lib.cir_plan_want_dev(self._h, d_need_runs, n_need_runs, n_blocks, block_size,
                                          n_files, d_cand_a, d_cand_b, d_have, d_want, d_res,
                                          stream))

    # ---- asynchronous per-block verify (FetchBlock::poll, fetch_blocks.rs:77)
    def verify_submit(self, data, expected, hash_type=None):
        """Queue one block with its expected digest; returns a ticket."""
        ht = (hash_type or HashType.blake2b_256()).code
        if len(expected) != 32:
            raise ValueError("expected digest must be 32 bytes")
        ptr, keep = _buf(data) if len(data) else (ctypes.c_void_p(0), None)
        exp = ctypes.create_string_buffer(bytes(expected), 32)
        t = ctypes.c_uint64()
        _n.check(_n.lib.cir_verify_submit(self._h, ht, ptr, len(data), exp, ctypes.byref(t)))
        del keep
        return t.value

    def verify_poll(self, ticket):
        """None while pending, else True (match) / False (mismatch)."""
        st = ctypes.c_int()
        _n.check(_n.lib.cir_verify_poll(self._h, ticket, ctypes.byref(st)))
        return None if st.value == 0 else st.value == 1

    def verify_wait(self, ticket):
        ok = ctypes.c_int()
        _n.check(_n.lib.cir_verify_wait(self._h, ticket, ctypes.byref(ok)))
        return ok.value == 1

    def verify_window(self, window_us, max_batch=4096):
        _n.check(_n.lib.cir_verify_window(self._h, window_us, max_batch))

    def verify_forget(self, ticket):
        """Drop a ticket (pending or finished) whose outcome is not wanted."""
        _n.check(_n.lib.cir_verify_forget(self._h, ticket))

    def verify_limits(self, max_bytes=0, max_results=0, nonblocking=False):
        """Bound the queue (block bytes accepted, not yet verified) and the
        outcomes held; 0 = the library default.  nonblocking: a submit that
        would pass max_bytes raises CiruelaError(CIR_EAGAIN) instead of
        waiting."""
        _n.check(_n.lib.cir_verify_limits(self._h, max_bytes, max_results,
                                          _n.CIR_VERIFY_NONBLOCK if nonblocking else 0))

    VERIFY_STATS_FIELDS = ("bytes_held", "peak_bytes_held", "pending", "outcomes_held",
                           "expired", "forgotten", "refused", "batches")

    def verify_stats(self):
        out = (ctypes.c_uint64 * _n.CIR_VERIFY_STATS_FIELDS)()
        _n.check(_n.lib.cir_verify_stats(self._h, out))
        return dict(zip(self.VERIFY_STATS_FIELDS, list(out)))

    def check_file(self, fd, block_size, expected, hash_type=None):
        ht = (hash_type or HashType.blake2b_256()).code
        if len(expected) % 32:
            raise ValueError("expected digests must be 32 bytes each")
        n = len(expected) // 32
        exp = ctypes.create_string_buffer(bytes(expected), max(len(expected), 1))
        ok = ctypes.c_int()
        _n.check(_n.lib.cir_check_file(self._h, ht, fd, block_size, exp, n, ctypes.byref(ok)))
        return ok.value == 1

    CHECK_STATS_FIELDS = ("files", "blocks", "bytes", "batches", "empty_entries", "peak_fds",
                          "errno", "first_bad_block")

    def check_index(self, root, index, threads=0, dir_fd=None):
        """commit_image's re-hash loop (src/daemon/disk/commit.rs:51-117) over
        the image at `root` (relative to dir_fd when given; root=None: dir_fd
        itself) against `index`, in one call: a CheckResult with the first
        failing entry in index order, or ok."""
        if len(index):
            ptr, keep = _buf(index)
        else:  # (an empty index is a parse error, not a null argument)
            keep = ctypes.create_string_buffer(1)
            ptr = ctypes.cast(keep, ctypes.c_void_p)
        kind = ctypes.c_int()
        path = ctypes.c_void_p()
        plen = ctypes.c_size_t()
        stats = (ctypes.c_uint64 * _n.CIR_CHECK_STATS_FIELDS)()
        if root is None and dir_fd is None:
            raise ValueError("check_index needs a root path or a directory fd")
        fd = -100 if dir_fd is None else dir_fd  # AT_FDCWD
        _n.check(_n.lib.cir_check_index(self._h, fd, None if root is None else os.fsencode(root),
                                        ptr, len(index), threads, ctypes.byref(kind),
                                        ctypes.byref(path), ctypes.byref(plen), stats))
        del keep
        raw = _n.take_buffer(path.value, plen.value) if path.value else None
        return CheckResult(kind.value, raw, dict(zip(self.CHECK_STATS_FIELDS, list(stats))))

    LINKS_STATS_FIELDS = ("ok", "checksum", "read", "blocks", "bytes", "batches", "peak_fds",
                          "empty_candidates")

    def check_links(self, index, roots, links, threads=0):
        """check_and_hardlink's verify (src/daemon/disk/public.rs:285-346) of
        every candidate in one call.  `roots`: the source images' directories
        -- a path, a directory fd (int) or a (dir_fd, path) pair each;
        `links`: (file ordinal, source ordinal) pairs as link_candidates
        returns them.  A LinksResult with one verdict per candidate; nothing
        is linked."""
        return self._check_links(index, roots, links, None, threads, False)

    def check_links_at(self, index, roots, links, paths, threads=0):
        """check_links with a place per candidate (cir_check_links_at):
        candidate i is looked for under its source root at paths[i] (bytes, as
        file_copies returns them; b"": the entry's own path) and must have the
        size, mode bits and digests of file entry links[i][0] of `index`.
        paths=None is check_links.  A path with a `.` or `..` component, or
        made of slashes only, raises CiruelaError (CIR_EINVAL) before any file
        is opened."""
        return self._check_links(index, roots, links, paths, threads, True)

    def _check_links(self, index, roots, links, paths, threads, at):
        if len(index):
            ptr, keep = _buf(index)
        else:  # (an empty index is a parse error, not a null argument)
            keep = ctypes.create_string_buffer(1)
            ptr = ctypes.cast(keep, ctypes.c_void_p)
        links = [(int(f), int(s)) for f, s in links]
        nsrc, n = len(roots), len(links)
        fds = (ctypes.c_int * max(nsrc, 1))()
        dirs = (ctypes.c_char_p * max(nsrc, 1))()
        for j, r in enumerate(roots):
            if isinstance(r, int):
                fds[j], dirs[j] = r, None
            elif isinstance(r, tuple):
                fds[j], dirs[j] = r[0], os.fsencode(r[1])
            else:
                fds[j], dirs[j] = -100, os.fsencode(r)  # AT_FDCWD
        lf = (ctypes.c_uint64 * max(n, 1))(*[f for f, _ in links])
        ls = (ctypes.c_uint32 * max(n, 1))(*[s for _, s in links])
        kinds = (ctypes.c_uint8 * max(n, 1))()
        errnos = (ctypes.c_int32 * max(n, 1))()
        stats = (ctypes.c_uint64 * _n.CIR_LINKS_STATS_FIELDS)()
        if at:
            offs, blob = None, None
            if paths is not None:
                paths = [bytes(p) for p in paths]
                if len(paths) != n:
                    raise ValueError("one path per candidate")
                acc = [0]
                for p in paths:
                    acc.append(acc[-1] + len(p))
                offs = (ctypes.c_uint64 * (n + 1))(*acc)
                blob = ctypes.cast(ctypes.create_string_buffer(b"".join(paths), max(acc[-1], 1)),
                                   ctypes.c_void_p)
            _n.check(_n.lib.cir_check_links_at(self._h, ptr, len(index), fds, dirs, nsrc, lf, ls,
                                               offs, blob, n, threads, kinds, errnos, stats))
        else:
            _n.check(_n.lib.cir_check_links(self._h, ptr, len(index), fds, dirs, nsrc, lf, ls, n,
                                            threads, kinds, errnos, stats))
        del keep
        return LinksResult(index, links, list(kinds)[:n], list(errnos)[:n],
                           dict(zip(self.LINKS_STATS_FIELDS, list(stats))))

    BLOCKS_STATS_FIELDS = ("have", "missing", "complete", "absent", "partial", "blocked", "bytes",
                           "batches", "peak_fds", "unread_blocks")

    def check_blocks(self, root, index, threads=0, dir_fd=None):
        """Which blocks of `index` the partial image at `root` (relative to
        dir_fd when given; root=None: dir_fd itself) already holds: a
        BlocksResult with one bit per block and one state per file.  What
        "Resuming download" (src/daemon/tracking/mod.rs:561-585) would need in
        order not to fetch everything again; nothing is written."""
        if len(index):
            ptr, keep = _buf(index)
        else:  # (an empty index is a parse error, not a null argument)
            keep = ctypes.create_string_buffer(1)
            ptr = ctypes.cast(keep, ctypes.c_void_p)
        if root is None and dir_fd is None:
            raise ValueError("check_blocks needs a root path or a directory fd")
        fd = -100 if dir_fd is None else dir_fd  # AT_FDCWD
        have = ctypes.c_void_p()
        nblk = ctypes.c_uint64()
        state = ctypes.c_void_p()
        errs = ctypes.c_void_p()
        nfiles = ctypes.c_size_t()
        stats = (ctypes.c_uint64 * _n.CIR_BLOCKS_STATS_FIELDS)()
        _n.check(_n.lib.cir_check_blocks(self._h, fd, None if root is None else os.fsencode(root),
                                         ptr, len(index), threads, ctypes.byref(have),
                                         ctypes.byref(nblk), ctypes.byref(state),
                                         ctypes.byref(errs), ctypes.byref(nfiles), stats))
        del keep
        nf = nfiles.value
        bits = _n.take_buffer(have.value, 8 * ((nblk.value + 63) // 64))
        states = _n.take_buffer(state.value, nf)
        raw = _n.take_buffer(errs.value, 4 * nf)
        errnos = list((ctypes.c_int32 * nf).from_buffer_copy(raw)) if nf else []
        return BlocksResult(index, nblk.value, bits, list(states), errnos,
                            dict(zip(self.BLOCKS_STATS_FIELDS, list(stats))))

    LOAD_STATS_FIELDS = BLOCKS_STATS_FIELDS + ("scattered_bytes", "skipped")

    def load_blocks(self, root, index, buffers, threads=0, dir_fd=None, stream=0):
        """check_blocks that keeps what it read (cir_load_blocks): the bytes of
        every block it read stand in the caller's device buffers afterwards,
        and the BlocksResult says which of them are the index's.  buffers: per
        file entry, in index order, None (a non-empty file is then "skipped":
        not opened, not read), a device pointer as int, or a (ptr, nbytes) pair
        or anything with data_ptr() and a byte count (a torch tensor); a span
        shorter than its entry is a ValueError.  The buffers live on the device
        of `stream`, behind whose earlier work the first byte lands; the call
        returns when the buffers are filled."""
        return _load_blocks(self, root, index, buffers, None, threads, dir_fd, stream)

    RELOAD_STATS_FIELDS = LOAD_STATS_FIELDS + ("copied_blocks", "copied_bytes", "resident_blocks",
                                               "resident_files", "dropped_length")

    def reload_blocks(self, root, index, buffers, resident, threads=0, dir_fd=None, stream=0):
        """load_blocks for a process that holds the previous version in device
        memory (cir_reload_blocks).  resident: the previous version's buffers,
        in any order -- (ptr, nbytes) pairs or anything with data_ptr() and a
        byte count, None and empty ones ignored --, on the same device, none of
        them overlapping a destination.  They are hashed where they lie; a
        block of `index` whose digest and length one of their blocks has is
        copied inside device memory, the rest is read from `root` as
        load_blocks reads it.  A file all of whose blocks came from memory is
        not opened: it is "complete" and its `resident` flag is set."""
        return _load_blocks(self, root, index, buffers, list(resident), threads, dir_fd, stream)

    UPDATE_STATS_FIELDS = RELOAD_STATS_FIELDS + ("kept_blocks", "kept_bytes", "staged_blocks",
                                                 "scratch_bytes", "demoted_blocks")

    def update_blocks(self, root, index, buffers, resident, scratch_bytes=None, threads=0,
                      dir_fd=None, stream=0):
        """reload_blocks without the overlap restriction (cir_update_blocks):
        the buffers may be the resident ones themselves, overlap them in any
        way, or be fresh memory.  A block that already stands at its
        destination with the index's digest is kept untouched; a block whose
        destination lies clear of every resident buffer is copied directly;
        any other block found in memory goes through a staging scratch of at
        most scratch_bytes (None: whatever it takes; 0: none, such blocks are
        read from `root`).  Resident buffers must not overlap one another, nor
        may the destinations.  Until the scratch is allocated nothing is
        written, so a CiruelaError(CIR_ENOMEM) leaves the old version whole;
        after that the result's bits are the truth about the buffers."""
        cap = (1 << 64) - 1 if scratch_bytes is None else int(scratch_bytes)
        if not 0 <= cap < 1 << 64:
            raise ValueError("scratch_bytes must fit 64 bits")
        return _load_blocks(self, root, index, buffers, list(resident), threads, dir_fd, stream,
                            scratch=cap)

    STORE_STATS_FIELDS = ("blocks", "files", "dirs_made", "bytes", "batches", "body_bytes")

    def store_blocks(self, root, files, block_size, hash_type, threads=0, dir_fd=None, stream=0,
                     image_id=None, stats=None):
        """load_blocks mirrored (cir_store_blocks): files held in device
        memory written out below the existing directory `root` (relative to
        dir_fd when given; root=None: dir_fd itself), and the tree's index.
        files = [(path, obj[, exe])] as index_memory takes them, on the device
        of `stream`, behind whose earlier work the first byte is read.
        Directories are made as needed; a file that exists, a symlink at any
        component or a write error raises CiruelaError (CIR_EIO) and leaves
        what was written.  Returns the index bytes: index_memory's of the same
        list and v1.scan's of the written tree.  image_id: a list that receives
        the ImageId; stats: a dict that receives STORE_STATS_FIELDS."""
        if root is None and dir_fd is None:
            raise ValueError("store_blocks needs a root path or a directory fd")
        fd = -100 if dir_fd is None else dir_fd  # AT_FDCWD
        paths, offs, exe, objs = _emit_files(files)
        spans = [_device_span(o) for o in objs]
        n = len(spans)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[p or None for p, _ in spans])
        out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
        iid = ctypes.create_string_buffer(32)
        st = (ctypes.c_uint64 * _n.CIR_STORE_STATS_FIELDS)()
        _n.check(_n.lib.cir_store_blocks(self._h, fd, None if root is None else os.fsencode(root),
                                         hash_type.code, block_size, paths, offs,
                                         _sizes([b for _, b in spans]), exe, n, ptrs, stream,
                                         threads, ctypes.byref(out), ctypes.byref(out_len), iid,
                                         st))
        del objs
        if image_id is not None:
            image_id.append(ImageId(iid.raw))
        if stats is not None:
            stats.update(zip(self.STORE_STATS_FIELDS, list(st)))
        return _n.take_buffer(out.value, out_len.value)

    def scan(self, config):
        dirs = [os.fsencode(d) for d, _ in config._dirs]
        pres = [p.encode() for _, p in config._dirs]
        cd = (ctypes.c_char_p * len(dirs))(*dirs)
        cp = (ctypes.c_char_p * len(pres))(*pres)
        out = ctypes.c_void_p()
        ln = ctypes.c_size_t()
        _n.check(_n.lib.cir_scan_v1(self._h, cd, cp, len(dirs), config._block_size,
                                    config._hash.code, config._threads, ctypes.byref(out),
                                    ctypes.byref(ln)))
        return _n.take_buffer(out.value, ln.value)

    def scan_into(self, config, out):
        """cir_scan_v1_write: append the index to `out` (a bytearray) while
        the scan emits it -- header, then each stretch of the body as files
        complete, the footer line last -- as v1::scan writes into the
        caller's Vec (src/client/sync/uploads.rs:55-57).  Returns the number
        of bytes appended.  An exception raised while appending stops the
        scan and is re-raised here."""
        dirs = [os.fsencode(d) for d, _ in config._dirs]
        pres = [p.encode() for _, p in config._dirs]
        cd = (ctypes.c_char_p * len(dirs))(*dirs)
        cp = (ctypes.c_char_p * len(pres))(*pres)
        failed = []

        def write(_user, data, n):
            try:
                out.extend((ctypes.c_char * n).from_address(data))
                return 0
            except BaseException as e:  # noqa: BLE001 - re-raised after the call
                failed.append(e)
                return 1
        cb = _n.WRITE_FN(write)
        ln = ctypes.c_size_t()
        rc = _n.lib.cir_scan_v1_write(self._h, cd, cp, len(dirs), config._block_size,
                                      config._hash.code, config._threads, cb, None,
                                      ctypes.byref(ln))
        if failed:
            raise failed[0]
        _n.check(rc)
        return ln.value

    # ---- footer placement and scan timing (diagnostics) -------------------
    FOOTER_HOST, FOOTER_GPU = 0, 1
    SCAN_BATCH_FIELDS = ("device", "bytes", "blocks", "wait_ms", "read_start_ms", "read_end_ms",
                         "h2d_start_ms", "h2d_end_ms", "hash_start_ms", "done_ms")
    SCAN_PHASE_FIELDS = ("walk_ms", "hash_loop_ms", "last_emit_ms", "footer_tail_ms",
                         "output_ms", "footer_busy_ms", "footer_mode", "batches", "index_bytes",
                         "footer_feeds")

    def set_footer_mode(self, mode):
        """Where cir_scan_v1 and cir_index_rewrite hash an index's footer, in
        either hash type: FOOTER_HOST (a host thread, the default) or
        FOOTER_GPU (blake2b/256: the chain kernel beside the scan;
        sha512/256: one lane at the end)."""
        _n.check(_n.lib.cir_set_footer_mode(self._h, mode))

    def scan_timing(self, enable=True):
        _n.check(_n.lib.cir_debug_scan_timing(self._h, 1 if enable else 0))

    def scan_batches(self):
        """One dict per staged batch of the scans since scan_timing(True)."""
        n = ctypes.c_size_t()
        _n.check(_n.lib.cir_debug_scan_batches(self._h, None, 0, ctypes.byref(n)))
        k = len(self.SCAN_BATCH_FIELDS)
        rows = (ctypes.c_double * (k * max(1, n.value)))()
        _n.check(_n.lib.cir_debug_scan_batches(self._h, rows, n.value, ctypes.byref(n)))
        return [dict(zip(self.SCAN_BATCH_FIELDS, rows[i * k:(i + 1) * k]))
                for i in range(n.value)]

    def scan_phases(self):
        """The phase record of the last scan since scan_timing(True)."""
        out = (ctypes.c_double * len(self.SCAN_PHASE_FIELDS))()
        _n.check(_n.lib.cir_debug_scan_phases(self._h, out))
        return dict(zip(self.SCAN_PHASE_FIELDS, list(out)))

    def index_rewrite(self, data):
        ptr, keep = _buf(data)
        out = ctypes.c_void_p()
        ln = ctypes.c_size_t()
        _n.check(_n.lib.cir_index_rewrite(self._h, ptr, len(data), ctypes.byref(out),
                                          ctypes.byref(ln)))
        del keep
        return _n.take_buffer(out.value, ln.value)


class CheckResult:
    """Verdict of check_index: ok, or the first failing entry in index order
    -- kind "checksum" (Error::Checksum) or "read" (Error::ReadFile, with
    errno), path as the index's raw bytes -- and the call's stats."""

    __slots__ = ("kind", "path", "errno", "stats")
    KINDS = {_n.CIR_CHECK_OK: "ok", _n.CIR_CHECK_CHECKSUM: "checksum", _n.CIR_CHECK_READ: "read"}

    def __init__(self, kind, path, stats):
        self.kind = self.KINDS[kind]
        self.path = path
        self.errno = stats["errno"]
        self.stats = stats

    @property
    def ok(self):
        return self.kind == "ok"

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return "CheckResult(%s%s)" % (self.kind, "" if self.ok else ", %r" % (self.path,))


def _unescape(name):
    """An index's \\xNN escapes back to raw bytes."""
    if b"\\" not in name:
        return name
    out = bytearray()
    i = 0
    while i < len(name):
        if name[i:i + 2] == b"\\x" and i + 4 <= len(name):
            out.append(int(name[i + 2:i + 4], 16))
            i += 4
        else:
            out.append(name[i])
            i += 1
    return bytes(out)


def _file_paths(index):
    """The paths (raw bytes) of an index's file entries, in index order."""
    paths = []
    cur = b"/"
    for line in bytes(index).split(b"\n")[1:]:
        if line.startswith(b"/"):
            cur = _unescape(line)
        elif line.startswith(b"  "):
            tok = line[2:].split(b" ")
            if len(tok) >= 2 and tok[1] in (b"f", b"x"):
                paths.append((b"" if cur == b"/" else cur) + b"/" + _unescape(tok[0]))
    return paths


class LinksResult:
    """Verdicts of check_links, one per candidate in the order given: kinds
    ("ok", "checksum" or "read"), errnos (of a "read", else 0), ok_paths --
    the index paths (raw bytes) of the candidates that passed, which is
    check_and_hardlink's HashSet<PathBuf> (src/daemon/disk/public.rs:285-305)
    -- and the call's stats."""

    __slots__ = ("links", "kinds", "errnos", "ok_paths", "stats")

    def __init__(self, index, links, kinds, errnos, stats):
        paths = _file_paths(index)
        self.links = links
        self.kinds = [CheckResult.KINDS[k] for k in kinds]
        self.errnos = errnos
        self.ok_paths = {paths[f] for (f, _), k in zip(links, kinds) if k == _n.CIR_CHECK_OK}
        self.stats = stats

    def __repr__(self):
        return "LinksResult(%d ok, %d checksum, %d read)" % (
            self.stats["ok"], self.stats["checksum"], self.stats["read"])


def _file_blocks(index):
    """(path as raw bytes, size, block count) of an index's file entries, in
    index order, and the index's block size."""
    lines = bytes(index).split(b"\n")
    bs = 0
    for tok in lines[0].split(b" "):
        if tok.startswith(b"block_size="):
            bs = int(tok[len(b"block_size="):])
    out = []
    cur = b"/"
    for line in lines[1:]:
        if line.startswith(b"/"):
            cur = _unescape(line)
        elif line.startswith(b"  "):
            tok = line[2:].split(b" ")
            if len(tok) >= 3 and tok[1] in (b"f", b"x"):
                size = int(tok[2])
                out.append(((b"" if cur == b"/" else cur) + b"/" + _unescape(tok[0]), size,
                            (size + bs - 1) // bs if bs else 0))
    return out, bs


class BlocksResult:
    """Verdict of check_blocks.  nblk: the index's blocks, numbered in index
    order over its file entries; have: their bitmap as bytes (bit g & 7 of
    byte g >> 3), has(g) one bit of it.  Per file entry, in index order:
    states ("complete", "absent", "partial" or "blocked"; from load_blocks
    also "skipped": a non-empty file that was given no buffer), long (the file
    is longer than its entry and is to be truncated before commit), resident
    (reload_blocks took every block of the file from device memory and did not
    open it), errnos (of a "blocked", else 0).  complete: every file is complete.  missing(): the
    (path as raw bytes, byte offset) of every block that is not there, in
    index order -- what fill_blocks would queue
    (src/daemon/tracking/progress.rs:136-151)."""

    __slots__ = ("nblk", "have", "states", "long", "resident", "errnos", "stats", "_index")
    STATES = {_n.CIR_FILE_COMPLETE: "complete", _n.CIR_FILE_ABSENT: "absent",
              _n.CIR_FILE_PARTIAL: "partial", _n.CIR_FILE_BLOCKED: "blocked"}
    SKIPPED = "skipped"

    def __init__(self, index, nblk, have, states, errnos, stats):
        self._index = index  # (split into lines only when missing() is asked for)
        self.nblk = nblk
        self.have = bytes(have)  # (little-endian u64 words: byte order is bit order)
        self.states = [self.SKIPPED if s & 0x7f == _n.CIR_FILE_SKIPPED else self.STATES[s & 3]
                       for s in states]
        self.long = [bool(s & _n.CIR_FILE_LONG) for s in states]
        self.resident = [bool(s & _n.CIR_FILE_RESIDENT) for s in states]
        self.errnos = list(errnos)
        self.stats = stats

    def has(self, g):
        if not 0 <= g < self.nblk:
            raise IndexError("block %r of %d" % (g, self.nblk))
        return bool(self.have[g >> 3] >> (g & 7) & 1)

    @property
    def complete(self):
        return all(s == "complete" for s in self.states)

    def __bool__(self):
        return self.complete

    def missing(self):
        files, bs = _file_blocks(self._index)
        out = []
        g = 0
        for path, _, n in files:
            for j in range(n):
                if not self.has(g + j):
                    out.append((path, j * bs))
            g += n
        return out

    def __repr__(self):
        return "BlocksResult(%d of %d blocks; %s)" % (
            self.stats["have"], self.nblk,
            ", ".join("%d %s" % (self.states.count(s), s) for s in self.STATES.values()))


class SourcesResult:
    """Answer of block_sources.  nblk: the index's blocks, numbered in index
    order over its file entries; per block g: src[g] the source ordinal (None
    when no local copy is known or the block was not wanted), file[g] the file
    ordinal inside that source's index, block[g] the block number inside that
    file.  found: how many blocks have a source; bytes_local: their bytes.
    copies(): (dst_path, dst_offset, length, src, src_path, src_offset) per
    found block in index order, paths as raw bytes -- what a caller copies
    instead of what fill_blocks would queue (src/daemon/tracking/progress.rs:
    136-151).  want_after(): the bitmap (as BlocksResult.have is laid out) of
    the wanted blocks that were not found."""

    __slots__ = ("nblk", "src", "file", "block", "stats", "skipped", "_index", "_sources", "_want")
    STATS_FIELDS = ("wanted", "found", "bytes_local", "pool_blocks", "sources_used",
                    "dropped_length", "table_slots", "on_device")

    def __init__(self, index, sources, nblk, src, file, block, stats, skipped=0, want=None):
        self._index = index      # (split into lines only when copies() is asked for)
        self._sources = sources
        self._want = want        # bytes of the want bitmap, or None = every block
        self.nblk = nblk
        self.src = [None if s == 0xFFFFFFFF else s for s in src]
        self.file = [f if s is not None else None for f, s in zip(file, self.src)]
        self.block = [b if s is not None else None for b, s in zip(block, self.src)]
        self.stats = stats
        self.skipped = skipped

    @property
    def found(self):
        return self.stats["found"]

    @property
    def bytes_local(self):
        return self.stats["bytes_local"]

    def copies(self):
        files, bs = _file_blocks(self._index)
        paths = {}
        g = 0
        for path, size, n in files:
            for j in range(n):
                s = self.src[g + j]
                if s is not None:
                    if s not in paths:
                        paths[s] = [p for p, _, _ in _file_blocks(self._sources[s])[0]]
                    yield (path, j * bs, min(bs, size - j * bs), s, paths[s][self.file[g + j]],
                           self.block[g + j] * bs)
            g += n

    def want_after(self):
        out = bytearray(8 * ((self.nblk + 63) // 64))
        for g in range(self.nblk):
            wanted = self._want is None or self._want[g >> 3] >> (g & 7) & 1
            if wanted and self.src[g] is None:
                out[g >> 3] |= 1 << (g & 7)
        return bytes(out)

    def __repr__(self):
        return "SourcesResult(%d of %d wanted blocks found, %d bytes)" % (
            self.stats["found"], self.stats["wanted"], self.stats["bytes_local"])


def _want_bitmap(index, want, skip_files, have):
    """The want bitmap of block_sources as bytes (whole u64 words), or None
    for "every block": `want` (bytes, bit g & 7 of byte g >> 3) minus the
    blocks of the files in skip_files minus the 1-bits of `have`."""
    if want is None and not skip_files and have is None:
        return None
    files, _ = _file_blocks(index)
    nblk = sum(n for _, _, n in files)
    nbytes = 8 * ((nblk + 63) // 64)
    if want is None:
        bits = bytearray(b"\xff" * nbytes)
    else:
        bits = bytearray(bytes(want)[:nbytes].ljust(nbytes, b"\0"))
    if skip_files:
        g = 0
        for f, (_, _, n) in enumerate(files):
            if f in skip_files:
                for k in range(g, g + n):
                    bits[k >> 3] &= ~(1 << (k & 7)) & 0xFF
            g += n
    if have is not None:
        hv = bytes(have.have if isinstance(have, BlocksResult) else have)
        for i, b in enumerate(hv[:nbytes]):
            bits[i] &= ~b & 0xFF
    return bytes(bits)


def block_sources(index, sources, want=None, skip_files=None, have=None, context=None):
    """Which blocks of `index` the older images whose indexes are `sources`
    (best first) already hold, and where: what fill_blocks
    (src/daemon/tracking/progress.rs:129-170) need not queue.  want: a bitmap
    over the index's blocks (bytes, bit g & 7 of byte g >> 3; None = all);
    skip_files: file ordinals whose blocks are not wanted (the hardlinked
    files); have: a BlocksResult or bitmap whose 1-bits are not wanted.  With
    a context the join runs on its first GPU; without one the same rule runs
    on the host (no default context is opened).  Returns a SourcesResult; no
    file is read and nothing is copied."""
    if len(index):
        ptr, keep = _buf(index)
    else:  # (an empty index is a parse error, not a null argument)
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    sources = [bytes(s) for s in sources]
    nsrc = len(sources)
    bufs = [ctypes.create_string_buffer(s, max(len(s), 1)) for s in sources]
    sp = (ctypes.c_void_p * max(nsrc, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * max(nsrc, 1))(*[len(s) for s in sources])
    wbits = _want_bitmap(index, want, skip_files, have)
    wbuf = None
    if wbits is not None:
        wbuf = (ctypes.c_uint64 * max(len(wbits) // 8, 1)).from_buffer_copy(
            wbits.ljust(8, b"\0"))
    so, fo, bo = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    nblk = ctypes.c_uint64()
    skipped = ctypes.c_size_t()
    stats = (ctypes.c_uint64 * _n.CIR_SOURCES_STATS_FIELDS)()
    _n.check(_n.lib.cir_block_sources(context.handle if context is not None else None, ptr,
                                      len(index), sp, sl, nsrc, wbuf, ctypes.byref(so),
                                      ctypes.byref(fo), ctypes.byref(bo), ctypes.byref(nblk),
                                      ctypes.byref(skipped), stats))
    del keep
    n = nblk.value
    raw_s = _n.take_buffer(so.value, 4 * n)
    raw_f = _n.take_buffer(fo.value, 8 * n)
    raw_b = _n.take_buffer(bo.value, 8 * n)
    src = list((ctypes.c_uint32 * n).from_buffer_copy(raw_s)) if n else []
    file = list((ctypes.c_uint64 * n).from_buffer_copy(raw_f)) if n else []
    block = list((ctypes.c_uint64 * n).from_buffer_copy(raw_b)) if n else []
    return SourcesResult(index, sources, n, src, file, block,
                         dict(zip(SourcesResult.STATS_FIELDS, list(stats))), skipped.value, wbits)


Extent = collections.namedtuple(
    "Extent", "first count need_file need_block src src_file src_block bytes")


class ExtentsResult:
    """Answer of block_extents.  nblk: the index's blocks; extents: Extent
    tuples in ascending `first` -- `count` consecutive blocks of file
    need_file from block need_block on, whose copies are the consecutive
    blocks of file src_file of source src from src_block on, `bytes` long in
    all; fetch: the bitmap of the wanted blocks without a local copy (bytes,
    laid out as BlocksResult.have: a valid `want` for a later call).
    copies(): (dst_path, dst_offset, length, src, src_path, src_offset) per
    extent, paths as raw bytes -- one copy_file_range each."""

    __slots__ = ("nblk", "extents", "fetch", "stats", "skipped", "_index", "_sources")
    STATS_FIELDS = SourcesResult.STATS_FIELDS + ("extents", "left_to_fetch")

    def __init__(self, index, sources, nblk, extents, fetch, stats, skipped=0):
        self._index = index      # (split into lines only when copies() is asked for)
        self._sources = sources
        self.nblk = nblk
        self.extents = extents
        self.fetch = fetch
        self.stats = stats
        self.skipped = skipped

    @property
    def found(self):
        return self.stats["found"]

    @property
    def bytes_local(self):
        return self.stats["bytes_local"]

    def copies(self):
        files, bs = _file_blocks(self._index)
        paths = {}
        for e in self.extents:
            if e.src not in paths:
                paths[e.src] = [p for p, _, _ in _file_blocks(self._sources[e.src])[0]]
            yield (files[e.need_file][0], e.need_block * bs, e.bytes, e.src,
                   paths[e.src][e.src_file], e.src_block * bs)

    def __repr__(self):
        return "ExtentsResult(%d extents, %d of %d wanted blocks found, %d bytes)" % (
            len(self.extents), self.stats["found"], self.stats["wanted"],
            self.stats["bytes_local"])


def block_extents(index, sources, want=None, skip_files=None, have=None, context=None):
    """block_sources' question answered as extents: the local copies of
    `index`'s blocks in the older images whose indexes are `sources` (best
    first), merged into maximal stretches that one copy_file_range each can
    copy, and the bitmap of what is left to fetch.  The arguments are
    block_sources'.  With a context the mapping and the merge run on its first
    GPU behind the join and only the extents and the bitmap come back; without
    one the same rule runs on the host (no default context is opened).
    Returns an ExtentsResult; no file is read and nothing is copied."""
    if len(index):
        ptr, keep = _buf(index)
    else:  # (an empty index is a parse error, not a null argument)
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    sources = [bytes(s) for s in sources]
    nsrc = len(sources)
    bufs = [ctypes.create_string_buffer(s, max(len(s), 1)) for s in sources]
    sp = (ctypes.c_void_p * max(nsrc, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * max(nsrc, 1))(*[len(s) for s in sources])
    wbits = _want_bitmap(index, want, skip_files, have)
    wbuf = None
    if wbits is not None:
        wbuf = (ctypes.c_uint64 * max(len(wbits) // 8, 1)).from_buffer_copy(
            wbits.ljust(8, b"\0"))
    eo, fo = ctypes.c_void_p(), ctypes.c_void_p()
    next_, nblk = ctypes.c_size_t(), ctypes.c_uint64()
    skipped = ctypes.c_size_t()
    stats = (ctypes.c_uint64 * _n.CIR_EXTENTS_STATS_FIELDS)()
    _n.check(_n.lib.cir_block_extents(context.handle if context is not None else None, ptr,
                                      len(index), sp, sl, nsrc, wbuf, ctypes.byref(eo),
                                      ctypes.byref(next_), ctypes.byref(fo), ctypes.byref(nblk),
                                      ctypes.byref(skipped), stats))
    del keep
    k = next_.value
    raw_e = _n.take_buffer(eo.value, 8 * _n.CIR_EXTENT_WORDS * k)
    fetch = bytes(_n.take_buffer(fo.value, 8 * ((nblk.value + 63) // 64)))
    words = (ctypes.c_uint64 * (_n.CIR_EXTENT_WORDS * k)).from_buffer_copy(raw_e) if k else []
    extents = [Extent(*words[8 * i:8 * i + 8]) for i in range(k)]
    return ExtentsResult(index, sources, nblk.value, extents, fetch,
                         dict(zip(ExtentsResult.STATS_FIELDS, list(stats))), skipped.value)


class RepeatsResult:
    """Answer of block_repeats.  nblk: the index's blocks; extents: Extent
    tuples in ascending `first`, as block_extents', with both files in the
    same index: src is the source's class, 0 = present (copy at once), 1 =
    fetched (copy after the fetch); fetch: the bitmap of the wanted blocks
    that are not repeats (bytes, laid out as BlocksResult.have: a valid `want`
    for any sibling call).  copies(): (dst_path, dst_offset, length,
    src_class, src_path, src_offset) per extent, paths as raw bytes -- one
    copy_file_range each."""

    __slots__ = ("nblk", "extents", "fetch", "stats", "_index")
    STATS_FIELDS = ("wanted", "repeats", "bytes_repeated", "took_part", "present",
                    "dropped_length", "table_slots", "on_device", "extents", "left_to_fetch")

    def __init__(self, index, nblk, extents, fetch, stats):
        self._index = index      # (split into lines only when copies() is asked for)
        self.nblk = nblk
        self.extents = extents
        self.fetch = fetch
        self.stats = stats

    @property
    def repeats(self):
        return self.stats["repeats"]

    @property
    def bytes_repeated(self):
        return self.stats["bytes_repeated"]

    def copies(self):
        files, bs = _file_blocks(self._index)
        for e in self.extents:
            yield (files[e.need_file][0], e.need_block * bs, e.bytes, e.src,
                   files[e.src_file][0], e.src_block * bs)

    def __repr__(self):
        return "RepeatsResult(%d extents, %d of %d wanted blocks repeat, %d bytes)" % (
            len(self.extents), self.stats["repeats"], self.stats["wanted"],
            self.stats["bytes_repeated"])


def _bitmap_words(bits, nwords):
    """A bitmap given as bytes as the nwords u64 words the library reads (None
    stays None); a short one is padded with zeros."""
    if bits is None:
        return None
    nbytes = 8 * max(nwords, 1)
    return (ctypes.c_uint64 * (nbytes // 8)).from_buffer_copy(
        bytes(bits)[:nbytes].ljust(nbytes, b"\0"))


def block_repeats(index, want=None, present=None, context=None):
    """Which blocks of `index` need not be fetched because the same image
    holds, or will fetch, a block with the same digest (a vendored directory,
    one file under two paths, a zero-filled file).  want: the bitmap of the
    blocks still to be obtained (bytes, bit g & 7 of byte g >> 3, whole u64
    words; None = all), for example block_extents' fetch; present: the bitmap
    of the blocks that are in the new directory or will be before any copy is
    made (None = none; a bit in both means wanted).  With a context the parse,
    the join and the merge run on its first GPU; without one the same rule
    runs on the host (no default context is opened).  Returns a RepeatsResult;
    no file is read and nothing is copied."""
    if len(index):
        ptr, keep = _buf(index)
    else:  # (an empty index is a parse error, not a null argument)
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    nwords = 0
    if want is not None or present is not None:
        try:
            files, bs = _file_blocks(index)
            bs = bs or DEFAULT_BLOCK_SIZE
            nwords = (sum((size + bs - 1) // bs for _, size, _ in files) + 63) // 64
        except (ValueError, IndexError):
            pass  # (not an index: the library says so before it reads a bitmap)
    wbuf, pbuf = _bitmap_words(want, nwords), _bitmap_words(present, nwords)
    eo, fo = ctypes.c_void_p(), ctypes.c_void_p()
    next_, nblk = ctypes.c_size_t(), ctypes.c_uint64()
    stats = (ctypes.c_uint64 * _n.CIR_REPEATS_STATS_FIELDS)()
    _n.check(_n.lib.cir_block_repeats(context.handle if context is not None else None, ptr,
                                      len(index), wbuf, pbuf, ctypes.byref(eo),
                                      ctypes.byref(next_), ctypes.byref(fo), ctypes.byref(nblk),
                                      stats))
    del keep
    k = next_.value
    raw_e = _n.take_buffer(eo.value, 8 * _n.CIR_EXTENT_WORDS * k)
    fetch = bytes(_n.take_buffer(fo.value, 8 * ((nblk.value + 63) // 64)))
    words = (ctypes.c_uint64 * (_n.CIR_EXTENT_WORDS * k)).from_buffer_copy(raw_e) if k else []
    extents = [Extent(*words[8 * i:8 * i + 8]) for i in range(k)]
    return RepeatsResult(index, nblk.value, extents, fetch,
                         dict(zip(RepeatsResult.STATS_FIELDS, list(stats))))


class IndexDigests:
    """Answer of index_digests.  hash_type: a CIR_HASH_* code; block_size;
    digests: numpy u8 (nblk, 32), the file entries' block digests in index
    order (the global block numbering of check_blocks); runs: numpy u64
    (nruns, 4), per non-empty file {first block, size, file ordinal, offset of
    the first hash token's leading space in the text}; nfiles: the file
    entries; stats: on_device, fell_back, declined_at (None when no line was
    reported), uploaded_bytes."""

    STATS_FIELDS = ("on_device", "fell_back", "declined_at", "uploaded_bytes")

    def __init__(self, hash_type, block_size, digests, runs, nfiles, stats):
        self.hash_type = hash_type
        self.block_size = block_size
        self.digests = digests
        self.runs = runs
        self.nfiles = nfiles
        self.stats = stats

    @property
    def nblk(self):
        return len(self.digests)

    def __repr__(self):
        return "IndexDigests(%d blocks of %d files, block_size %d)" % (
            self.nblk, self.nfiles, self.block_size)


def index_digests(index, ctx=None):
    """An index's block digests as an array: the text parsed into a flat
    digest list and a run record per non-empty file.  With a context the text
    is uploaded and parsed by the gfx950 kernels on its first GPU
    (cir_index_digests_dev; a text outside the canonical form the device
    takes goes through the host parser instead); without one the host parser
    alone runs and no GPU is needed.  Both give identical arrays and raise the
    same errors.  Returns an IndexDigests."""
    import numpy as np
    if len(index):
        ptr, keep = _buf(index)
    else:  # (an empty index is a parse error, not a null argument)
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    ht = ctypes.c_int()
    bs, nblk = ctypes.c_uint64(), ctypes.c_uint64()
    dg, rn = ctypes.c_void_p(), ctypes.c_void_p()
    nruns, nfiles = ctypes.c_size_t(), ctypes.c_size_t()
    stats = (ctypes.c_uint64 * _n.CIR_INDEX_STATS_FIELDS)()
    _n.check(_n.lib.cir_index_digests(ctx.handle if ctx is not None else None, ptr, len(index),
                                      ctypes.byref(ht), ctypes.byref(bs), ctypes.byref(dg),
                                      ctypes.byref(nblk), ctypes.byref(rn), ctypes.byref(nruns),
                                      ctypes.byref(nfiles), stats))
    del keep
    digests = np.frombuffer(_n.take_buffer(dg.value, 32 * nblk.value), dtype=np.uint8)
    runs = np.frombuffer(_n.take_buffer(rn.value, 32 * nruns.value), dtype=np.uint64)
    st = dict(zip(IndexDigests.STATS_FIELDS, list(stats)))
    if st["declined_at"] == (1 << 64) - 1:
        st["declined_at"] = None
    return IndexDigests(ht.value, bs.value, digests.reshape(-1, 32), runs.reshape(-1, 4),
                        nfiles.value, st)


SKETCH_STATS_FIELDS = ("on_device", "why_host", "blocks", "keys", "uploaded", "downloaded")


def index_sketch(index, context=None, k=_n.CIR_SKETCH_DEFAULT_K, stats=None):
    """The content sketch of an index (cir_index_sketch): the k smallest
    distinct 64-bit keys of its block digests in a blob of 40 + 8 count bytes,
    to keep beside the index and hand to sketch_rank.  With a context the text
    is parsed and sketched on its first GPU and only the keys come down;
    without one (or for a text or a sketch the device declines) the host rule
    answers and no GPU is needed.  Both give identical bytes and raise the
    same errors as index_digests.  stats: a dict that receives the call's
    SKETCH_STATS_FIELDS."""
    if len(index):
        ptr, keep = _buf(index)
    else:  # (an empty index is a parse error, not a null argument)
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    blob, blob_len = ctypes.c_void_p(), ctypes.c_size_t()
    st = (ctypes.c_uint64 * _n.CIR_SKETCH_STATS_FIELDS)()
    _n.check(_n.lib.cir_index_sketch(context.handle if context is not None else None, ptr,
                                     len(index), k, ctypes.byref(blob), ctypes.byref(blob_len),
                                     st))
    del keep
    if stats is not None:
        stats.update(zip(SKETCH_STATS_FIELDS, list(st)))
    return _n.take_buffer(blob.value, blob_len.value)


def sketch_key(digest):
    """The sketch key of one 32-byte digest (cir_sketch_key)."""
    digest = bytes(digest)
    if len(digest) != 32:
        raise ValueError("a digest is 32 bytes")
    return _n.lib.cir_sketch_key(digest)


def sketch_rank(need, sources, skipped=None):
    """Ranks source sketches against the sketch of a new image
    (cir_sketch_rank): [(ordinal, shared, examined)], best first by shared /
    examined, ties in the caller's order.  A source that is None, not a valid
    sketch or of another hash type or block size is left out (skipped: a list
    that receives their count).  Host-only, no GPU."""
    need = bytes(need)
    nsrc = len(sources)
    bufs = [None if s is None else ctypes.create_string_buffer(bytes(s), max(len(s), 1))
            for s in sources]
    n = max(nsrc, 1)
    sp = (ctypes.c_void_p * n)(*[None if b is None else ctypes.cast(b, ctypes.c_void_p)
                                 for b in bufs])
    sl = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in sources])
    order, shared, examined = ((ctypes.c_uint64 * n)() for _ in range(3))
    nranked, nskipped = ctypes.c_size_t(), ctypes.c_size_t()
    _n.check(_n.lib.cir_sketch_rank(ctypes.create_string_buffer(need, max(len(need), 1)),
                                    len(need), sp, sl, nsrc, order, shared, examined,
                                    ctypes.byref(nranked), ctypes.byref(nskipped)))
    if skipped is not None:
        skipped.append(nskipped.value)
    return [(order[i], shared[i], examined[i]) for i in range(nranked.value)]


MEMINDEX_STATS_FIELDS = ("blocks", "device_emit", "files", "body_bytes", "uploaded", "downloaded")


def _emit_files(files):
    """The parallel arrays of a file list [(path, x[, exe])]: (paths buffer,
    path_off, sizes or None, exe, the x column)."""
    paths, offs, exe, col = [], [0], [], []
    for f in files:
        path = os.fsencode(f[0]) if isinstance(f[0], str) else bytes(f[0])
        paths.append(path)
        offs.append(offs[-1] + len(path))
        col.append(f[1])
        exe.append(1 if len(f) > 2 and f[2] else 0)
    n = len(files)
    blob = b"".join(paths)
    return (ctypes.create_string_buffer(blob, max(len(blob), 1)), (ctypes.c_uint64 * (n + 1))(*offs),
            ctypes.create_string_buffer(bytes(exe), max(n, 1)), col)


def _sizes(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*values)


def index_emit_layout(files, block_size=DEFAULT_BLOCK_SIZE):
    """The layout of a file list [(path, size[, exe])]
    (cir_index_emit_layout): (pieces: numpy u64 (npieces, 5) {out_off, lit_off,
    lit_len, first_block, nblk} in emission order, lits: bytes, first_block:
    numpy u64 per file in the caller's order, nblocks, body_len).  What
    Context.index_emit_dev takes once uploaded.  Host-only, no GPU."""
    import numpy as np
    paths, offs, exe, sizes = _emit_files(files)
    n = len(files)
    pp, lp = ctypes.c_void_p(), ctypes.c_void_p()
    npieces, nlits = ctypes.c_size_t(), ctypes.c_size_t()
    first = (ctypes.c_uint64 * max(n, 1))()
    nblk, body = ctypes.c_uint64(), ctypes.c_uint64()
    _n.check(_n.lib.cir_index_emit_layout(block_size, paths, offs, _sizes(sizes), exe, n,
                                          ctypes.byref(pp), ctypes.byref(npieces),
                                          ctypes.byref(lp), ctypes.byref(nlits), first,
                                          ctypes.byref(nblk), ctypes.byref(body)))
    pieces = np.frombuffer(_n.take_buffer(pp.value, 8 * _n.CIR_EMIT_PIECE_WORDS * npieces.value),
                           dtype=np.uint64).reshape(-1, _n.CIR_EMIT_PIECE_WORDS)
    lits = _n.take_buffer(lp.value, nlits.value)
    return pieces, lits, np.array(first[:n], dtype=np.uint64), nblk.value, body.value


def index_emit_tables(pieces, lits, digests, body_len):
    """The body of an index from its tables on the host
    (cir_index_emit_tables): pieces as index_emit_layout gives them (any
    buffer of 5 u64 per piece), lits and digests bytes-like.  Returns (the
    body_len rounded up to 16 bytes, padding included, the count of pieces
    whose ranges lie outside the arrays).  Host-only, no GPU."""
    pieces, lits, digests = bytes(pieces), bytes(lits), bytes(digests)
    if len(pieces) % (8 * _n.CIR_EMIT_PIECE_WORDS) or len(digests) % 32:
        raise ValueError("pieces are 40 bytes each, digests 32")
    cap = (body_len + 15) // 16 * 16
    body = ctypes.create_string_buffer(max(cap, 1))
    res = (ctypes.c_uint64 * _n.CIR_EMIT_RES_FIELDS)()
    _n.check(_n.lib.cir_index_emit_tables(
        ctypes.create_string_buffer(digests, max(len(digests), 1)), len(digests) // 32,
        ctypes.create_string_buffer(pieces, max(len(pieces), 1)),
        len(pieces) // (8 * _n.CIR_EMIT_PIECE_WORDS),
        ctypes.create_string_buffer(lits, max(len(lits), 1)), len(lits), body, body_len, res))
    return body.raw[:cap], res[0]


def index_emit(files, digests, block_size=DEFAULT_BLOCK_SIZE, hash_type=None, image_id=None):
    """The index of a flat list of regular files from host digests
    (cir_index_emit): files = [(path, size[, exe])] in any order, path bytes or
    str, absolute; digests = one bytes-like of 32 bytes per block, file i's
    behind file i-1's in the files' order.  The text is what v1.scan gives for
    a directory holding these files.  image_id: a list that receives the
    ImageId.  Host-only, no GPU."""
    ht = (hash_type or HashType.blake2b_256()).code
    digests = bytes(digests)
    if len(digests) % 32:
        raise ValueError("a digest is 32 bytes")
    paths, offs, exe, sizes = _emit_files(files)
    out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
    iid = ctypes.create_string_buffer(32)
    _n.check(_n.lib.cir_index_emit(ht, block_size, paths, offs, _sizes(sizes), exe, len(files),
                                   ctypes.create_string_buffer(digests, max(len(digests), 1)),
                                   len(digests) // 32, ctypes.byref(out), ctypes.byref(out_len),
                                   iid))
    if image_id is not None:
        image_id.append(ImageId(iid.raw))
    return _n.take_buffer(out.value, out_len.value)


def _load_blocks(ctx, root, index, buffers, resident, threads, dir_fd, stream, scratch=None):
    """Context.load_blocks (resident is None), Context.reload_blocks and
    Context.update_blocks (scratch is its cap): the arguments are checked
    before the context is touched."""
    if len(index):
        ptr, keep = _buf(index)
    else:  # (an empty index is a parse error, not a null argument)
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    if root is None and dir_fd is None:
        raise ValueError("load_blocks needs a root path or a directory fd")
    fd = -100 if dir_fd is None else dir_fd  # AT_FDCWD
    buffers = list(buffers)
    ptrs = []
    sizes = None
    for i, b in enumerate(buffers):
        if b is None:
            ptrs.append(None)
        elif isinstance(b, int):
            ptrs.append(b or None)
        else:
            p, nbytes = _device_span(b)
            if sizes is None:
                sizes = [size for _, size, _ in _file_blocks(index)[0]]
            if i < len(sizes) and nbytes < sizes[i]:
                raise ValueError("buffer %d holds %d bytes, its entry %d" % (i, nbytes, sizes[i]))
            ptrs.append(p or None)
    n = len(ptrs)
    d_data = (ctypes.c_void_p * max(n, 1))(*ptrs)
    have = ctypes.c_void_p()
    nblk = ctypes.c_uint64()
    state = ctypes.c_void_p()
    errs = ctypes.c_void_p()
    nfiles = ctypes.c_size_t()
    outs = (ctypes.byref(have), ctypes.byref(nblk), ctypes.byref(state), ctypes.byref(errs),
            ctypes.byref(nfiles))
    path = None if root is None else os.fsencode(root)
    if resident is None:
        fields = Context.LOAD_STATS_FIELDS
        stats = (ctypes.c_uint64 * _n.CIR_LOAD_STATS_FIELDS)()
        _n.check(_n.lib.cir_load_blocks(ctx._h, fd, path, ptr, len(index), threads, d_data, n,
                                        stream, *outs, stats))
    else:
        spans = [_device_span(r) for r in resident if r is not None]
        d_have = (ctypes.c_void_p * max(len(spans), 1))(*[p or None for p, _ in spans])
        held = (d_have, _sizes([b for _, b in spans]), len(spans))
        if scratch is None:
            fields = Context.RELOAD_STATS_FIELDS
            stats = (ctypes.c_uint64 * _n.CIR_RELOAD_STATS_FIELDS)()
            _n.check(_n.lib.cir_reload_blocks(ctx._h, fd, path, ptr, len(index), threads, d_data,
                                              n, *held, stream, *outs, stats))
        else:
            fields = Context.UPDATE_STATS_FIELDS
            stats = (ctypes.c_uint64 * _n.CIR_UPDATE_STATS_FIELDS)()
            _n.check(_n.lib.cir_update_blocks(ctx._h, fd, path, ptr, len(index), threads, d_data,
                                              n, *held, scratch, stream, *outs, stats))
    del keep, buffers, resident
    nf = nfiles.value
    bits = _n.take_buffer(have.value, 8 * ((nblk.value + 63) // 64))
    states = _n.take_buffer(state.value, nf)
    raw = _n.take_buffer(errs.value, 4 * nf)
    errnos = list((ctypes.c_int32 * nf).from_buffer_copy(raw)) if nf else []
    return BlocksResult(index, nblk.value, bits, list(states), errnos,
                        dict(zip(fields, list(stats))))


def _device_span(obj):
    """(device pointer, bytes) of a (ptr, nbytes) pair or of anything with
    data_ptr() and a byte count (a torch tensor: element_size() x numel(), or
    nbytes); nothing is imported for it."""
    if isinstance(obj, (tuple, list)) and len(obj) == 2:
        return int(obj[0]), int(obj[1])
    if not hasattr(obj, "data_ptr"):
        raise TypeError("expected (ptr, nbytes) or an object with data_ptr(), got %r" % type(obj))
    is_contiguous = getattr(obj, "is_contiguous", None)
    if is_contiguous is not None and not is_contiguous():
        raise ValueError("device data must be contiguous")
    if hasattr(obj, "element_size") and hasattr(obj, "numel"):
        nbytes = obj.element_size() * obj.numel()
    elif hasattr(obj, "nbytes"):
        nbytes = obj.nbytes
    else:
        raise TypeError("%r has data_ptr() but no byte count" % type(obj))
    return int(obj.data_ptr()), int(nbytes)


def index_memory(files, block_size=DEFAULT_BLOCK_SIZE, hash_type=None, context=None, stream=0,
                 image_id=None, stats=None):
    """The index of files held in device memory (cir_index_memory_dev): files
    = [(path, obj[, exe])], obj a (ptr, nbytes) pair or anything with
    data_ptr() and a byte count (a torch tensor), contiguous.  Hashing and the
    text both run on the GPU of `stream`, queued behind whatever that stream
    already holds; only the text comes down.  Returns the index bytes, equal to
    v1.scan of a directory holding the same files.  image_id: a list that
    receives the ImageId; stats: a dict that receives MEMINDEX_STATS_FIELDS."""
    ht = (hash_type or HashType.blake2b_256()).code
    ctx = context or default_context()
    paths, offs, exe, objs = _emit_files(files)
    spans = [_device_span(o) for o in objs]
    n = len(files)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[p or None for p, _ in spans])
    out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
    iid = ctypes.create_string_buffer(32)
    st = (ctypes.c_uint64 * _n.CIR_MEMINDEX_STATS_FIELDS)()
    _n.check(_n.lib.cir_index_memory_dev(ctx.handle, ht, block_size, paths, offs,
                                         _sizes([b for _, b in spans]), exe, n, ptrs, stream,
                                         ctypes.byref(out), ctypes.byref(out_len), iid, st))
    del objs
    if image_id is not None:
        image_id.append(ImageId(iid.raw))
    if stats is not None:
        stats.update(zip(MEMINDEX_STATS_FIELDS, list(st)))
    return _n.take_buffer(out.value, out_len.value)


_default = None
_default_lock = threading.Lock()


def load_image(root, index, context=None, only=None, threads=0):
    """An image directory read into device memory, verified (cir_load_blocks):
    one torch.uint8 tensor per non-empty file entry of `index` -- with `only`
    (paths as raw bytes or str) for those entries alone --, on the context's
    first device, filled from the directory `root`.  Returns ({path as raw
    bytes: tensor}, BlocksResult): a "complete" file's tensor is the file, the
    result's bits say which blocks of the others are the index's."""
    return _load_image(root, index, context, only, threads, None)


def _load_image(root, index, context, only, threads, resident):
    import torch
    ctx = context or default_context()
    dev = torch.device("cuda", ctx.devices()[0])
    files, _ = _file_blocks(index)
    keep = None if only is None else {os.fsencode(p) if isinstance(p, str) else bytes(p)
                                      for p in only}
    tensors = {}
    buffers = []
    for path, size, _ in files:
        if size and (keep is None or path in keep):
            tensors[path] = torch.empty(size, dtype=torch.uint8, device=dev)
            buffers.append(tensors[path])
        else:
            buffers.append(None)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if resident is None:
            res = ctx.load_blocks(root, index, buffers, threads=threads, stream=stream)
        else:
            res = ctx.reload_blocks(root, index, buffers, resident, threads=threads, stream=stream)
    return tensors, res


def reload_image(root, index, resident, context=None, only=None, threads=0):
    """load_image for a process that holds the previous version of the image in
    device memory (cir_reload_blocks): resident is a dict or a list of tensors,
    typically the dict the previous load_image returned.  New tensors are
    allocated and the old ones left alone; what the old ones hold of the new
    image is copied on the device, the rest is read from `root`."""
    held = list(resident.values()) if isinstance(resident, dict) else list(resident)
    return _load_image(root, index, context, only, threads, held)


def update_image(root, index, held, context=None, only=None, threads=0, scratch_bytes=None):
    """reload_image in the tensors that hold the previous version
    (cir_update_blocks): held is the {path: tensor} dict the previous
    load_image (or update_image) returned.  An entry of `index` whose path is
    in held with a tensor of exactly the entry's size gets that same tensor as
    its destination; every other non-empty entry -- with `only`, of those named
    -- gets a new tensor.  All of held is the resident list.  Blocks that
    already stand where they belong are not touched, the others found in held
    are copied on the device (through at most scratch_bytes of staging where
    they land on old bytes; None: whatever it takes), the rest is read from
    `root`.  Returns ({path: tensor}, BlocksResult); held itself is not
    modified, and tensors of paths that vanished are simply not in the result
    -- their bytes may have served as sources, but nothing is written to
    them."""
    import torch
    ctx = context or default_context()
    dev = torch.device("cuda", ctx.devices()[0])
    files, _ = _file_blocks(index)
    keep = None if only is None else {os.fsencode(p) if isinstance(p, str) else bytes(p)
                                      for p in only}
    held = {os.fsencode(p) if isinstance(p, str) else bytes(p): t for p, t in held.items()}
    tensors = {}
    buffers = []
    for path, size, _ in files:
        if size and (keep is None or path in keep):
            old = held.get(path)
            if old is not None and _device_span(old)[1] == size:
                tensors[path] = old
            else:
                tensors[path] = torch.empty(size, dtype=torch.uint8, device=dev)
            buffers.append(tensors[path])
        else:
            buffers.append(None)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        res = ctx.update_blocks(root, index, buffers, list(held.values()),
                                scratch_bytes=scratch_bytes, threads=threads, stream=stream)
    return tensors, res


def store_image(root, files, block_size=DEFAULT_BLOCK_SIZE, hash_type=None, context=None,
                threads=0):
    """load_image mirrored (cir_store_blocks): files = [(path, obj[, exe])] as
    index_memory takes them -- obj a torch tensor or anything with data_ptr()
    and a byte count, or a (ptr, nbytes) pair -- written out below the existing
    directory `root`, on the current torch stream.  Returns the index bytes of
    the written tree: check_index(root, store_image(root, files)) passes, and
    load_image(root, ...) of it gives the files back."""
    import torch
    ctx = context or default_context()
    dev = torch.device("cuda", ctx.devices()[0])
    for f in files:
        if getattr(f[1], "is_cuda", False):
            dev = f[1].device
            break
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        return ctx.store_blocks(root, files, block_size, hash_type or HashType.blake2b_256(),
                                threads=threads, stream=stream)


def default_context():
    """Process-wide context on every visible device (created on first use)."""
    global _default
    with _default_lock:
        if _default is None:
            _default = Context()
        return _default


def _hex(b):
    return b.hex()


class BlockHash:
    """32-byte block id (src/block_id.rs:19); displays as lowercase hex."""

    __slots__ = ("_b",)

    def __init__(self, raw):
        if len(raw) != 32:
            raise ValueError("BlockHash is 32 bytes")
        self._b = bytes(raw)

    @staticmethod
    def from_bytes(raw):
        """Some(BlockHash) for 32 bytes, None otherwise (src/block_id.rs:28-35)."""
        return BlockHash(raw) if len(raw) == 32 else None

    @staticmethod
    def hash_bytes(data):
        """BLAKE2b-256 of data, on the GPU (src/block_id.rs:37-43)."""
        ptr, keep = _buf(bytes(data)) if len(data) else (None, None)
        out = ctypes.create_string_buffer(32)
        _n.check(_n.lib.cir_blake2b256(ptr, len(data), out))
        del keep
        return BlockHash(out.raw)

    def __bytes__(self):
        return self._b

    def __eq__(self, other):
        return isinstance(other, BlockHash) and other._b == self._b

    def __hash__(self):
        return hash(self._b)

    def __str__(self):
        return _hex(self._b)

    def __repr__(self):
        return "BlockHash(%s)" % _hex(self._b)


class ImageId:
    """Image id = the hash on the index's last line (src/id.rs:142-217)."""

    __slots__ = ("_b",)

    def __init__(self, raw):
        self._b = bytes(raw)

    @staticmethod
    def from_str(s):
        try:
            return ImageId(bytes.fromhex(s))
        except ValueError:
            raise ValueError("errors parding hexadecimal image id")

    def __bytes__(self):
        return self._b

    def __eq__(self, other):
        return isinstance(other, ImageId) and other._b == self._b

    def __hash__(self):
        return hash(self._b)

    def __str__(self):
        return _hex(self._b)

    def __repr__(self):
        return "ImageId(%s)" % _hex(self._b)


class HashType:
    """dir_signature::HashType."""

    __slots__ = ("code", "name")

    def __init__(self, code, name):
        self.code = code
        self.name = name

    @staticmethod
    def blake2b_256():
        return HashType(_n.CIR_HASH_BLAKE2B_256, "blake2b/256")

    @staticmethod
    def sha512_256():
        return HashType(_n.CIR_HASH_SHA512_256, "sha512/256")

    def __eq__(self, other):
        return isinstance(other, HashType) and other.code == self.code

    def __repr__(self):
        return "HashType(%s)" % self.name


class Hashes:
    """Per-block hashes of one file (dir_signature::v1::Hashes)."""

    def __init__(self, raw, block_size, hash_type=None):
        self._raw = bytes(raw)
        self._bs = block_size
        self._ht = hash_type or HashType.blake2b_256()

    @staticmethod
    def hash_file(hash_type, block_size, reader, context=None):
        """(size, Hashes) of everything `reader` yields (src/blocks.rs:193).

        reader: an int fd, an object with fileno(), or bytes-like data.
        """
        ctx = context or default_context()
        if isinstance(reader, (bytes, bytearray, memoryview)):
            raw = ctx.hash_memory(reader, block_size, hash_type)
            return len(reader), Hashes(raw, block_size, hash_type)
        fd = reader if isinstance(reader, int) else reader.fileno()
        size, raw = ctx.hash_file(fd, block_size, hash_type)
        return size, Hashes(raw, block_size, hash_type)

    def __len__(self):
        return len(self._raw) // 32

    def get(self, i):
        return self._raw[32 * i:32 * i + 32]

    def __iter__(self):
        return (self.get(i) for i in range(len(self)))

    def block_size(self):
        return self._bs

    def raw(self):
        return self._raw

    def check_file(self, reader, context=None):
        """Hashes::check_file (src/daemon/disk/commit.rs:104): re-hash the file
        on the GPU; True iff it has exactly these blocks."""
        ctx = context or default_context()
        fd = reader if isinstance(reader, int) else reader.fileno()
        return ctx.check_file(fd, self._bs, self._raw, self._ht)


class ScannerConfig:
    """dir_signature::ScannerConfig (used at src/client/sync/uploads.rs:50-54)."""

    def __init__(self):
        self._threads = 4  # GlobalOptions.threads default (src/client/global_options.rs:13)
        self._hash = HashType.blake2b_256()
        self._dirs = []
        self._block_size = DEFAULT_BLOCK_SIZE
        self._progress = False

    @staticmethod
    def new():
        return ScannerConfig()

    def threads(self, n):
        self._threads = int(n)
        return self

    def auto_threads(self):
        self._threads = 0
        return self

    def hash(self, hash_type):
        self._hash = hash_type
        return self

    def block_size(self, n):
        self._block_size = int(n)
        return self

    def add_dir(self, path, prefix="/"):
        self._dirs.append((os.fspath(path), prefix))
        return self

    def print_progress(self):
        self._progress = True
        return self


class v1:  # noqa: N801 - mirrors the `dir_signature::v1` module
    @staticmethod
    def scan(config, out=None, context=None):
        """dir_signature::v1::scan(&cfg, &mut Vec<u8>).

        With `out` (a bytearray), like the reference: the index is appended
        to it as the scan writes it out (cir_scan_v1_write: no whole-index
        copy after the scan) and None is returned.  Without, the index bytes
        are returned (cir_scan_v1)."""
        ctx = context or default_context()
        if out is not None:
            ctx.scan_into(config, out)
            return None
        return ctx.scan(config)


def sha512_256(data):
    """SHA-512/256 of data on the GPU (dir-signature's HashType::sha512_256)."""
    ptr, keep = _buf(bytes(data)) if len(data) else (None, None)
    out = ctypes.create_string_buffer(32)
    _n.check(_n.lib.cir_sha512_256(ptr, len(data), out))
    del keep
    return out.raw


def check_index(root, index, threads=0, dir_fd=None, context=None):
    """Context.check_index on the default context."""
    return (context or default_context()).check_index(root, index, threads, dir_fd)


def check_links(index, roots, links, threads=0, context=None):
    """Context.check_links on the default context."""
    return (context or default_context()).check_links(index, roots, links, threads)


def check_links_at(index, roots, links, paths, threads=0, context=None):
    """Context.check_links_at on the default context."""
    return (context or default_context()).check_links_at(index, roots, links, paths, threads)


def check_blocks(root, index, threads=0, dir_fd=None, context=None):
    """Context.check_blocks on the default context."""
    return (context or default_context()).check_blocks(root, index, threads, dir_fd)


FILE_SOURCES_STATS = ("files", "candidates", "bytes", "pool_files", "sources_used",
                      "table_slots", "on_device", "why_host")


def file_sources(index, sources, context=None):
    """link_candidates matched on the GPU (cir_file_sources): the same rule and
    the same pairs.  With a context the texts are parsed and the files joined
    on its first GPU; whatever the device cannot answer exactly is answered by
    the host rule (stats["why_host"] says why: a CIR_FILE_WHY_* code).  Without
    a context the host rule runs (no default context is opened).  Returns
    ([(file ordinal, source ordinal)], stats dict)."""
    return _candidates(index, sources, context, True)


FILE_COPIES_STATS = FILE_SOURCES_STATS + ("skipped_files", "same_path")


def file_copies(index, sources, context=None, skip=None):
    """Hardlink candidates matched by content (cir_file_copies): for every file
    entry of `index` that is not empty and not in `skip` (an iterable of file
    ordinals, or None), the first of `sources` that holds a file with equal exe
    flag, size and digests at any path, and the first such file inside it.
    With a context the texts are parsed and the files joined on its first GPU;
    whatever the device cannot answer exactly is answered by the host rule
    (stats["why_host"]: a CIR_FILE_WHY_* code).  Without a context the host
    rule runs (no default context is opened).  Returns ([(file ordinal, source
    ordinal, file ordinal inside the source, source path bytes)], stats
    dict)."""
    if len(index):
        ptr, keep = _buf(index)
    else:
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    nsrc = len(sources)
    bufs = [ctypes.create_string_buffer(bytes(s), max(len(s), 1)) for s in sources]
    sp = (ctypes.c_void_p * max(nsrc, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * max(nsrc, 1))(*[len(s) for s in sources])
    bitmap = None
    if skip is not None:
        # (sized for every ordinal the index can hold: its shortest file line is 8 bytes)
        words = [0] * (len(index) // 512 + 1)
        for i in skip:
            if i < 0 or i >= 64 * len(words):
                raise ValueError("no file entry %d in an index of %d bytes" % (i, len(index)))
            words[i >> 6] |= 1 << (i & 63)
        bitmap = (ctypes.c_uint64 * len(words))(*words)
    outs = [ctypes.c_void_p() for _ in range(5)]
    n = ctypes.c_size_t()
    skipped = ctypes.c_size_t()
    stats = (ctypes.c_uint64 * _n.CIR_FILE_COPIES_STATS_FIELDS)()
    _n.check(_n.lib.cir_file_copies(context.handle if context is not None else None, ptr,
                                    len(index), sp, sl, nsrc, bitmap,
                                    *[ctypes.byref(o) for o in outs], ctypes.byref(n),
                                    ctypes.byref(skipped), stats))
    del keep
    found = []
    if n.value:
        k = n.value
        files = list((ctypes.c_uint64 * k).from_address(outs[0].value))
        srcs = list((ctypes.c_uint32 * k).from_address(outs[1].value))
        sfiles = list((ctypes.c_uint64 * k).from_address(outs[2].value))
        offs = list((ctypes.c_uint64 * (k + 1)).from_address(outs[3].value))
        paths = ctypes.string_at(outs[4].value, offs[k])
        for o in outs:
            _n.lib.cir_free(o)
        found = [(files[i], srcs[i], sfiles[i], paths[offs[i]:offs[i + 1]]) for i in range(k)]
    st = dict(zip(FILE_COPIES_STATS, list(stats)))
    st["skipped"] = skipped.value
    return found, st


class PlanResult:
    """Answer of fetch_plan.  links: [(file ordinal, source ordinal)], the
    hardlinks at the same path (file_sources' pairs, minus `deny`); copies:
    [(file ordinal, source ordinal, file ordinal inside the source, source path
    bytes)], the hardlinks by content (file_copies' tuples); extents: Extent
    tuples, the local copies from older images (block_extents'); repeats:
    Extent tuples inside the image (block_repeats': src 0 = present, 1 =
    fetched); fetch: the bitmap of the blocks left to fetch (bytes, laid out as
    BlocksResult.have); nblk: the index's blocks; skipped: sources that took no
    part; stats: the four calls' stats under their own names ("sources",
    "copies", "extents", "repeats") and the plan's own."""

    __slots__ = ("links", "copies", "extents", "repeats", "fetch", "nblk", "stats", "skipped")
    OWN_STATS = ("withdrawn", "linked", "linked_blocks", "have_blocks", "on_device", "why_host")

    def __init__(self, links, copies, extents, repeats, fetch, nblk, stats, skipped):
        self.links = links
        self.copies = copies
        self.extents = extents
        self.repeats = repeats
        self.fetch = fetch
        self.nblk = nblk
        self.stats = stats
        self.skipped = skipped

    def left_to_fetch(self):
        return sum(bin(b).count("1") for b in self.fetch)

    def __repr__(self):
        return "PlanResult(%d links, %d copies, %d extents, %d repeats, %d of %d blocks to fetch)" % (
            len(self.links), len(self.copies), len(self.extents), len(self.repeats),
            self.left_to_fetch(), self.nblk)


def _ordinal_bitmap(ordinals, nwords, what):
    words = [0] * nwords
    for i in ordinals:
        if i < 0 or i >= 64 * nwords:
            raise ValueError("no %s %d in this index" % (what, i))
        words[i >> 6] |= 1 << (i & 63)
    return (ctypes.c_uint64 * nwords)(*words)


def fetch_plan(index, sources, context=None, deny=None, have=None):
    """The whole download plan of a new image in one call (cir_fetch_plan):
    file_sources' links minus `deny` (an iterable of file ordinals for which no
    whole-file link may be proposed, or None), file_copies for the files still
    unlinked, block_extents for the blocks of the files linked by neither,
    minus `have` (the bitmap of the blocks already present and correct, bytes
    laid out as BlocksResult.have, or None), and block_repeats over what is
    still to fetch.  With a context every text is uploaded and parsed once and
    the four joins run back to back on its first GPU; whatever the device
    cannot answer exactly is answered by the same composition on the host
    (stats["why_host"]).  Without a context the host composition runs (no
    default context is opened).  Returns a PlanResult; no file is read and
    nothing is linked or copied."""
    if len(index):
        ptr, keep = _buf(index)
    else:  # (an empty index is a parse error, not a null argument)
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    sources = [bytes(s) for s in sources]
    nsrc = len(sources)
    bufs = [ctypes.create_string_buffer(s, max(len(s), 1)) for s in sources]
    sp = (ctypes.c_void_p * max(nsrc, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * max(nsrc, 1))(*[len(s) for s in sources])
    # (sized for every ordinal the index can hold: its shortest file line is 8
    # bytes, a block's token 65)
    dbuf = None if deny is None else _ordinal_bitmap(deny, len(index) // 512 + 1, "file entry")
    hbuf = _bitmap_words(have, len(index) // (64 * 65) + 1)
    outs = [ctypes.c_void_p() for _ in range(10)]
    nl, nc, ne, nr, nskip = (ctypes.c_size_t() for _ in range(5))
    nblk = ctypes.c_uint64()
    stats = (ctypes.c_uint64 * _n.CIR_PLAN_STATS_FIELDS)()
    ref = ctypes.byref
    _n.check(_n.lib.cir_fetch_plan(context.handle if context is not None else None, ptr,
                                   len(index), sp, sl, nsrc, dbuf, hbuf,
                                   ref(outs[0]), ref(outs[1]), ref(nl),
                                   ref(outs[2]), ref(outs[3]), ref(outs[4]), ref(outs[5]),
                                   ref(outs[6]), ref(nc), ref(outs[7]), ref(ne), ref(outs[8]),
                                   ref(nr), ref(outs[9]), ref(nblk), ref(nskip), stats))
    del keep
    try:
        k = nl.value
        links = []
        if k:
            links = list(zip((ctypes.c_uint64 * k).from_address(outs[0].value),
                             (ctypes.c_uint32 * k).from_address(outs[1].value)))
        k = nc.value
        copies = []
        if k:
            files = list((ctypes.c_uint64 * k).from_address(outs[2].value))
            srcs = list((ctypes.c_uint32 * k).from_address(outs[3].value))
            sfiles = list((ctypes.c_uint64 * k).from_address(outs[4].value))
            offs = list((ctypes.c_uint64 * (k + 1)).from_address(outs[5].value))
            paths = ctypes.string_at(outs[6].value, offs[k])
            copies = [(files[i], srcs[i], sfiles[i], paths[offs[i]:offs[i + 1]])
                      for i in range(k)]
        both = []
        for o, cnt in ((outs[7], ne.value), (outs[8], nr.value)):
            words = (ctypes.c_uint64 * (_n.CIR_EXTENT_WORDS * cnt)).from_address(o.value) \
                if cnt else []
            both.append([Extent(*words[8 * i:8 * i + 8]) for i in range(cnt)])
        nwords = (nblk.value + 63) // 64
        fetch = ctypes.string_at(outs[9].value, 8 * nwords) if nwords and outs[9].value else b""
    finally:
        for o in outs:
            if o.value:
                _n.lib.cir_free(o)
    raw = list(stats)
    st = {
        "sources": dict(zip(FILE_SOURCES_STATS, raw[0:8])),
        "copies": dict(zip(FILE_COPIES_STATS, raw[8:18])),
        "extents": dict(zip(ExtentsResult.STATS_FIELDS, raw[18:28])),
        "repeats": dict(zip(RepeatsResult.STATS_FIELDS, raw[28:38])),
    }
    st.update(zip(PlanResult.OWN_STATS, raw[38:44]))
    return PlanResult(links, copies, both[0], both[1], fetch, nblk.value, st, nskip.value)


def link_candidates(index, sources):
    """scan_links (src/daemon/metadata/hardlink_sources.rs:107-153): for every
    file entry of `index`, the first of `sources` (older images' indexes, best
    first) that lists the same path with equal exe flag, size and digests.
    Returns [(file ordinal, source ordinal)], file ordinals counting the
    index's file entries from 0.  A source that does not parse or has another
    hash type or block size takes no part.  Host only."""
    return _candidates(index, sources, None, False)


def _candidates(index, sources, context, with_stats):
    if len(index):
        ptr, keep = _buf(index)
    else:
        keep = ctypes.create_string_buffer(1)
        ptr = ctypes.cast(keep, ctypes.c_void_p)
    nsrc = len(sources)
    bufs = [ctypes.create_string_buffer(bytes(s), max(len(s), 1)) for s in sources]
    sp = (ctypes.c_void_p * max(nsrc, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * max(nsrc, 1))(*[len(s) for s in sources])
    f = ctypes.c_void_p()
    s = ctypes.c_void_p()
    n = ctypes.c_size_t()
    skipped = ctypes.c_size_t()
    stats = (ctypes.c_uint64 * _n.CIR_FILE_SOURCES_STATS_FIELDS)()
    if with_stats:
        _n.check(_n.lib.cir_file_sources(context.handle if context is not None else None, ptr,
                                         len(index), sp, sl, nsrc, ctypes.byref(f),
                                         ctypes.byref(s), ctypes.byref(n), ctypes.byref(skipped),
                                         stats))
    else:
        _n.check(_n.lib.cir_link_candidates(ptr, len(index), sp, sl, nsrc, ctypes.byref(f),
                                            ctypes.byref(s), ctypes.byref(n),
                                            ctypes.byref(skipped)))
    del keep
    pairs = []
    if n.value:
        files = list((ctypes.c_uint64 * n.value).from_address(f.value))
        srcs = list((ctypes.c_uint32 * n.value).from_address(s.value))
        _n.lib.cir_free(f)
        _n.lib.cir_free(s)
        pairs = list(zip(files, srcs))
    if not with_stats:
        return pairs
    st = dict(zip(FILE_SOURCES_STATS, list(stats)))
    st["skipped"] = skipped.value
    return pairs, st


def get_hash(index):
    """dir_signature::get_hash: the id bytes on the index's last line."""
    ptr, keep = _buf(index) if len(index) else (None, None)
    out = ctypes.create_string_buffer(64)
    n = ctypes.c_size_t()
    _n.check(_n.lib.cir_index_get_hash(ptr, len(index), out, ctypes.byref(n)))
    del keep
    return out.raw[:n.value]


class IndexError_(CiruelaError):  # noqa: N801 - ciruela::index::IndexError
    pass


class DirError(CiruelaError):
    """ciruela::blocks::DirError (src/blocks.rs:114-127)."""


class ReadError(CiruelaError):
    """ReadError of src/index.rs:74-85 / src/blocks.rs:95-111."""


def _raise_as(cls, fn):
    try:
        fn()
    except CiruelaError as e:
        raise cls(e.status, e.detail) from None


class InMemoryIndexes:
    """GetIndex implementation serving indexes from memory (src/index.rs:53)."""

    def __init__(self):
        self._h = _n.lib.cir_indexes_new()

    def __del__(self):
        try:
            _n.lib.cir_indexes_free(self._h)
        except Exception:
            pass

    def register_index(self, data):
        """Returns the ImageId (src/index.rs:98-105); IndexError_ on parse failure."""
        ptr, keep = _buf(bytes(data)) if len(data) else (ctypes.c_void_p(1), None)
        out = ctypes.create_string_buffer(64)
        n = ctypes.c_size_t()
        _raise_as(IndexError_, lambda: _n.check(
            _n.lib.cir_indexes_register(self._h, ptr, len(data), out, ctypes.byref(n))))
        del keep
        return ImageId(out.raw[:n.value])

    def read_index(self, image_id):
        raw = bytes(image_id)
        p = ctypes.c_void_p()
        n = ctypes.c_size_t()
        _raise_as(ReadError, lambda: _n.check(
            _n.lib.cir_indexes_read(self._h, raw, len(raw), ctypes.byref(p), ctypes.byref(n))))
        return _n.take_buffer(p.value, n.value)


class BlockHint:
    """src/blocks.rs:46-48 (currently always empty)."""

    @staticmethod
    def empty():
        return BlockHint()


class ThreadedBlockReader:
    """GetBlock implementation (src/blocks.rs:85-240)."""

    def __init__(self, num_threads=40):
        self._h = _n.lib.cir_blocks_new()
        self._threads = num_threads

    @staticmethod
    def new():
        return ThreadedBlockReader()

    @staticmethod
    def new_num_threads(num):
        return ThreadedBlockReader(num)

    def __del__(self):
        try:
            _n.lib.cir_blocks_free(self._h)
        except Exception:
            pass

    def __len__(self):
        return _n.lib.cir_blocks_len(self._h)

    def register_dir(self, dir, index_data):  # noqa: A002 - reference name
        ptr, keep = _buf(bytes(index_data)) if len(index_data) else (ctypes.c_void_p(1), None)
        _raise_as(DirError, lambda: _n.check(_n.lib.cir_blocks_register_dir(
            self._h, os.fsencode(dir), ptr, len(index_data))))
        del keep

    def register_memory_blocks(self, hash_type, block_size, data, context=None):
        """src/blocks.rs:187-204: block ids are Hashes::hash_file(hash_type, ..)
        digests (put-file passes the index's hash type, put_file/network.rs:56)."""
        ctx = context or default_context()
        ptr, keep = _buf(bytes(data)) if len(data) else (None, None)
        _n.check(_n.lib.cir_blocks_register_memory_ht(ctx.handle, self._h, hash_type.code, ptr,
                                                      len(data), block_size))
        del keep

    def read_block(self, block_hash, hint=None):
        raw = bytes(block_hash)
        if len(raw) != 32:
            raise ValueError("BlockHash is 32 bytes")
        p = ctypes.c_void_p()
        n = ctypes.c_size_t()
        _raise_as(ReadError, lambda: _n.check(
            _n.lib.cir_blocks_read(self._h, raw, ctypes.byref(p), ctypes.byref(n))))
        return _n.take_buffer(p.value, n.value)
