// cir_block_repeats: which blocks of a new image repeat a block of the same
// image, so that they are copied inside it instead of fetched;
// cir_match_repeats_dev, the join behind it on the device.
//
// Reference: fill_blocks (src/daemon/tracking/progress.rs:129-170) queues one
// Block per (path, offset), so a digest that occurs twice inside the new image
// is fetched twice; the reference never looks at this.  The hardlinks
// (cir_check_links), the resume bitmap (cir_check_blocks) and the copies from
// older images (cir_block_extents) leave a bitmap of blocks still to fetch;
// this call takes it as `want`, with the blocks those calls account for as
// `present`, and answers with extents of the same index and a smaller bitmap.
//
// The rule and the host join are repeats.hpp; the kernels of the device join
// are repeats.hip.  The mapping and the merge are cir_block_extents' own
// (extents.hpp, sources.hpp, extents.hip) over the need run table twice, and
// with a context the text is parsed by cir_index_digests_dev's kernels
// (idxscan.hip) through devcall.hpp's parse_one_text, on its DeviceCall, and
// the extents come down through its device_extent_tail; with ctx = NULL they
// are sources::extents_owned's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "devcall.hpp"
#include "dirsig.hpp"
#include "idxscan.hpp"
#include "repeats.hpp"
#include "runtime.hpp"
#include "sources.hpp"

namespace cir {
namespace {

static_assert(repeats::kMaxBlocks == dev::kRepeatMaxBlocks && repeats::kNone == dev::kJoinEmpty &&
                  2 * repeats::kMaxBlocks <= dev::kJoinMaxPool,
              "the host rule, the device join and the extent kernels share their limits");
static_assert(CIR_REPEATS_MAX_BLOCKS == repeats::kMaxBlocks, "the header's limit is the rule's");

int match_repeats_dev_impl(const uint8_t* d_digests, size_t n, const uint64_t* d_want,
                           const uint64_t* d_present, uint32_t* d_table, uint64_t table_slots,
                           uint64_t seed, uint32_t* d_match, uint32_t* d_nmatch, void* stream) {
  auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  if ((n && (!d_digests || !d_match)) || !d_table) return fail(CIR_EINVAL, "null device pointer");
  if (n && (addr(d_digests) & 15u))
    return fail(CIR_EINVAL, "the digest array must be 16-byte aligned");
  if ((addr(d_want) | addr(d_present)) & 7u)
    return fail(CIR_EINVAL, "the bitmaps must be 8-byte aligned");
  if ((addr(d_match) | addr(d_table) | addr(d_nmatch)) & 3u)
    return fail(CIR_EINVAL, "match array, table and count must be 4-byte aligned");
  if ((uint64_t)n > repeats::kMaxBlocks) return fail(CIR_EINVAL, "more than 2^30-1 digests");
  if (table_slots == 0 || (table_slots & (table_slots - 1)) ||
      table_slots < dev::join_table_slots(n))
    return fail(CIR_EINVAL, "table_slots must be a power of two >= cir_match_table_slots(n)");
  CIR_HIP(dev::launch_repeat_join(d_digests, n, d_want, d_present, d_table, table_slots, seed,
                                  d_match, d_nmatch, (hipStream_t)stream));
  return CIR_OK;
}

struct Outs {
  uint64_t** extents_out;
  size_t* nextents_out;
  uint64_t** fetch_out;
  uint64_t* nblk_out;
  uint64_t* stats;
  void clear() const {
    *extents_out = nullptr;
    *nextents_out = 0;
    *fetch_out = nullptr;
    *nblk_out = 0;
    for (int i = 0; i < CIR_REPEATS_STATS_FIELDS; ++i) stats[i] = 0;
  }
};

int too_many_blocks() { return fail(CIR_EINVAL, "more than 2^30-1 blocks in the index"); }

// The host path: repeats::host_match, then sources::map_matches and
// extents_of over the doubled run table.  need.n > 0.
int answer_on_host(const Outs& o, const sources::BlockList& need, const uint8_t* digests,
                   uint64_t bs, const uint64_t* want, const uint64_t* present, bool trace) {
  const uint64_t n = need.n;
  const auto t0 = Clock::now();
  std::vector<uint32_t> match(n), src(n);
  std::vector<uint64_t> file(n), block(n);
  const repeats::Counts c = repeats::host_match(digests, n, want, present, match.data(), draw_seed());
  const auto t1 = Clock::now();
  const sources::BlockList pool = repeats::doubled(need);
  const sources::MapStats ms = sources::map_matches(need, pool, bs, want, match.data(), src.data(),
                                                    file.data(), block.data());
  uint64_t left = 0;
  if (!sources::extents_owned(need, bs, want, src.data(), file.data(), block.data(), o.extents_out,
                              o.nextents_out, o.fetch_out, &left))
    return fail(CIR_ENOMEM, "malloc");
  *o.nblk_out = n;
  o.stats[0] = ms.wanted;
  o.stats[1] = ms.found;
  o.stats[2] = ms.bytes;
  o.stats[3] = c.wanted + c.present;
  o.stats[4] = c.present;
  o.stats[5] = ms.dropped;
  o.stats[8] = *o.nextents_out;
  o.stats[9] = left;
  if (trace)
    fprintf(stderr,
            "cir block_repeats: %llu blocks, %llu take part, host; join %.2f ms, map and merge "
            "%.2f ms; %zu extents\n",
            (unsigned long long)n, (unsigned long long)o.stats[3], ms_between(t0, t1),
            ms_between(t1, Clock::now()), *o.nextents_out);
  return CIR_OK;
}

// The new index parsed on the host into its block list and digests.
int host_parse(const uint8_t* index, size_t len, sources::BlockList* need,
               std::vector<uint8_t>* digests, uint64_t* bs) {
  dirsig::Index idx;
  std::string err;
  if (!dirsig::parse(index, len, &idx, &err)) return parse_fail(idx.bad_hash_size, err);
  sources::append_runs(idx, 0, need);
  *bs = idx.header.block_size;
  if (need->n > repeats::kMaxBlocks) return too_many_blocks();
  digests->resize(32 * need->n);
  sources::copy_digests(idx, digests->data());
  return CIR_OK;
}

// With a context: on its first device, under that device's lock.  The text is
// uploaded once and cir_index_digests_dev's kernels leave the digests and the
// run table in device memory (one digest buffer: the pool is the need list);
// the run table comes back (32 bytes per non-empty file), the doubled table
// and the bitmaps go up, the join and the extent map run, one synchronise
// learns the extent count, the records are emitted and downloaded with the
// fetch bitmap.  The per-block arrays are never made.  framed: dirsig::frame
// took the text and it may be parsed on the device; a text the device
// declines takes the host parser (the lock is not held meanwhile) and its
// digests are uploaded instead.
int repeats_on_device(cir_ctx* ctx, const uint8_t* index, size_t len, bool framed,
                      const dirsig::Header& h, size_t body_off, size_t body_end,
                      const uint64_t* want, const uint64_t* present, const Outs& o, bool trace) {
  // host memory that asynchronous copies read or write: declared before the call
  sources::BlockList need;
  std::vector<uint8_t> h_digests;
  std::vector<uint64_t> h_runs, tabs;
  uint64_t i_res[CIR_INDEX_RES_FIELDS] = {0, 0, 0, 0, 0};
  uint64_t x_res[extents::kResFields] = {0, 0, 0, 0, 0, 0};
  uint64_t bs = h.block_size;
  const auto t0 = Clock::now();
  if (!framed) {
    const int rc = host_parse(index, len, &need, &h_digests, &bs);
    if (rc) return rc;  // (before the context is looked at)
  }
  if (ctx->devs.empty()) return fail(CIR_EINVAL, "context without a device");
  TraceEvents<3> jev, xev;
  DeviceCall c(ctx);
  hipStream_t s = c.s;
  uint8_t* d_dig = nullptr;
  uint64_t* d_runs = nullptr;
  bool dev_parsed = false;
  int rc;
  if ((rc = c.begin())) return rc;
  if (framed) {
    if ((rc = parse_one_text(c, index, len, body_off, body_end, bs, i_res, &d_dig, &d_runs)))
      return rc;
    if (i_res[0] == CIR_INDEX_OK) {
      dev_parsed = true;
      if (i_res[3] > repeats::kMaxBlocks) return too_many_blocks();
      h_runs.resize(4 * i_res[2]);
      if (i_res[2]) {
        CIR_HIP(hipMemcpyAsync(h_runs.data(), d_runs, 32 * i_res[2], hipMemcpyDeviceToHost, s));
        CIR_HIP(hipStreamSynchronize(s));
      }
      for (uint64_t r = 0; r < i_res[2]; ++r)
        need.runs.push_back(
            sources::FileRun{h_runs[4 * r], h_runs[4 * r + 1], h_runs[4 * r + 2], 0});
      need.n = i_res[3];
    } else {
      c.unlock();
      rc = host_parse(index, len, &need, &h_digests, &bs);
      c.lock();
      if (rc) return rc;
    }
  }
  const auto t1 = Clock::now();
  const uint64_t n = need.n, nwords = (n + 63) / 64;
  if (n == 0) {  // (nothing to join, on either side)
    o.stats[7] = 1;
    return CIR_OK;
  }
  if (!dev_parsed) {
    if ((rc = c.alloc(&d_dig, 32 * n))) return rc;
    CIR_HIP(hipMemcpyAsync(d_dig, h_digests.data(), 32 * n, hipMemcpyHostToDevice, s));
  }
  // the need run table twice: its first copy is the need table as well
  const size_t nr = need.runs.size();
  const sources::BlockList pool = repeats::doubled(need);
  tabs.resize(8 * nr);
  sources::pack_runs(pool, tabs.data());
  const uint64_t slots = dev::join_table_slots(n);
  uint64_t* d_tabs = nullptr;
  uint64_t* d_want = nullptr;
  uint64_t* d_present = nullptr;
  uint32_t* d_table = nullptr;
  uint32_t* d_match = nullptr;
  uint64_t* d_work = nullptr;
  uint64_t* d_xres = nullptr;
  uint64_t* d_fetch = nullptr;
  if ((rc = c.alloc(&d_tabs, 64 * nr)) ||
      (want && (rc = c.alloc(&d_want, 8 * nwords))) ||
      (present && (rc = c.alloc(&d_present, 8 * nwords))) ||
      (rc = c.alloc(&d_table, slots * sizeof(uint32_t))) ||
      (rc = c.alloc(&d_match, (n + 4) * sizeof(uint32_t))) ||
      (rc = c.alloc(&d_work, dev::ext_work_bytes(n))) ||
      (rc = c.alloc(&d_xres, sizeof x_res)) || (rc = c.alloc(&d_fetch, 8 * nwords)))
    return rc;
  if (trace && ((rc = jev.create()) || (rc = xev.create()))) return rc;
  CIR_HIP(hipMemcpyAsync(d_tabs, tabs.data(), 64 * nr, hipMemcpyHostToDevice, s));
  if (want) CIR_HIP(hipMemcpyAsync(d_want, want, 8 * nwords, hipMemcpyHostToDevice, s));
  if (present) CIR_HIP(hipMemcpyAsync(d_present, present, 8 * nwords, hipMemcpyHostToDevice, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t2 = Clock::now();
  CIR_HIP(dev::launch_repeat_join(d_dig, n, d_want, d_present, d_table, slots, draw_seed(), d_match,
                                  d_match + n, s, trace ? jev.ev : nullptr));
  const dev::ExtentArgs args{d_match, n, d_tabs, nr, d_tabs, 2 * nr, 2 * n, bs, d_want};
  // (no cap: the count decides the allocation, not the other way round)
  CIR_HIP(dev::launch_extent_map(args, nullptr, nullptr, nullptr, d_fetch, ~0ull, d_work, d_xres, s,
                                 trace ? xev.ev : nullptr));
  CIR_HIP(hipMemcpyAsync(x_res, d_xres, sizeof x_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  const auto t3 = Clock::now();
  const uint64_t count = x_res[5];
  auto t_emit = t3;
  if ((rc = device_extent_tail(c, args, count, d_work, d_xres, d_fetch, false, o.extents_out,
                               o.fetch_out, &t_emit)))
    return rc;
  const repeats::Counts cc = repeats::count_classes(want, present, n);
  *o.nextents_out = count;
  *o.nblk_out = n;
  o.stats[0] = x_res[1];
  o.stats[1] = x_res[2];
  o.stats[2] = x_res[3];
  o.stats[3] = cc.wanted + cc.present;
  o.stats[4] = cc.present;
  o.stats[5] = x_res[4];
  o.stats[6] = slots;
  o.stats[7] = 1;
  o.stats[8] = count;
  o.stats[9] = x_res[1] - x_res[2];
  if (trace) {
    const float build = jev.lap(0), probe = jev.lap(1), map = xev.lap(0), scan = xev.lap(1);
    fprintf(stderr,
            "cir block_repeats: %llu blocks, %llu take part, device (text parsed on the %s); parse "
            "%.2f ms, tables upload %.2f ms (%zu runs twice), build kernel %.3f ms, probe kernel "
            "%.3f ms, map kernel %.3f ms, scan kernel %.3f ms, join to counts %.2f ms, emit and "
            "downloads %.2f ms; %llu extents\n",
            (unsigned long long)n, (unsigned long long)o.stats[3], dev_parsed ? "device" : "host",
            ms_between(t0, t1), ms_between(t1, t2), nr, build, probe, map, scan,
            ms_between(t2, t3), ms_between(t3, Clock::now()), (unsigned long long)count);
  }
  return CIR_OK;
}

int block_repeats_impl(cir_ctx* ctx, const uint8_t* index, size_t len, const uint64_t* want,
                       const uint64_t* present, const Outs& o) {
  if (!index || !o.extents_out || !o.nextents_out || !o.fetch_out || !o.nblk_out || !o.stats)
    return fail(CIR_EINVAL, "null pointer");
  o.clear();
  const bool trace = trace_enabled();
  if (ctx) {
    dirsig::Header h;
    size_t body_off = 0, body_end = 0;
    std::string err;
    // (a frame that does not parse is the host parser's to report)
    const bool framed = !parse_on_host() && device_takes(len) &&
                        dirsig::frame(index, len, &h, &body_off, &body_end, &err);
    const int rc = repeats_on_device(ctx, index, len, framed, h, body_off, body_end, want, present,
                                     o, trace);
    if (rc) o.clear();
    return rc;
  }
  sources::BlockList need;
  std::vector<uint8_t> digests;
  uint64_t bs = 0;
  int rc = host_parse(index, len, &need, &digests, &bs);
  if (rc || need.n == 0) return rc;
  rc = answer_on_host(o, need, digests.data(), bs, want, present, trace);
  if (rc) o.clear();
  return rc;
}

}  // namespace
}  // namespace cir

extern "C" int cir_match_repeats_dev(cir_ctx* ctx, const uint8_t* d_digests, size_t n,
                                     const uint64_t* d_want, const uint64_t* d_present,
                                     uint32_t* d_table, uint64_t table_slots, uint64_t seed,
                                     uint32_t* d_match, uint32_t* d_nmatch, void* stream) try {
  (void)ctx;  // no scratch, no side streams
  return cir::match_repeats_dev_impl(d_digests, n, d_want, d_present, d_table, table_slots, seed,
                                     d_match, d_nmatch, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_block_repeats(cir_ctx* ctx, const uint8_t* index, size_t len,
                                 const uint64_t* want, const uint64_t* present,
                                 uint64_t** extents_out, size_t* nextents_out,
                                 uint64_t** fetch_out, uint64_t* nblk_out,
                                 uint64_t stats[CIR_REPEATS_STATS_FIELDS]) try {
  const cir::Outs o{extents_out, nextents_out, fetch_out, nblk_out, stats};
  return cir::block_repeats_impl(ctx, index, len, want, present, o);
} CIR_CATCH_BOUNDARY
