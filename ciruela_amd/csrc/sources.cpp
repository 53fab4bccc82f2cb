// cir_block_sources: which blocks of a new image older local images already
// hold, and where; cir_match_digests_dev, the join behind it on the device.
//
// Reference: after the hardlinks, fill_blocks (src/daemon/tracking/
// progress.rs:129-170) queues every block of every file that was not
// hardlinked whole, and scan_links (src/daemon/metadata/hardlink_sources.rs:
// 107-153) matches whole files only (:131-133).  So one changed block puts
// every block of its file on the wire -- an appended log, a patched binary, a
// file moved to another path -- although the indexes the daemon already holds
// say where the other blocks sit on the local disk.  That question is a join
// of two digest lists; no file is read here, and the copy stays the caller's.
//
// The rule, the pool builder, the host join and the mapping are sources.hpp
// (no HIP); the device join is join.hip.  With a context the indexes' text is
// parsed on the device as well (idxscan.hip, the rule idxscan.hpp): the need
// list and the pool are decoded straight into the join's buffers and only the
// run tables come back.
//
// cir_block_extents answers the same question merged into extents, with the
// bitmap of what is left to fetch; cir_match_extents_dev is the mapping and
// the merge behind it on the device (extents.hip, the rule extents.hpp), and
// maps cir_block_sources' matches there too.  One flow serves both calls.
//
// The hold on the device, the two-pass parse of the texts (TextSet) and the
// extent tail on the device are devcall.hpp's, shared with repeats.cpp,
// files.cpp and idxscan.cpp; the extent tail on the host and the run tables'
// packing are sources.hpp's.  What is here is the policy: a text the device
// declines goes to the host parser alone, and a bad token found by the decode
// pass means one more attempt with that text on the host.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "devcall.hpp"
#include "dirsig.hpp"
#include "idxscan.hpp"
#include "runtime.hpp"
#include "sources.hpp"

namespace cir {
namespace {

static_assert(sources::kMaxPool == dev::kJoinMaxPool && sources::kNone == dev::kJoinEmpty,
              "the host rule and the device join share their limits");

int match_dev_impl(const uint8_t* d_need, size_t n_need, const uint8_t* d_pool, size_t n_pool,
                   uint32_t* d_table, uint64_t table_slots, uint64_t seed, uint32_t* d_match,
                   uint32_t* d_nmatch, void* stream) {
  if ((n_need && (!d_need || !d_match)) || (n_pool && !d_pool) || !d_table)
    return fail(CIR_EINVAL, "null device pointer");
  if ((n_need && (reinterpret_cast<uintptr_t>(d_need) & 15u)) ||
      (n_pool && (reinterpret_cast<uintptr_t>(d_pool) & 15u)))
    return fail(CIR_EINVAL, "digest arrays must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_match) | reinterpret_cast<uintptr_t>(d_table) |
       reinterpret_cast<uintptr_t>(d_nmatch)) & 3u)
    return fail(CIR_EINVAL, "match array, table and count must be 4-byte aligned");
  if ((uint64_t)n_pool > dev::kJoinMaxPool) return fail(CIR_EINVAL, "more than 2^31-1 pool digests");
  if ((uint64_t)n_need > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 needed digests");
  if (table_slots == 0 || (table_slots & (table_slots - 1)) ||
      table_slots < dev::join_table_slots(n_pool))
    return fail(CIR_EINVAL, "table_slots must be a power of two >= cir_match_table_slots(n_pool)");
  CIR_HIP(dev::launch_join(d_need, n_need, d_pool, n_pool, d_table, table_slots, seed, d_match,
                           d_nmatch, (hipStream_t)stream));
  return CIR_OK;
}

int match_extents_dev_impl(const uint32_t* d_match, uint64_t n_need, const uint64_t* d_need_runs,
                           uint64_t n_need_runs, const uint64_t* d_pool_runs, uint64_t n_pool_runs,
                           uint64_t n_pool, uint64_t bs, const uint64_t* d_want, uint32_t* d_src,
                           uint64_t* d_file, uint64_t* d_block, uint64_t* d_fetch,
                           uint64_t* d_extents, uint64_t cap_extents, void* d_work,
                           uint64_t work_bytes, uint64_t* d_res, void* stream) {
  auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  if ((n_need && !d_match) || (n_need_runs && !d_need_runs) || (n_pool_runs && !d_pool_runs) ||
      (cap_extents && !d_extents) || !d_work || !d_res)
    return fail(CIR_EINVAL, "null device pointer");
  const int given = (d_src != nullptr) + (d_file != nullptr) + (d_block != nullptr);
  if (given != 0 && given != 3)
    return fail(CIR_EINVAL, "the per-block arrays are given all three or none");
  if (addr(d_match) & 3u || addr(d_src) & 3u)
    return fail(CIR_EINVAL, "d_match and d_src must be 4-byte aligned");
  if ((addr(d_need_runs) | addr(d_pool_runs) | addr(d_want) | addr(d_file) | addr(d_block) |
       addr(d_fetch) | addr(d_extents) | addr(d_work) | addr(d_res)) & 7u)
    return fail(CIR_EINVAL,
                "run tables, bitmaps, u64 arrays, scratch and result must be 8-byte aligned");
  if (bs == 0) return fail(CIR_EINVAL, "block_size is 0");
  if (n_need > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 needed blocks");
  if (n_pool > dev::kJoinMaxPool) return fail(CIR_EINVAL, "more than 2^31-1 pool blocks");
  if (cap_extents > (1ull << 57)) return fail(CIR_EINVAL, "cap_extents x 64 bytes passes 2^63");
  if (work_bytes < dev::ext_work_bytes(n_need))
    return fail(CIR_EINVAL, "work_bytes is below cir_extents_work_bytes(n_need)");
  const dev::ExtentArgs a{d_match, n_need, d_need_runs, n_need_runs, d_pool_runs,
                          n_pool_runs, n_pool, bs, d_want};
  hipStream_t s = (hipStream_t)stream;
  CIR_HIP(dev::launch_extent_map(a, d_src, d_file, d_block, d_fetch, cap_extents,
                                 (uint64_t*)d_work, d_res, s));
  CIR_HIP(dev::launch_extent_emit(a, d_extents, cap_extents, n_need, (uint64_t*)d_work, d_res, s));
  return CIR_OK;
}

struct Laps {
  double upload = 0, build = 0, probe = 0, download = 0;
};

// The join on ctx's first device: buffers for the call, one upload of each
// list, launch_join on the device's compute stream, one download.  need, pool
// and match are the caller's and outlive the call's drain.
int device_join(cir_ctx* ctx, const std::vector<uint8_t>& need, uint64_t n_need,
                const std::vector<uint8_t>& pool, uint64_t n_pool, uint64_t slots,
                uint32_t* match, bool trace, Laps* laps) {
  TraceEvents<3> jev;
  DeviceCall c(ctx);
  int rc;
  if ((rc = c.begin())) return rc;
  uint8_t* d_need = nullptr;
  uint8_t* d_pool = nullptr;
  uint32_t* d_table = nullptr;
  uint32_t* d_match = nullptr;
  if ((rc = c.alloc(&d_need, std::max<size_t>(32 * n_need, 32))) ||
      (rc = c.alloc(&d_pool, std::max<size_t>(32 * n_pool, 32))) ||
      (rc = c.alloc(&d_table, slots * sizeof(uint32_t))) ||
      (rc = c.alloc(&d_match, (n_need + 4) * sizeof(uint32_t))))
    return rc;
  if (trace && (rc = jev.create())) return rc;
  hipStream_t s = c.s;
  const auto t0 = Clock::now();
  CIR_HIP(hipMemcpyAsync(d_need, need.data(), 32 * n_need, hipMemcpyHostToDevice, s));
  if (n_pool) CIR_HIP(hipMemcpyAsync(d_pool, pool.data(), 32 * n_pool, hipMemcpyHostToDevice, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t1 = Clock::now();
  CIR_HIP(dev::launch_join(d_need, n_need, d_pool, n_pool, d_table, slots, draw_seed(), d_match,
                           d_match + n_need, s, trace ? jev.ev : nullptr));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t2 = Clock::now();
  CIR_HIP(hipMemcpyAsync(match, d_match, n_need * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  if (trace) {
    laps->build = jev.lap(0);
    laps->probe = jev.lap(1);
    laps->upload = ms_between(t0, t1);
    laps->download = ms_between(t2, Clock::now());
  }
  return CIR_OK;
}

// CIR_SOURCES_MAP, read per call: "host" keeps sources::map_matches (and
// extents_of) on a host thread behind the device join, "device" runs
// k_map_matches there whatever the size.  Unset: cir_block_extents maps on
// the device, and so does cir_block_sources from kMapDeviceMinBlocks needed
// blocks on.  Below that the device map's fixed cost (six more hipMalloc,
// one more upload, three more downloads: about 0.13 ms) is more than the host
// loop's: one source of n blocks against n, whole call, device map against
// the parent commit's build (profiles/block_extents/size_sweep.json): n =
// 4,000 0.42-0.45 ms against 0.33-0.34; 8,000 0.44-0.51 against 0.47-0.49, a
// tie; 16,000 0.50-0.54 against 0.75-0.77; 128,000 1.87-1.91 against 6.73-6.76.
constexpr uint64_t kMapDeviceMinBlocks = 16384;
bool map_on_device(bool extents, uint64_t n_need) {
  const char* v = getenv("CIR_SOURCES_MAP");
  if (v && strcmp(v, "host") == 0) return false;
  if (v && strcmp(v, "device") == 0) return true;
  return extents || n_need >= kMapDeviceMinBlocks;
}

// Where a call's answer goes: cir_block_sources' three arrays, or
// cir_block_extents' records and fetch bitmap.  One flow serves both.
struct Answer {
  bool extents = false;
  uint32_t** src_out = nullptr;
  uint64_t** src_file_out = nullptr;
  uint64_t** src_block_out = nullptr;
  uint64_t** extents_out = nullptr;
  size_t* nextents_out = nullptr;
  uint64_t** fetch_out = nullptr;
  uint64_t* nblk_out = nullptr;
  size_t* nskipped_out = nullptr;
  uint64_t* stats = nullptr;
  int nstats() const { return extents ? CIR_EXTENTS_STATS_FIELDS : CIR_SOURCES_STATS_FIELDS; }
  void clear() const {
    if (extents) {
      *extents_out = nullptr;
      *nextents_out = 0;
      *fetch_out = nullptr;
    } else {
      *src_out = nullptr;
      *src_file_out = nullptr;
      *src_block_out = nullptr;
    }
    *nblk_out = 0;
    if (nskipped_out) *nskipped_out = 0;
    for (int i = 0; i < nstats(); ++i) stats[i] = 0;
  }
};

// match[] to the answer on the host: sources::map_matches, and extents_of
// behind it for cir_block_extents.  need.n > 0.
int answer_on_host(const Answer& a, const sources::BlockList& need,
                   const sources::BlockList& pool, uint64_t bs, const uint64_t* want,
                   const uint32_t* match) {
  const uint64_t n = need.n;
  uint32_t* so = (uint32_t*)malloc(n * sizeof(uint32_t));
  uint64_t* fo = (uint64_t*)malloc(n * sizeof(uint64_t));
  uint64_t* bo = (uint64_t*)malloc(n * sizeof(uint64_t));
  auto drop = [&](int rc) {
    free(so);
    free(fo);
    free(bo);
    return rc;
  };
  if (!so || !fo || !bo) return drop(fail(CIR_ENOMEM, "malloc"));
  const sources::MapStats ms = sources::map_matches(need, pool, bs, want, match, so, fo, bo);
  a.stats[0] = ms.wanted;
  a.stats[1] = ms.found;
  a.stats[2] = ms.bytes;
  a.stats[5] = ms.dropped;
  *a.nblk_out = n;
  if (!a.extents) {
    *a.src_out = so;
    *a.src_file_out = fo;
    *a.src_block_out = bo;
    return CIR_OK;
  }
  if (!sources::extents_owned(need, bs, want, so, fo, bo, a.extents_out, a.nextents_out,
                              a.fetch_out, &a.stats[9])) {
    *a.nblk_out = 0;
    return drop(fail(CIR_ENOMEM, "malloc"));
  }
  a.stats[8] = *a.nextents_out;
  return drop(CIR_OK);
}

// One index text of a call with the device parse.
struct Text {
  const uint8_t* p = nullptr;
  size_t len = 0;
  dirsig::Header h;
  size_t body_off = 0, body_end = 0;
  bool framed = false;     // dirsig::frame took it
  bool candidate = false;  // takes part unless its body does not parse
  bool dev = false;        // its body is parsed on the device in this attempt
  bool usable = false;
  uint64_t nblk = 0;
  size_t slot = 0;       // device path: its place in this attempt's TextSet
  dirsig::Index parsed;  // on the host path
  std::string err;
  bool host_done = false, host_ok = false;  // dirsig::parse ran / took it
  std::vector<uint8_t> digests;       // host path: its digests, until they are uploaded
};

// What an attempt returns besides a CIR_* code (none of those is positive).
constexpr int kRetry = 1;     // again, with more texts on the host
struct DevLaps {
  double frame = 0, text_upload = 0, count = 0, host_parse = 0, decode = 0, runs_download = 0;
  double upload = 0, build = 0, probe = 0, download = 0, map = 0;
  double tables_upload = 0, scan = 0, emit = 0;  // the device map's (answer_on_device)
};

// match[] (d_match, on the device behind the join) to the answer with the
// kernels of extents.hip, on stream s: the combined run tables go up (32
// bytes per file; *tabs, which outlives the stream's work), k_map_matches and
// k_extent_scan run, and then
//   cir_block_sources   the three per-block arrays and the counts come down;
//   cir_block_extents   the counts come down, one synchronise learns the
//                       extent count, the records are allocated exactly,
//                       emitted and downloaded with the fetch bitmap; the
//                       per-block arrays are never made.
// need.n > 0.  x_res, like *tabs, is the caller's and outlives c's drain.
int answer_on_device(const Answer& a, const sources::BlockList& need,
                     const sources::BlockList& pool, uint64_t n_pool, uint64_t bs,
                     const uint64_t* want, const uint32_t* d_match, DeviceCall& c,
                     std::vector<uint64_t>* tabs, uint64_t* x_res, bool trace, DevLaps* laps) {
  hipStream_t s = c.s;
  const uint64_t n = need.n, nwords = (n + 63) / 64;
  const size_t nr = need.runs.size(), pr = pool.runs.size();
  tabs->resize(4 * (nr + pr));
  sources::pack_runs(need, tabs->data());
  sources::pack_runs(pool, tabs->data() + 4 * nr);
  uint64_t* d_tabs = nullptr;
  uint64_t* d_want = nullptr;
  uint64_t* d_work = nullptr;
  uint64_t* d_xres = nullptr;
  uint32_t* d_so = nullptr;
  uint64_t* d_fo = nullptr;
  uint64_t* d_bo = nullptr;
  uint64_t* d_fetch = nullptr;
  int rc;
  if ((rc = c.alloc(&d_tabs, 32 * (nr + pr))) ||
      (want && (rc = c.alloc(&d_want, 8 * nwords))) ||
      (rc = c.alloc(&d_work, dev::ext_work_bytes(n))) ||
      (rc = c.alloc(&d_xres, sizeof(uint64_t) * extents::kResFields)))
    return rc;
  if (a.extents) {
    if ((rc = c.alloc(&d_fetch, 8 * nwords))) return rc;
  } else if ((rc = c.alloc(&d_so, 4 * n)) || (rc = c.alloc(&d_fo, 8 * n)) ||
             (rc = c.alloc(&d_bo, 8 * n))) {
    return rc;
  }
  const auto t0 = Clock::now();
  CIR_HIP(hipMemcpyAsync(d_tabs, tabs->data(), 32 * (nr + pr), hipMemcpyHostToDevice, s));
  if (want) CIR_HIP(hipMemcpyAsync(d_want, want, 8 * nwords, hipMemcpyHostToDevice, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t1 = Clock::now();
  const dev::ExtentArgs args{d_match, n, d_tabs, nr, d_tabs + 4 * nr, pr, n_pool, bs, d_want};
  // (no cap: the count decides the allocation, not the other way round)
  TraceEvents<3> tev;
  if (trace && (rc = tev.create())) return rc;
  CIR_HIP(dev::launch_extent_map(args, d_so, d_fo, d_bo, d_fetch, ~0ull, d_work, d_xres, s,
                                 trace ? tev.ev : nullptr));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t2 = Clock::now();
  uint32_t* so = nullptr;
  uint64_t* fo = nullptr;
  uint64_t* bo = nullptr;
  auto drop = [&](int code) {
    (void)hipStreamSynchronize(s);  // (no copy is in flight into what is freed)
    free(so);
    free(fo);
    free(bo);
    return code;
  };
  hipError_t e = hipSuccess;
  if (!a.extents) {
    so = (uint32_t*)malloc(n * sizeof(uint32_t));
    fo = (uint64_t*)malloc(n * sizeof(uint64_t));
    bo = (uint64_t*)malloc(n * sizeof(uint64_t));
    if (!so || !fo || !bo) return drop(fail(CIR_ENOMEM, "malloc"));
    if ((e = hipMemcpyAsync(so, d_so, 4 * n, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipMemcpyAsync(fo, d_fo, 8 * n, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipMemcpyAsync(bo, d_bo, 8 * n, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return drop(hip_fail(e, "download of the per-block arrays"));
  }
  if ((e = hipMemcpyAsync(x_res, d_xres, sizeof(uint64_t) * extents::kResFields,
                          hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipStreamSynchronize(s)) != hipSuccess)
    return drop(hip_fail(e, "download of the map's counts"));
  const auto t3 = Clock::now();
  auto t4 = t3;
  if (a.extents) {
    const uint64_t count = x_res[5];
    if ((rc = device_extent_tail(c, args, count, d_work, d_xres, d_fetch, trace, a.extents_out,
                                 a.fetch_out, &t4)))
      return rc;
    *a.nextents_out = count;
    a.stats[8] = count;
    a.stats[9] = x_res[1] - x_res[2];
  } else {
    *a.src_out = so;
    *a.src_file_out = fo;
    *a.src_block_out = bo;
  }
  a.stats[0] = x_res[1];
  a.stats[1] = x_res[2];
  a.stats[2] = x_res[3];
  a.stats[5] = x_res[4];
  *a.nblk_out = n;
  if (trace) {
    laps->tables_upload = ms_between(t0, t1);
    laps->map = tev.lap(0);
    laps->scan = tev.lap(1);
    laps->emit = ms_between(t3, t4);
    laps->download = ms_between(t2, t3) + ms_between(t4, Clock::now());
    fprintf(stderr,
            "cir extents map (block_%s): %llu blocks; tables upload %.2f ms (%zu + %zu runs), map "
            "kernel %.3f ms, scan kernel %.3f ms, emit kernels %.3f ms, downloads %.2f ms; %llu "
            "extents, %llu bytes downloaded\n",
            a.extents ? "extents" : "sources", (unsigned long long)n, laps->tables_upload, nr, pr,
            laps->map, laps->scan, laps->emit, laps->download, (unsigned long long)x_res[5],
            (unsigned long long)(a.extents ? 64 * x_res[5] + 8 * nwords + 48 : 20 * n + 48));
  }
  return CIR_OK;
}

// One attempt of cir_block_sources with the texts parsed on the device.
// force_host[k]: text k (nsrc = the new index) goes through the host parser.
// Returns kRetry, with more force_host flags set, when a token turned out bad
// in the decode pass: by then the pool's layout rested on that text's counts.
// The counts of the count pass are provisional until the decode pass has given
// its verdicts, so nothing is reported from them alone: a call they would end
// without a decode pass -- a new index without blocks, a pool or a need list
// past its limit -- returns kHostFlow and is decided by the host parser.
// No text is kept from the device for being small: one source of n blocks
// against n, whole call, device parse against CIR_SOURCES_PARSE=host
// (profiles/index_digests/bench.json, size_sweep): n = 500 (33 KB per text)
// 0.22-0.25 ms against 0.18-0.33 ms, a tie; 2,000 0.25-0.29 against 0.64-0.75;
// 512,000 6.8-6.9 against 132-138.  No size was found at which the host wins.
int sources_dev_attempt(cir_ctx* ctx, std::vector<Text>& tx, size_t nsrc,
                        std::vector<uint8_t>& force_host, const uint64_t* want, const Answer& ans,
                        bool trace, DevLaps* laps) {
  size_t* const nskipped_out = ans.nskipped_out;
  uint64_t* const stats = ans.stats;
  Text& nw = tx[nsrc];
  const auto t0 = Clock::now();
  auto host_parse = [&](Text& t) {  // (once per text: a second attempt keeps the first's)
    if (t.host_done) return;
    t.host_ok = t.p && dirsig::parse(t.p, t.len, &t.parsed, &t.err);
    t.host_done = true;
  };
  auto want_dev = [&](size_t k) {
    const Text& t = tx[k];
    return t.framed && !force_host[k] && device_takes(t.len);
  };
  // the new index first: its header decides which sources take part
  nw.dev = want_dev(nsrc);
  if (!nw.dev) {
    host_parse(nw);
    if (!nw.host_ok) return parse_fail(nw.parsed.bad_hash_size, nw.err);
    nw.h = nw.parsed.header;
  }
  std::vector<size_t> on_host, on_dev;
  if (nw.dev) on_dev.push_back(nsrc);
  for (size_t j = 0; j < nsrc; ++j) {
    Text& t = tx[j];
    t.candidate = t.framed && t.h.hash == nw.h.hash && t.h.block_size == nw.h.block_size;
    t.dev = t.candidate && want_dev(j);
    t.usable = false;
    if (t.dev)
      on_dev.push_back(j);
    else if (t.candidate)
      on_host.push_back(j);
  }
  if (nsrc > 0xFFFFFFFEull) return fail(CIR_EINVAL, "too many sources");
  const uint64_t bs = nw.h.block_size;
  // the host's share first: the device's lock is not held across a host parse
  const auto th0 = Clock::now();
  fan_out(on_host.size(), [&](size_t i) { host_parse(tx[on_host[i]]); });
  const double host_first_ms = ms_between(th0, Clock::now());

  // host memory that asynchronous copies read or write: declared before the call
  TextSet ts;  // the texts, their scratch, result words and run tables
  for (size_t k : on_dev) tx[k].slot = ts.add(tx[k].p, tx[k].len, tx[k].body_off, tx[k].body_end);
  std::vector<uint64_t> tabs;  // the combined run tables, uploaded for the device map
  uint64_t x_res[extents::kResFields] = {0, 0, 0, 0, 0, 0};
  TraceEvents<3> jev;
  DeviceCall c(ctx);
  hipStream_t s = c.s;
  int rc;
  if ((rc = c.begin()) || (rc = ts.count(c, bs, 0, trace))) return rc;
  const auto t1 = ts.t_bufs, t2 = ts.t_up, t5 = ts.t_counted;
  // what the count pass declined takes the host parser, that text alone
  std::vector<size_t> declined;
  for (size_t k : on_dev) {
    Text& t = tx[k];
    if (!ts.counted_ok(t.slot)) {
      t.dev = false;
      force_host[k] = 1;
      declined.push_back(k);
    } else {
      t.usable = true;
      t.nblk = ts.item[t.slot].cnt[3];
    }
  }
  if (!declined.empty()) {
    c.unlock();
    fan_out(declined.size(), [&](size_t i) { host_parse(tx[declined[i]]); });
    c.lock();
  }
  if (!nw.dev) {
    if (!nw.host_ok) return parse_fail(nw.parsed.bad_hash_size, nw.err);
    nw.usable = true;  // (its header is the frame's: both read it by the same rules)
    nw.nblk = sources::count_blocks(nw.parsed);
  }
  for (size_t j = 0; j < nsrc; ++j) {
    Text& t = tx[j];
    if (t.dev || !t.candidate) continue;
    t.usable = t.host_ok && t.parsed.header.hash == nw.h.hash &&
               t.parsed.header.block_size == nw.h.block_size;
    t.nblk = t.usable ? sources::count_blocks(t.parsed) : 0;
  }
  const auto t6 = Clock::now();
  size_t used = 0;
  uint64_t n_pool = 0;
  for (size_t j = 0; j < nsrc; ++j)
    if (tx[j].usable) {
      ++used;
      n_pool += tx[j].nblk;
    }
  const uint64_t n_need = nw.nblk;
  // (a source's count may still fall to a bad token: the host parser decides
  // what ends here, before any join, exactly as without the device parse)
  if (n_need == 0 || n_need > 0xFFFFFFFFull || !sources::pool_count_ok(n_pool)) return kHostFlow;
  // the join's buffers; the digests are decoded, or uploaded, straight into them
  const uint64_t slots = dev::join_table_slots(n_pool);
  uint8_t* d_need = nullptr;
  uint8_t* d_pool = nullptr;
  uint32_t* d_table = nullptr;
  uint32_t* d_match = nullptr;
  if ((rc = c.alloc(&d_need, 32 * n_need)) || (rc = c.alloc(&d_pool, 32 * n_pool)) ||
      (rc = c.alloc(&d_table, slots * sizeof(uint32_t))) ||
      (rc = c.alloc(&d_match, (n_need + 4) * sizeof(uint32_t))) || (trace && (rc = jev.create())))
    return rc;
  uint64_t at = 0;  // pool ordinal of the next source's block 0
  double upload_ms = 0;
  for (size_t k = 0; k <= nsrc; ++k) {
    const size_t j = k == 0 ? nsrc : k - 1;  // the new index, then the sources in order
    Text& t = tx[j];
    if (!t.usable) continue;
    uint8_t* dst = j == nsrc ? d_need : d_pool + 32 * at;
    if (t.dev) {
      if ((rc = ts.emit(c, t.slot, dst, t.nblk))) return rc;
    } else if (t.nblk) {
      const auto u0 = Clock::now();
      t.digests.resize(32 * t.nblk);
      sources::copy_digests(t.parsed, t.digests.data());
      CIR_HIP(hipMemcpyAsync(dst, t.digests.data(), 32 * t.nblk, hipMemcpyHostToDevice, s));
      upload_ms += ms_between(u0, Clock::now());
    }
    if (j != nsrc) at += t.nblk;
  }
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t7 = Clock::now();
  // the verdicts again (a bad token shows only now) and the run tables
  if ((rc = ts.finish(c, true))) return rc;
  const auto t8 = Clock::now();
  bool again = false;
  for (size_t k : on_dev)
    if (tx[k].dev && ts.status(tx[k].slot) != CIR_INDEX_OK) {
      force_host[k] = 1;
      again = true;
    }
  if (again) return kRetry;
  // every verdict is in: the counts are the host parser's
  if (nskipped_out) *nskipped_out = nsrc - used;
  stats[3] = n_pool;
  stats[4] = used;
  stats[7] = 1;
  // the block lists, from the run tables
  sources::BlockList need, pool;
  for (size_t k = 0; k <= nsrc; ++k) {
    const size_t j = k == 0 ? nsrc : k - 1;
    Text& t = tx[j];
    if (!t.usable) continue;
    sources::BlockList* list = j == nsrc ? &need : &pool;
    const uint32_t src = j == nsrc ? 0 : (uint32_t)j;
    if (t.dev) {
      for (const idxscan::Run& r : ts.item[t.slot].runs)
        list->runs.push_back(sources::FileRun{list->n + r.first, r.size, r.file, src});
      list->n += t.nblk;
    } else {
      sources::append_runs(t.parsed, src, list);
      t.parsed = dirsig::Index();
      t.digests = std::vector<uint8_t>();
    }
  }
  stats[6] = slots;
  hipError_t e = dev::launch_join(d_need, n_need, d_pool, n_pool, d_table, slots, draw_seed(),
                                  d_match, d_match + n_need, s, trace ? jev.ev : nullptr);
  if (e != hipSuccess) return hip_fail(e, "launch_join");
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t9 = Clock::now();
  auto t10 = t9;
  const bool dev_map = map_on_device(ans.extents, n_need);
  if (!dev_map) {
    std::vector<uint32_t> match(n_need);
    CIR_HIP(hipMemcpyAsync(match.data(), d_match, n_need * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           s));
    CIR_HIP(hipStreamSynchronize(s));
    t10 = Clock::now();
    if ((rc = answer_on_host(ans, need, pool, bs, want, match.data()))) return rc;
  } else {
    if ((rc = answer_on_device(ans, need, pool, n_pool, bs, want, d_match, c, &tabs, x_res, trace,
                               laps)))
      return rc;
    t10 = Clock::now();
  }
  if (trace) {
    laps->build = jev.lap(0);
    laps->probe = jev.lap(1);
    laps->frame += ms_between(t0, t1);  // (with the host's share and the buffers' hipMalloc)
    laps->text_upload += ms_between(t1, t2);
    laps->count += ms_between(t2, t5);
    laps->host_parse += host_first_ms + ms_between(t5, t6);
    laps->decode += ms_between(t6, t7) - upload_ms;
    laps->upload += upload_ms;
    laps->runs_download += ms_between(t7, t8);
    if (!dev_map) {
      laps->download = ms_between(t9, t10);
      laps->map = ms_between(t10, Clock::now());
    }
    fprintf(stderr,
            "cir block_sources: %llu blocks against %llu pool blocks of %zu source(s), device; "
            "parse %.2f ms, pool %.2f ms, upload %.2f ms, build kernel %.3f ms, probe kernel "
            "%.3f ms, download %.2f ms, map %.2f ms; device parse of %zu text(s): frame %.2f ms, "
            "text upload %.2f ms, count kernels %.2f ms, host parse %.2f ms, decode kernels "
            "%.2f ms, runs download %.2f ms\n",
            (unsigned long long)n_need, (unsigned long long)n_pool, used, ms_between(t0, t8), 0.0,
            laps->upload, laps->build, laps->probe, laps->download, laps->map, on_dev.size(),
            laps->frame, laps->text_upload, laps->count, laps->host_parse, laps->decode,
            laps->runs_download);
  }
  return CIR_OK;
}

// cir_block_sources / cir_block_extents with a context: the texts are framed
// on the host and their bodies parsed on the device, straight into the join's
// buffers.
int block_sources_dev(cir_ctx* ctx, const uint8_t* index, size_t len,
                      const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                      const uint64_t* want, const Answer& ans, bool trace) {
  std::vector<Text> tx(nsrc + 1);
  for (size_t k = 0; k <= nsrc; ++k) {
    Text& t = tx[k];
    t.p = k == nsrc ? index : src_index[k];
    t.len = k == nsrc ? len : src_len[k];
    std::string err;
    t.framed = t.p && dirsig::frame(t.p, t.len, &t.h, &t.body_off, &t.body_end, &err);
  }
  std::vector<uint8_t> force_host(nsrc + 1, 0);
  DevLaps laps;
  for (;;) {  // (again only after a bad token: at most once per text)
    const int rc = sources_dev_attempt(ctx, tx, nsrc, force_host, want, ans, trace, &laps);
    if (rc != kRetry) return rc;
  }
}

int block_sources_impl(cir_ctx* ctx, const uint8_t* index, size_t len,
                       const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                       const uint64_t* want, const Answer& ans) {
  uint64_t* const stats = ans.stats;
  size_t* const nskipped_out = ans.nskipped_out;
  const bool outs = ans.extents ? ans.extents_out && ans.nextents_out && ans.fetch_out
                                : ans.src_out && ans.src_file_out && ans.src_block_out;
  if (!index || !outs || !ans.nblk_out || !stats || (nsrc && (!src_index || !src_len)))
    return fail(CIR_EINVAL, "null pointer");
  ans.clear();
  const bool trace = trace_enabled();
  if (ctx && !parse_on_host()) {
    const int rc = block_sources_dev(ctx, index, len, src_index, src_len, nsrc, want, ans, trace);
    if (rc != kHostFlow) return rc;  // (nothing was reported yet)
  }
  const auto t0 = Clock::now();
  // the new index and the sources, parsed in parallel; a source that does
  // not parse or has another hash type or block size takes no part
  dirsig::Index idx;
  std::string err;
  bool index_ok = false;
  std::vector<dirsig::Index> parsed(nsrc);
  std::vector<uint8_t> usable(nsrc, 0);
  fan_out(nsrc + 1, [&](size_t k) {
    if (k == nsrc) {
      index_ok = dirsig::parse(index, len, &idx, &err);
      return;
    }
    std::string serr;
    usable[k] = src_index[k] && dirsig::parse(src_index[k], src_len[k], &parsed[k], &serr);
  });
  if (!index_ok) return parse_fail(idx.bad_hash_size, err);
  for (size_t j = 0; j < nsrc; ++j)
    usable[j] = usable[j] && parsed[j].header.hash == idx.header.hash &&
                parsed[j].header.block_size == idx.header.block_size;
  const auto t1 = Clock::now();
  size_t used = 0;
  uint64_t n_pool = 0;
  for (size_t j = 0; j < nsrc; ++j)
    if (usable[j]) {
      ++used;
      n_pool += sources::count_blocks(parsed[j]);
    }
  if (nskipped_out) *nskipped_out = nsrc - used;
  if (!sources::pool_count_ok(n_pool))
    return fail(CIR_EINVAL, "more than 2^31-1 pool blocks: pass fewer sources");
  if (nsrc > 0xFFFFFFFEull) return fail(CIR_EINVAL, "too many sources");
  const uint64_t bs = idx.header.block_size;
  sources::BlockList need, pool;
  sources::append_runs(idx, 0, &need);
  if (need.n > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 blocks in the index");
  stats[3] = n_pool;
  stats[4] = used;
  stats[7] = ctx ? 1 : 0;  // (an index without blocks has nothing to join, on either side)
  if (need.n == 0) return CIR_OK;
  // one contiguous buffer per list
  std::vector<uint8_t> need_d(32 * need.n), pool_d(32 * n_pool);
  sources::copy_digests(idx, need_d.data());
  for (size_t j = 0; j < nsrc; ++j)
    if (usable[j]) {
      sources::copy_digests(parsed[j], pool_d.data() + 32 * pool.n);
      sources::append_runs(parsed[j], (uint32_t)j, &pool);
      parsed[j] = dirsig::Index();  // (its digests now live in the pool)
    }
  std::vector<uint32_t> match(need.n);
  const auto t2 = Clock::now();
  Laps laps;
  double host_join_ms = 0;
  if (ctx) {
    const uint64_t slots = dev::join_table_slots(n_pool);
    const int rc = device_join(ctx, need_d, need.n, pool_d, n_pool, slots, match.data(), trace, &laps);
    if (rc) return rc;
    stats[6] = slots;
  } else {
    sources::host_join(need_d.data(), need.n, pool_d.data(), n_pool, want, match.data(),
                       draw_seed());
    host_join_ms = ms_between(t2, Clock::now());
  }
  const auto t3 = Clock::now();
  {
    const int rc = answer_on_host(ans, need, pool, bs, want, match.data());
    if (rc) return rc;
  }
  if (trace) {
    const double map_ms = ms_between(t3, Clock::now());
    if (ctx)
      fprintf(stderr,
              "cir block_sources: %llu blocks against %llu pool blocks of %zu source(s), device; "
              "parse %.2f ms, pool %.2f ms, upload %.2f ms, build kernel %.3f ms, probe kernel "
              "%.3f ms, download %.2f ms, map %.2f ms\n",
              (unsigned long long)need.n, (unsigned long long)n_pool, used, ms_between(t0, t1),
              ms_between(t1, t2), laps.upload, laps.build, laps.probe, laps.download, map_ms);
    else
      fprintf(stderr,
              "cir block_sources: %llu blocks against %llu pool blocks of %zu source(s), host; "
              "parse %.2f ms, pool %.2f ms, join %.2f ms, map %.2f ms\n",
              (unsigned long long)need.n, (unsigned long long)n_pool, used, ms_between(t0, t1),
              ms_between(t1, t2), host_join_ms, map_ms);
  }
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" uint64_t cir_match_table_slots(uint64_t n_pool) {
  return cir::dev::join_table_slots(n_pool);
}

extern "C" int cir_match_digests_dev(cir_ctx* ctx, const uint8_t* d_need, size_t n_need,
                                     const uint8_t* d_pool, size_t n_pool, uint32_t* d_table,
                                     uint64_t table_slots, uint64_t seed, uint32_t* d_match,
                                     uint32_t* d_nmatch, void* stream) try {
  (void)ctx;  // no scratch, no side streams
  return cir::match_dev_impl(d_need, n_need, d_pool, n_pool, d_table, table_slots, seed, d_match,
                             d_nmatch, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_block_sources(cir_ctx* ctx, const uint8_t* index, size_t len,
                                 const uint8_t* const* src_index, const size_t* src_len,
                                 size_t nsrc, const uint64_t* want, uint32_t** src_out,
                                 uint64_t** src_file_out, uint64_t** src_block_out,
                                 uint64_t* nblk_out, size_t* nskipped_out,
                                 uint64_t stats[CIR_SOURCES_STATS_FIELDS]) try {
  cir::Answer ans;
  ans.src_out = src_out;
  ans.src_file_out = src_file_out;
  ans.src_block_out = src_block_out;
  ans.nblk_out = nblk_out;
  ans.nskipped_out = nskipped_out;
  ans.stats = stats;
  return cir::block_sources_impl(ctx, index, len, src_index, src_len, nsrc, want, ans);
} CIR_CATCH_BOUNDARY

extern "C" int cir_block_extents(cir_ctx* ctx, const uint8_t* index, size_t len,
                                 const uint8_t* const* src_index, const size_t* src_len,
                                 size_t nsrc, const uint64_t* want, uint64_t** extents_out,
                                 size_t* nextents_out, uint64_t** fetch_out, uint64_t* nblk_out,
                                 size_t* nskipped_out,
                                 uint64_t stats[CIR_EXTENTS_STATS_FIELDS]) try {
  cir::Answer ans;
  ans.extents = true;
  ans.extents_out = extents_out;
  ans.nextents_out = nextents_out;
  ans.fetch_out = fetch_out;
  ans.nblk_out = nblk_out;
  ans.nskipped_out = nskipped_out;
  ans.stats = stats;
  return cir::block_sources_impl(ctx, index, len, src_index, src_len, nsrc, want, ans);
} CIR_CATCH_BOUNDARY

extern "C" uint64_t cir_extents_work_bytes(uint64_t n_need) {
  return cir::dev::ext_work_bytes(n_need);
}

extern "C" uint64_t cir_debug_extent_tile_blocks(void) { return cir::dev::kExtTile; }

extern "C" int cir_match_extents_dev(cir_ctx* ctx, const uint32_t* d_match, uint64_t n_need,
                                     const uint64_t* d_need_runs, uint64_t n_need_runs,
                                     const uint64_t* d_pool_runs, uint64_t n_pool_runs,
                                     uint64_t n_pool, uint64_t block_size, const uint64_t* d_want,
                                     uint32_t* d_src, uint64_t* d_file, uint64_t* d_block,
                                     uint64_t* d_fetch, uint64_t* d_extents, uint64_t cap_extents,
                                     void* d_work, uint64_t work_bytes, uint64_t* d_res,
                                     void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::match_extents_dev_impl(d_match, n_need, d_need_runs, n_need_runs, d_pool_runs,
                                     n_pool_runs, n_pool, block_size, d_want, d_src, d_file,
                                     d_block, d_fetch, d_extents, cap_extents, d_work, work_bytes,
                                     d_res, stream);
} CIR_CATCH_BOUNDARY
