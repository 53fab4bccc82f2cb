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
// (no HIP); the device join is join.hip.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <chrono>
#include <random>
#include <string>
#include <vector>

#include "dirsig.hpp"
#include "runtime.hpp"
#include "sources.hpp"

namespace cir {
namespace {

static_assert(sources::kMaxPool == dev::kJoinMaxPool && sources::kNone == dev::kJoinEmpty,
              "the host rule and the device join share their limits");

uint64_t draw_seed() {
  uint64_t s = 0;
  if (getrandom(&s, sizeof s, 0) == (ssize_t)sizeof s) return s;
  std::random_device rd;
  return ((uint64_t)rd() << 32) ^ rd();
}

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

// Device memory of one call, freed on every return path.
struct DevBufs {
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~DevBufs() {
    for (void* q : p)
      if (q) (void)hipFree(q);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

struct Laps {
  double upload = 0, build = 0, probe = 0, download = 0;
};

// The join on ctx's first device: buffers for the call, one upload of each
// list, launch_join on the device's compute stream, one download.
int device_join(cir_ctx* ctx, const std::vector<uint8_t>& need, uint64_t n_need,
                const std::vector<uint8_t>& pool, uint64_t n_pool, uint64_t slots,
                uint32_t* match, bool trace, Laps* laps) {
  Device& d = *ctx->devs[0];
  std::lock_guard<std::mutex> lk(d.mu);
  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d.id));
  DevBufs b;
  const size_t bytes[4] = {std::max<size_t>(32 * n_need, 32), std::max<size_t>(32 * n_pool, 32),
                           (size_t)slots * sizeof(uint32_t), (n_need + 4) * sizeof(uint32_t)};
  for (int i = 0; i < 4; ++i)
    if (hipMalloc(&b.p[i], bytes[i]) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CIR_ENOMEM, "hipMalloc of the join's buffers");
    }
  if (trace)
    for (hipEvent_t& e : b.ev) CIR_HIP(hipEventCreate(&e));
  uint8_t* d_need = (uint8_t*)b.p[0];
  uint8_t* d_pool = (uint8_t*)b.p[1];
  uint32_t* d_table = (uint32_t*)b.p[2];
  uint32_t* d_match = (uint32_t*)b.p[3];
  hipStream_t s = d.compute;
  const auto t0 = Clock::now();
  CIR_HIP(hipMemcpyAsync(d_need, need.data(), 32 * n_need, hipMemcpyHostToDevice, s));
  if (n_pool) CIR_HIP(hipMemcpyAsync(d_pool, pool.data(), 32 * n_pool, hipMemcpyHostToDevice, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t1 = Clock::now();
  CIR_HIP(dev::launch_join(d_need, n_need, d_pool, n_pool, d_table, slots, draw_seed(), d_match,
                           d_match + n_need, s, trace ? b.ev : nullptr));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t2 = Clock::now();
  CIR_HIP(hipMemcpyAsync(match, d_match, n_need * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  if (trace) {
    float f = 0;
    CIR_HIP(hipEventElapsedTime(&f, b.ev[0], b.ev[1]));
    laps->build = f;
    CIR_HIP(hipEventElapsedTime(&f, b.ev[1], b.ev[2]));
    laps->probe = f;
    laps->upload = ms_between(t0, t1);
    laps->download = ms_between(t2, Clock::now());
  }
  return CIR_OK;
}

int block_sources_impl(cir_ctx* ctx, const uint8_t* index, size_t len,
                       const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                       const uint64_t* want, uint32_t** src_out, uint64_t** src_file_out,
                       uint64_t** src_block_out, uint64_t* nblk_out, size_t* nskipped_out,
                       uint64_t* stats) {
  if (!index || !src_out || !src_file_out || !src_block_out || !nblk_out || !stats ||
      (nsrc && (!src_index || !src_len)))
    return fail(CIR_EINVAL, "null pointer");
  *src_out = nullptr;
  *src_file_out = nullptr;
  *src_block_out = nullptr;
  *nblk_out = 0;
  if (nskipped_out) *nskipped_out = 0;
  for (int i = 0; i < CIR_SOURCES_STATS_FIELDS; ++i) stats[i] = 0;
  const bool trace = trace_enabled();
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
  if (!index_ok)
    return idx.bad_hash_size ? fail(CIR_EHASHSIZE, "hash size is unsupported: " + err)
                             : fail(CIR_EPARSE, "error parsing index: " + err);
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
  uint32_t* so = (uint32_t*)malloc(need.n * sizeof(uint32_t));
  uint64_t* fo = (uint64_t*)malloc(need.n * sizeof(uint64_t));
  uint64_t* bo = (uint64_t*)malloc(need.n * sizeof(uint64_t));
  if (!so || !fo || !bo) {
    free(so);
    free(fo);
    free(bo);
    return fail(CIR_ENOMEM, "malloc");
  }
  const auto t2 = Clock::now();
  Laps laps;
  double host_join_ms = 0;
  if (ctx) {
    const uint64_t slots = dev::join_table_slots(n_pool);
    const int rc = device_join(ctx, need_d, need.n, pool_d, n_pool, slots, match.data(), trace, &laps);
    if (rc) {
      free(so);
      free(fo);
      free(bo);
      return rc;
    }
    stats[6] = slots;
  } else {
    sources::host_join(need_d.data(), need.n, pool_d.data(), n_pool, want, match.data(),
                       draw_seed());
    host_join_ms = ms_between(t2, Clock::now());
  }
  const auto t3 = Clock::now();
  const sources::MapStats ms =
      sources::map_matches(need, pool, bs, want, match.data(), so, fo, bo);
  stats[0] = ms.wanted;
  stats[1] = ms.found;
  stats[2] = ms.bytes;
  stats[5] = ms.dropped;
  *src_out = so;
  *src_file_out = fo;
  *src_block_out = bo;
  *nblk_out = need.n;
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
  return cir::block_sources_impl(ctx, index, len, src_index, src_len, nsrc, want, src_out,
                                 src_file_out, src_block_out, nblk_out, nskipped_out, stats);
} CIR_CATCH_BOUNDARY
