// cir_update_blocks: the next version of an image loaded in the buffers that
// hold the previous one.
//
// cir_reload_blocks (reload.cpp) refuses a destination that overlaps a resident
// buffer: a block being overwritten may be another block's source.  This call
// takes them.  It is the same load (check.cpp's load_blocks_resident) with
// another memory half (reload.hpp ResidentFn): the resident hash, the digest
// upload and the join are reload's, then update.hpp's rule gives every block a
// class -- kept where it stands, copied directly, copied through a staging
// scratch, or left to the disk -- and k_copy_runs (copyblk.hip, unchanged) runs
// twice: phase 1 reads the resident buffers for the last time, phase 2 and the
// load pipeline's scatter write into them afterwards, in stream order.  The
// reference has no counterpart: it holds no image in device memory.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "devcall.hpp"
#include "reload.hpp"
#include "runtime.hpp"
#include "update.hpp"

namespace cir {
namespace {

static_assert(CIR_UPDATE_STATS_FIELDS == CIR_RELOAD_STATS_FIELDS + 5, "reload's stats, then five more");

// CIR_UPDATE=disk, read per call: the resident list is ignored and the call is
// cir_load_blocks into the same buffers (A/B measurement).
bool update_from_disk() {
  const char* v = getenv("CIR_UPDATE");
  return v && strcmp(v, "disk") == 0;
}

struct Update {
  void* const* d_data;
  // the resident buffers {address, size}, sorted by address, disjoint
  std::vector<std::pair<uint64_t, uint64_t>> held;
  uint64_t scratch_bytes;
  void* stream;
  uint64_t res[update::kResFields] = {};
  uint64_t hashed = 0, scratch_allocated = 0;
  // CIR_TRACE: the step's laps in ms {tables, resident hash, digest upload, join, plan + copy}
  double laps[5] = {0, 0, 0, 0, 0};
  uint64_t n_need = 0;
};

// The resident list, sorted by address; CIR_EINVAL when two buffers overlap.
int take_resident(Update& U, const void* const* d_have, const uint64_t* have_bytes, size_t nhave) {
  for (size_t k = 0; k < nhave; ++k) {
    const uint64_t at = reinterpret_cast<uintptr_t>(d_have[k]), size = have_bytes[k];
    if (!at || !size) continue;
    if (size > UINT64_MAX - at) return fail(CIR_EINVAL, "a resident buffer wraps the address space");
    U.held.push_back({at, size});
  }
  std::sort(U.held.begin(), U.held.end());
  for (size_t k = 1; k < U.held.size(); ++k)
    if (U.held[k].first < U.held[k - 1].first + U.held[k - 1].second)
      return fail(CIR_EINVAL, "two resident buffers overlap: the call writes into them");
  return CIR_OK;
}

// The memory half (reload.hpp ResidentFn): everything up to the first HIP call
// decides CIR_EINVAL; until the scratch is allocated nothing is written to a
// caller's buffer; the device work is queued on the caller's stream, behind
// whatever it holds, and waited for here.
int fill_in_place(Update& U, const stage::Layout& im, Device& d, std::vector<uint64_t>* mem) {
  const bool trace = trace_enabled();
  const auto t0 = Clock::now();
  const uint64_t bs = im.bs, n_need = im.nblk_total;
  const size_t nfiles = im.items.size();
  std::vector<uint64_t> dests(nfiles, 0), need_runs;
  std::vector<std::pair<uint64_t, uint64_t>> spans;
  for (size_t i = 0; i < nfiles; ++i) {
    const stage::Item& it = im.items[i];
    if (!it.nblk || !U.d_data[i]) continue;
    const uint64_t at = reinterpret_cast<uintptr_t>(U.d_data[i]);
    if (it.size > UINT64_MAX - at) return fail(CIR_EINVAL, "a destination wraps the address space");
    dests[i] = at;
    spans.push_back({at, at + it.size});
  }
  if (update::spans_overlap(std::move(spans)))
    return fail(CIR_EINVAL, "two destinations overlap");
  // the resident table over one arena, the lowest pointer (as cir_index_memory_dev's)
  std::vector<uint64_t> tab_off, tab_abs;  // {first_block, offset | address, size}
  uint64_t n_pool = 0;
  const uint64_t arena = U.held.empty() ? 0 : U.held[0].first;
  for (const auto& h : U.held) {
    const uint64_t off[3] = {n_pool, h.first - arena, h.second};
    tab_off.insert(tab_off.end(), off, off + 3);
    const uint64_t abs[3] = {n_pool, h.first, h.second};
    tab_abs.insert(tab_abs.end(), abs, abs + 3);
    n_pool += h.second / bs + (h.second % bs != 0);
    if (n_pool > dev::kJoinMaxPool) return fail(CIR_EINVAL, "more than 2^31-1 resident blocks");
  }
  if (n_need > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 blocks in the index");
  if (n_pool == 0 || n_need == 0) return CIR_OK;  // (nothing resident: cir_load_blocks)
  // the need side: the host parser's digests, flat, and one run per non-empty file
  std::vector<uint8_t> need_dig((size_t)(32 * n_need));
  for (size_t i = 0; i < nfiles; ++i) {
    const stage::Item& it = im.items[i];
    if (!it.nblk) continue;
    memcpy(need_dig.data() + 32 * it.first_blk, im.digests(it, 0), (size_t)(32 * it.nblk));
    const uint64_t run[4] = {it.first_blk, it.size, (uint64_t)i, 0};
    need_runs.insert(need_runs.end(), run, run + 4);
  }
  const uint64_t nwords = (n_need + 63) / 64, nbuf = U.held.size();
  const uint64_t slots = dev::join_table_slots(n_pool);
  mem->assign((size_t)nwords, 0);
  uint64_t* res = U.res;
  uint64_t c_res[2 * CIR_COPY_RES_FIELDS] = {};
  const auto t1 = Clock::now();
  // ---- nothing above made a HIP call
  hipStream_t s = (hipStream_t)U.stream;
  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d.id));
  DevSet b;
  StreamDrain drain{s};
  uint64_t *d_tab_off = nullptr, *d_tab_abs = nullptr, *d_off = nullptr, *d_need_runs = nullptr,
           *d_dests = nullptr, *d_bits = nullptr, *d_recs_a = nullptr, *d_recs_b = nullptr,
           *d_work = nullptr, *d_res = nullptr;
  uint32_t *d_len = nullptr, *d_table = nullptr, *d_match = nullptr;
  uint8_t *d_pool = nullptr, *d_need = nullptr, *d_scratch = nullptr;
  int rc;
  if ((rc = b.alloc((void**)&d_tab_off, 24 * nbuf)) || (rc = b.alloc((void**)&d_tab_abs, 24 * nbuf)) ||
      (rc = b.alloc((void**)&d_off, 8 * n_pool)) || (rc = b.alloc((void**)&d_len, 4 * n_pool)) ||
      (rc = b.alloc((void**)&d_pool, 32 * n_pool)) || (rc = b.alloc((void**)&d_need, 32 * n_need)) ||
      (rc = b.alloc((void**)&d_table, 4 * slots)) ||
      (rc = b.alloc((void**)&d_match, 4 * (n_need + 4))) ||
      (rc = b.alloc((void**)&d_need_runs, 8 * need_runs.size())) ||
      (rc = b.alloc((void**)&d_dests, 8 * nfiles)) || (rc = b.alloc((void**)&d_bits, 8 * nwords)) ||
      (rc = b.alloc((void**)&d_recs_a, 8 * copyblk::kRunWords * n_need)) ||
      (rc = b.alloc((void**)&d_recs_b, 8 * copyblk::kRunWords * n_need)) ||
      (rc = b.alloc((void**)&d_work, dev::update_plan_work_bytes(n_need))) ||
      (rc = b.alloc((void**)&d_res, sizeof U.res + sizeof c_res)))
    return rc;
  // 1. the resident blocks, hashed where they lie
  CIR_HIP(hipMemcpyAsync(d_tab_off, tab_off.data(), 24 * nbuf, hipMemcpyHostToDevice, s));
  CIR_HIP(hipMemcpyAsync(d_tab_abs, tab_abs.data(), 24 * nbuf, hipMemcpyHostToDevice, s));
  CIR_HIP(dev::launch_mem_desc(d_tab_off, nbuf, bs, n_pool, d_off, d_len, s));
  if ((rc = hash_desc_ordered(d, reinterpret_cast<const uint8_t*>((uintptr_t)arena), d_off, d_len,
                              n_pool, d_pool, s, im.ht)))
    return rc;
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t2 = Clock::now();
  // 2. the new index's digests, runs and destinations
  CIR_HIP(hipMemcpyAsync(d_need, need_dig.data(), 32 * n_need, hipMemcpyHostToDevice, s));
  CIR_HIP(hipMemcpyAsync(d_need_runs, need_runs.data(), 8 * need_runs.size(),
                         hipMemcpyHostToDevice, s));
  CIR_HIP(hipMemcpyAsync(d_dests, dests.data(), 8 * nfiles, hipMemcpyHostToDevice, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t3 = Clock::now();
  // 3. the join
  CIR_HIP(dev::launch_join(d_need, n_need, d_pool, n_pool, d_table, slots, draw_seed(), d_match,
                           d_match + n_need, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t4 = Clock::now();
  // 4. the classes and their counts; one synchronise learns them
  update::Plan plan{{d_match, n_need, d_need_runs, need_runs.size() / 4, d_dests, nfiles, d_tab_abs,
                     nbuf, n_pool, bs},
                    d_pool,
                    d_need,
                    U.scratch_bytes == UINT64_MAX ? update::kNoCap : U.scratch_bytes / 16,
                    0};
  CIR_HIP(dev::launch_update_count(plan, d_work, d_res, s));
  CIR_HIP(hipMemcpyAsync(res, d_res, sizeof U.res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  if (res[update::kARecs] > n_need || res[update::kBRecs] > res[update::kARecs] ||
      res[update::kBUnits] > res[update::kAUnits] ||
      (plan.cap_units != update::kNoCap && res[update::kBUnits] > plan.cap_units))
    return fail(CIR_EIO, "the update plan's counts do not fit the index");
  // 5. the scratch.  ---- nothing above wrote a byte of a caller's buffer
  if (res[update::kBUnits]) {
    if ((rc = b.alloc((void**)&d_scratch, 16 * res[update::kBUnits]))) return rc;
    U.scratch_allocated = 16 * res[update::kBUnits];
    plan.scratch = reinterpret_cast<uintptr_t>(d_scratch);
  }
  // 6. the bitmap and the tables; phase 1, the last read of the resident
  // buffers; phase 2, out of the scratch
  uint64_t* d_cres = d_res + update::kResFields;
  CIR_HIP(dev::launch_update_emit(plan, d_work, n_need, d_bits, d_recs_a, d_recs_b, d_res, s));
  CIR_HIP(dev::launch_copy_runs(d_recs_a, res[update::kARecs], res[update::kAUnits], d_cres, s));
  CIR_HIP(dev::launch_copy_runs(d_recs_b, res[update::kBRecs], res[update::kBUnits],
                                d_cres + CIR_COPY_RES_FIELDS, s));
  // 7. the memory bitmap, the counts and the copies' verdicts
  CIR_HIP(hipMemcpyAsync(mem->data(), d_bits, 8 * nwords, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(res, d_res, sizeof U.res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(c_res, d_cres, sizeof c_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  if (c_res[0] || c_res[1]) return fail(CIR_EIO, "the copy kernel met a bad record");
  if (res[update::kDirectBlocks] + res[update::kBRecs] != res[update::kARecs])
    return fail(CIR_EIO, "the update plan's two passes disagree");
  U.hashed = n_pool;
  if (trace) {
    const double laps[5] = {ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, t3),
                            ms_between(t3, t4), ms_between(t4, Clock::now())};
    memcpy(U.laps, laps, sizeof laps);
    U.n_need = n_need;
  }
  return CIR_OK;
}

int update_impl(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                uint32_t threads, void* const* d_data, size_t ndata, const void* const* d_have,
                const uint64_t* have_bytes, size_t nhave, uint64_t scratch_bytes, void* stream,
                uint64_t** have_out, uint64_t* nblk_out, uint8_t** state_out, int32_t** errno_out,
                size_t* nfiles_out, uint64_t* stats) {
  if (!stats) return fail(CIR_EINVAL, "null pointer");
  for (int i = 0; i < CIR_UPDATE_STATS_FIELDS; ++i) stats[i] = 0;
  if (nhave && (!d_have || !have_bytes)) return fail(CIR_EINVAL, "null pointer");
  const bool disk = update_from_disk();
  Update U{d_data, {}, scratch_bytes, stream};
  if (!disk) {
    const int rc = take_resident(U, d_have, have_bytes, nhave);
    if (rc) return rc;
  }
  const ResidentFn fn = [&U](const stage::Layout& im, Device& d, std::vector<uint64_t>* mem) {
    return fill_in_place(U, im, d, mem);
  };
  const auto t0 = Clock::now();
  const int rc = load_blocks_resident(ctx, dirfd, dir, index, len, threads, d_data, ndata, stream,
                                      disk ? nullptr : &fn, have_out, nblk_out, state_out,
                                      errno_out, nfiles_out, stats);
  if (rc) return rc;
  const uint64_t* r = U.res;
  stats[12] = r[update::kDirectBlocks] + r[update::kBRecs];
  stats[13] = r[update::kDirectBytes] + r[update::kStagedBytes];
  stats[14] = U.hashed;
  for (size_t i = 0; i < *nfiles_out; ++i)
    if ((*state_out)[i] & CIR_FILE_RESIDENT) ++stats[15];
  stats[16] = r[update::kDroppedMatches];
  stats[17] = r[update::kKeptBlocks];
  stats[18] = r[update::kKeptBytes];
  stats[19] = r[update::kBRecs];
  stats[20] = U.scratch_allocated;
  stats[21] = r[update::kDemotedBlocks];
  if (trace_enabled()) {
    const double whole = ms_between(t0, Clock::now());
    const double step = U.laps[0] + U.laps[1] + U.laps[2] + U.laps[3] + U.laps[4];
    fprintf(stderr,
            "cir update_blocks%s: %llu blocks against %llu resident blocks of %llu buffer(s); "
            "tables %.2f ms, resident hash %.2f ms, digest upload %.2f ms, join %.2f ms, plan + "
            "copy %.2f ms, index parse and pipeline %.2f ms, whole call %.2f ms; %llu blocks "
            "(%llu bytes) kept, %llu (%llu bytes) copied, %llu of them staged through %llu bytes, "
            "%llu demoted, %llu dropped, %llu files resident\n",
            disk ? " (CIR_UPDATE=disk)" : "", (unsigned long long)U.n_need,
            (unsigned long long)U.hashed, (unsigned long long)U.held.size(), U.laps[0], U.laps[1],
            U.laps[2], U.laps[3], U.laps[4], whole - step, whole, (unsigned long long)stats[17],
            (unsigned long long)stats[18], (unsigned long long)stats[12],
            (unsigned long long)stats[13], (unsigned long long)stats[19],
            (unsigned long long)stats[20], (unsigned long long)stats[21],
            (unsigned long long)stats[16], (unsigned long long)stats[15]);
  }
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" int cir_update_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index,
                                 size_t len, uint32_t threads, void* const* d_data, size_t ndata,
                                 const void* const* d_have, const uint64_t* have_bytes,
                                 size_t nhave, uint64_t scratch_bytes, void* stream,
                                 uint64_t** have_out, uint64_t* nblk_out, uint8_t** state_out,
                                 int32_t** errno_out, size_t* nfiles_out,
                                 uint64_t stats[CIR_UPDATE_STATS_FIELDS]) try {
  return cir::update_impl(ctx, dirfd, dir, index, len, threads, d_data, ndata, d_have, have_bytes,
                          nhave, scratch_bytes, stream, have_out, nblk_out, state_out, errno_out,
                          nfiles_out, stats);
} CIR_CATCH_BOUNDARY
