// cir_reload_blocks: the next version of an image loaded over the one held in
// device memory; cir_copy_runs, cir_copy_runs_dev: the copy behind it on its
// own.
//
// Reference: for the daemon's disk, "most blocks of version N + 1 are already
// here in version N" is what hardlinking and block reuse rest on (scan_links,
// src/daemon/metadata/hardlink_sources.rs:107-153).  A process that holds
// version N in device memory has no such path there or, until now, here:
// cir_load_blocks reads, uploads and hashes every byte again.
//
// The call is cir_load_blocks (check.cpp) with one step between the index's
// parse and the first look at the image directory (reload.hpp): the resident
// buffers are hashed where they lie (k_mem_desc + hash_desc_ordered, as
// cir_index_memory_dev does), the new index's digests are joined against them
// (join.hip), k_copy_plan turns the matches into a copy table and a bitmap, and
// k_copy_runs moves the blocks inside device memory (copyblk.hip; the rules are
// copyblk.hpp).  The load pipeline then reads only the blocks the bitmap lacks.
// The resident bytes are believed only as far as their digest, taken in this
// call, goes: no older index is asked for.
//
// The new index's digests and runs are the host parser's: the load pipeline
// needs the parsed index whatever happens here, so the digests go up as 32
// bytes per block instead of the text's 65 being parsed a second time on the
// device.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "copyblk.hpp"
#include "devcall.hpp"
#include "reload.hpp"
#include "runtime.hpp"

namespace cir {
namespace {

static_assert(CIR_COPY_RUN_WORDS == copyblk::kRunWords && CIR_COPY_RES_FIELDS == dev::kCopyResFields,
              "the header's constants are the rule's and the kernel's");
static_assert(CIR_RELOAD_STATS_FIELDS >= CIR_LOAD_STATS_FIELDS + 5, "load's stats, then five more");

// CIR_RELOAD=disk, read per call: the resident list is ignored and the call is
// cir_load_blocks (A/B measurement).
bool reload_from_disk() {
  const char* v = getenv("CIR_RELOAD");
  return v && strcmp(v, "disk") == 0;
}

int check_copy(const void* runs, uint64_t nruns, uint64_t nunits, const void* res) {
  if ((nruns && !runs) || !res) return fail(CIR_EINVAL, "null pointer");
  if (nruns > copyblk::kMaxRuns) return fail(CIR_EINVAL, "more than 2^32-1 records");
  if (nunits > copyblk::kMaxUnits) return fail(CIR_EINVAL, "more than 2^60 units");
  return CIR_OK;
}

int copy_host_impl(const uint64_t* runs, uint64_t nruns, uint64_t nunits, uint64_t* res) {
  const int rc = check_copy(runs, nruns, nunits, res);
  if (rc) return rc;
  res[0] = copyblk::apply_host(runs, nruns, nunits);
  return CIR_OK;
}

int copy_dev_impl(const uint64_t* d_runs, uint64_t nruns, uint64_t nunits, uint64_t* d_res,
                  void* stream) {
  const int rc = check_copy(d_runs, nruns, nunits, d_res);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(d_runs) | reinterpret_cast<uintptr_t>(d_res)) & 7u)
    return fail(CIR_EINVAL, "d_runs and d_res must be 8-byte aligned");
  CIR_HIP(dev::launch_copy_runs(d_runs, nruns, nunits, d_res, (hipStream_t)stream));
  return CIR_OK;
}

// One resident buffer, or one destination, as an interval of device addresses.
struct Span {
  uint64_t lo, hi;
  bool resident;
};

// Does any destination overlap any resident buffer?
bool spans_overlap(std::vector<Span>& v) {
  std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
  uint64_t end[2] = {0, 0};  // the furthest end so far of the destinations / of the resident buffers
  for (const Span& s : v) {
    if (s.lo < end[!s.resident]) return true;
    end[s.resident] = std::max(end[s.resident], s.hi);
  }
  return false;
}

struct Resident {
  void* const* d_data;
  const void* const* d_have;
  const uint64_t* have_bytes;
  size_t nhave;
  void* stream;
  // what the step found: blocks copied, their bytes, resident blocks hashed,
  // matches dropped for their length
  uint64_t copied = 0, bytes = 0, hashed = 0, dropped = 0;
  // CIR_TRACE: the step's laps in ms {tables, resident hash, digest upload, join, plan + copy}
  double laps[5] = {0, 0, 0, 0, 0};
  uint64_t n_need = 0, nbuf = 0;
};

// The memory half (reload.hpp ResidentFn): everything up to the first HIP call
// decides CIR_EINVAL; the device work is queued on the caller's stream, behind
// whatever it holds, and waited for here.
int fill_from_memory(Resident& R, const stage::Layout& im, Device& d, std::vector<uint64_t>* mem) {
  const bool trace = trace_enabled();
  const auto t0 = Clock::now();
  const uint64_t bs = im.bs, n_need = im.nblk_total;
  // the resident table over one arena, the lowest pointer (as cir_index_memory_dev's)
  std::vector<uint64_t> tab_off, tab_abs;  // {first_block, offset | address, size}
  std::vector<Span> spans;
  uint64_t n_pool = 0;
  uintptr_t arena = UINTPTR_MAX;
  for (size_t k = 0; k < R.nhave; ++k)
    if (R.d_have[k] && R.have_bytes[k])
      arena = std::min(arena, reinterpret_cast<uintptr_t>(R.d_have[k]));
  for (size_t k = 0; k < R.nhave; ++k) {
    const uint64_t size = R.have_bytes[k];
    if (!R.d_have[k] || !size) continue;
    const uint64_t at = reinterpret_cast<uintptr_t>(R.d_have[k]);
    if (size > UINT64_MAX - at) return fail(CIR_EINVAL, "a resident buffer wraps the address space");
    const uint64_t first[3] = {n_pool, at - arena, size};
    tab_off.insert(tab_off.end(), first, first + 3);
    const uint64_t abs[3] = {n_pool, at, size};
    tab_abs.insert(tab_abs.end(), abs, abs + 3);
    spans.push_back({at, at + size, true});
    n_pool += size / bs + (size % bs != 0);
    if (n_pool > dev::kJoinMaxPool) return fail(CIR_EINVAL, "more than 2^31-1 resident blocks");
  }
  if (n_need > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 blocks in the index");
  const size_t nfiles = im.items.size();
  std::vector<uint64_t> dests(nfiles, 0), need_runs;
  for (size_t i = 0; i < nfiles; ++i) {
    const stage::Item& it = im.items[i];
    if (!it.nblk || !R.d_data[i]) continue;
    const uint64_t at = reinterpret_cast<uintptr_t>(R.d_data[i]);
    dests[i] = at;
    spans.push_back({at, at + it.size, false});
  }
  if (spans_overlap(spans))
    return fail(CIR_EINVAL, "a destination overlaps a resident buffer: updating an image in the "
                            "buffers that hold it is not supported");
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
  const uint64_t nwords = (n_need + 63) / 64, nbuf = tab_off.size() / 3;
  const uint64_t slots = dev::join_table_slots(n_pool);
  mem->assign((size_t)nwords, 0);
  uint64_t p_res[copyblk::kPlanResFields] = {}, c_res[CIR_COPY_RES_FIELDS] = {};
  const auto t1 = Clock::now();
  // ---- nothing above made a HIP call
  hipStream_t s = (hipStream_t)R.stream;
  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d.id));
  DevSet b;
  StreamDrain drain{s};
  uint64_t *d_tab_off = nullptr, *d_tab_abs = nullptr, *d_off = nullptr, *d_need_runs = nullptr,
           *d_dests = nullptr, *d_bits = nullptr, *d_recs = nullptr, *d_work = nullptr,
           *d_res = nullptr;
  uint32_t *d_len = nullptr, *d_table = nullptr, *d_match = nullptr;
  uint8_t *d_pool = nullptr, *d_need = nullptr;
  int rc;
  if ((rc = b.alloc((void**)&d_tab_off, 24 * nbuf)) || (rc = b.alloc((void**)&d_tab_abs, 24 * nbuf)) ||
      (rc = b.alloc((void**)&d_off, 8 * n_pool)) || (rc = b.alloc((void**)&d_len, 4 * n_pool)) ||
      (rc = b.alloc((void**)&d_pool, 32 * n_pool)) || (rc = b.alloc((void**)&d_need, 32 * n_need)) ||
      (rc = b.alloc((void**)&d_table, 4 * slots)) ||
      (rc = b.alloc((void**)&d_match, 4 * (n_need + 4))) ||
      (rc = b.alloc((void**)&d_need_runs, 8 * need_runs.size())) ||
      (rc = b.alloc((void**)&d_dests, 8 * nfiles)) || (rc = b.alloc((void**)&d_bits, 8 * nwords)) ||
      (rc = b.alloc((void**)&d_recs, 8 * copyblk::kRunWords * n_need)) ||
      (rc = b.alloc((void**)&d_work, dev::copy_plan_work_bytes(n_need))) ||
      (rc = b.alloc((void**)&d_res, sizeof p_res + sizeof c_res)))
    return rc;
  // 1. the resident blocks, hashed where they lie
  CIR_HIP(hipMemcpyAsync(d_tab_off, tab_off.data(), 24 * nbuf, hipMemcpyHostToDevice, s));
  CIR_HIP(hipMemcpyAsync(d_tab_abs, tab_abs.data(), 24 * nbuf, hipMemcpyHostToDevice, s));
  CIR_HIP(dev::launch_mem_desc(d_tab_off, nbuf, bs, n_pool, d_off, d_len, s));
  if ((rc = hash_desc_ordered(d, reinterpret_cast<const uint8_t*>(arena), d_off, d_len, n_pool,
                              d_pool, s, im.ht)))
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
  // 3. the join, the plan, the copy
  CIR_HIP(dev::launch_join(d_need, n_need, d_pool, n_pool, d_table, slots, draw_seed(), d_match,
                           d_match + n_need, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t4 = Clock::now();
  const copyblk::Plan plan{d_match, n_need, d_need_runs, need_runs.size() / 4, d_dests, nfiles,
                           d_tab_abs,  nbuf,   n_pool,      bs};
  CIR_HIP(dev::launch_copy_plan(plan, d_bits, d_recs, n_need, d_work, d_res, s));
  // (the copy's grid is the host's to size: one synchronise learns the counts)
  CIR_HIP(hipMemcpyAsync(p_res, d_res, sizeof p_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  if (p_res[0] > n_need) return fail(CIR_EIO, "the copy plan counted more records than blocks");
  CIR_HIP(dev::launch_copy_runs(d_recs, p_res[0], p_res[1], d_res + copyblk::kPlanResFields, s));
  // 4. the memory bitmap and the copy's verdict
  CIR_HIP(hipMemcpyAsync(mem->data(), d_bits, 8 * nwords, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(c_res, d_res + copyblk::kPlanResFields, sizeof c_res,
                         hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  if (c_res[0]) return fail(CIR_EIO, "the copy kernel met a bad record");
  R.copied = p_res[0];
  R.bytes = p_res[2];
  R.hashed = n_pool;
  R.dropped = p_res[3];
  if (trace) {
    const double laps[5] = {ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, t3),
                            ms_between(t3, t4), ms_between(t4, Clock::now())};
    memcpy(R.laps, laps, sizeof laps);
    R.n_need = n_need;
    R.nbuf = nbuf;
  }
  return CIR_OK;
}

int reload_impl(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                uint32_t threads, void* const* d_data, size_t ndata, const void* const* d_have,
                const uint64_t* have_bytes, size_t nhave, void* stream, uint64_t** have_out,
                uint64_t* nblk_out, uint8_t** state_out, int32_t** errno_out, size_t* nfiles_out,
                uint64_t* stats) {
  if (!stats) return fail(CIR_EINVAL, "null pointer");
  for (int i = 0; i < CIR_RELOAD_STATS_FIELDS; ++i) stats[i] = 0;
  if (nhave && (!d_have || !have_bytes)) return fail(CIR_EINVAL, "null pointer");
  Resident R{d_data, d_have, have_bytes, nhave, stream};
  const ResidentFn fn = [&R](const stage::Layout& im, Device& d, std::vector<uint64_t>* mem) {
    return fill_from_memory(R, im, d, mem);
  };
  const bool disk = reload_from_disk();
  const auto t0 = Clock::now();
  const int rc = load_blocks_resident(ctx, dirfd, dir, index, len, threads, d_data, ndata, stream,
                                      disk ? nullptr : &fn, have_out, nblk_out, state_out,
                                      errno_out, nfiles_out, stats);
  if (rc) return rc;
  stats[12] = R.copied;
  stats[13] = R.bytes;
  stats[14] = R.hashed;
  for (size_t i = 0; i < *nfiles_out; ++i)
    if ((*state_out)[i] & CIR_FILE_RESIDENT) ++stats[15];
  stats[16] = R.dropped;
  if (trace_enabled()) {
    const double whole = ms_between(t0, Clock::now());
    const double step = R.laps[0] + R.laps[1] + R.laps[2] + R.laps[3] + R.laps[4];
    fprintf(stderr,
            "cir reload_blocks%s: %llu blocks against %llu resident blocks of %llu buffer(s); "
            "tables %.2f ms, resident hash %.2f ms, digest upload %.2f ms, join %.2f ms, plan + "
            "copy %.2f ms, index parse and pipeline %.2f ms, whole call %.2f ms; %llu blocks "
            "(%llu bytes) taken from memory, %llu dropped, %llu files resident\n",
            disk ? " (CIR_RELOAD=disk)" : "", (unsigned long long)R.n_need,
            (unsigned long long)R.hashed, (unsigned long long)R.nbuf, R.laps[0], R.laps[1],
            R.laps[2], R.laps[3], R.laps[4], whole - step, whole, (unsigned long long)R.copied,
            (unsigned long long)R.bytes, (unsigned long long)R.dropped,
            (unsigned long long)stats[15]);
  }
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" int cir_copy_runs(const uint64_t* runs, uint64_t nruns, uint64_t nunits,
                             uint64_t res[CIR_COPY_RES_FIELDS]) try {
  return cir::copy_host_impl(runs, nruns, nunits, res);
} CIR_CATCH_BOUNDARY

extern "C" int cir_copy_runs_dev(cir_ctx* ctx, const uint64_t* d_runs, uint64_t nruns,
                                 uint64_t nunits, uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::copy_dev_impl(d_runs, nruns, nunits, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_reload_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index,
                                 size_t len, uint32_t threads, void* const* d_data, size_t ndata,
                                 const void* const* d_have, const uint64_t* have_bytes,
                                 size_t nhave, void* stream, uint64_t** have_out,
                                 uint64_t* nblk_out, uint8_t** state_out, int32_t** errno_out,
                                 size_t* nfiles_out, uint64_t stats[CIR_RELOAD_STATS_FIELDS]) try {
  return cir::reload_impl(ctx, dirfd, dir, index, len, threads, d_data, ndata, d_have, have_bytes,
                          nhave, stream, have_out, nblk_out, state_out, errno_out, nfiles_out,
                          stats);
} CIR_CATCH_BOUNDARY
