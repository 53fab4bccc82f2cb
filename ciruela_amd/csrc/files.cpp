// cir_file_sources: which files of a new image may be hardlinked from older
// images, matched on the device; cir_index_files_dev and cir_match_files_dev,
// the two device-resident calls behind it.
//
// Reference: scan_links (src/daemon/metadata/hardlink_sources.rs:107-153)
// walks the new index and up to 37 older ones on one host thread;
// cir_link_candidates (links.cpp) restates it with dirsig::parse and a hash
// map per source.  Here the texts are framed on the host and parsed where the
// digests already are: the records, the path hash and the fold are files.hpp,
// the kernels files.hip and idxscan.hip.  Whatever the device cannot answer
// exactly -- a text it declines, a collided fold, a count past a limit -- is
// answered by the host rule, unchanged.  The hold on the device, the two-pass
// parse of the texts, the file records and the policy -- any text declined
// sends the whole call to the host rule, with a reason -- are devcall.hpp's
// (DeviceCall, TextSet, FileStage), shared with copies.cpp and plan.cpp; the
// join, its buffers and the compaction of its answer are here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "devcall.hpp"
#include "dirsig.hpp"
#include "files.hpp"
#include "idxscan.hpp"
#include "links.hpp"
#include "runtime.hpp"

namespace cir {
namespace {

static_assert(CIR_FILE_WORDS == files::kFileWords && CIR_FILES_RES_FIELDS == files::kResFields &&
                  CIR_FILES_OK == files::kOk && CIR_FILES_COLLISION == files::kCollision,
              "the header's constants are the rule's");
static_assert(files::kMaxPoolFiles == dev::kJoinMaxPool, "the table holds u32 ordinals");
static_assert(sizeof(files::Rec) == 32, "a file record is four u64");

uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

int index_files_dev_impl(const uint8_t* d_text, uint64_t len, uint64_t body_off, uint64_t body_end,
                         uint64_t block_size, uint64_t off_bias, uint64_t block_bias,
                         uint64_t* d_files, uint64_t cap_files, void* d_work, uint64_t work_bytes,
                         uint64_t* d_res, void* stream) {
  if ((len && !d_text) || (cap_files && !d_files) || !d_work || !d_res)
    return fail(CIR_EINVAL, "null device pointer");
  if ((addr(d_text) | addr(d_files) | addr(d_work) | addr(d_res)) & 7u)
    return fail(CIR_EINVAL, "text, records, scratch and result must be 8-byte aligned");
  if (body_off > body_end || body_end > len)
    return fail(CIR_EINVAL, "the body must lie inside the text");
  if (block_size == 0) return fail(CIR_EINVAL, "block_size is 0");
  if (len > dev::kIdxMaxLen) return fail(CIR_EINVAL, "an index text of more than 2^36 bytes");
  if (work_bytes < dev::files_work_bytes(len))
    return fail(CIR_EINVAL, "work_bytes is below cir_index_files_work_bytes(len)");
  if (cap_files > (1ull << 58)) return fail(CIR_EINVAL, "cap_files x 32 bytes passes 2^63");
  CIR_HIP(dev::launch_index_files(d_text, len, body_off, body_end, block_size, off_bias,
                                  block_bias, d_files, cap_files, (uint64_t*)d_work, d_res,
                                  (hipStream_t)stream));
  return CIR_OK;
}

int match_files_dev_impl(const dev::FilesSide& need, const dev::FilesSide& pool,
                         const uint64_t* d_src_first, uint64_t nsrc, uint64_t bs,
                         const uint8_t* d_pool_verify, uint64_t seed, void* d_work,
                         uint64_t work_bytes, uint32_t* d_cand_src, uint64_t* d_cand_file,
                         uint64_t* d_res, void* stream) {
  for (const dev::FilesSide* s : {&need, &pool}) {
    if ((s->nfiles && (!s->recs || !s->text)) || (s->nblocks && !s->digests))
      return fail(CIR_EINVAL, "null device pointer");
    if (addr(s->digests) & 15u) return fail(CIR_EINVAL, "digest arrays must be 16-byte aligned");
    if (addr(s->recs) & 7u) return fail(CIR_EINVAL, "file records must be 8-byte aligned");
    if (s->nblocks > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 blocks on a side");
  }
  if (!d_src_first || !d_work || !d_res || (need.nfiles && (!d_cand_src || !d_cand_file)))
    return fail(CIR_EINVAL, "null device pointer");
  if (addr(d_pool_verify) & 15u) return fail(CIR_EINVAL, "digest arrays must be 16-byte aligned");
  if ((addr(d_src_first) | addr(d_work) | addr(d_cand_file) | addr(d_res)) & 7u)
    return fail(CIR_EINVAL, "d_src_first, scratch, d_cand_file and result must be 8-byte aligned");
  if (addr(d_cand_src) & 3u) return fail(CIR_EINVAL, "d_cand_src must be 4-byte aligned");
  if (bs == 0) return fail(CIR_EINVAL, "block_size is 0");
  if (pool.nfiles > files::kMaxPoolFiles) return fail(CIR_EINVAL, "more than 2^31-1 pool files");
  if (need.nfiles > files::kMaxNeedFiles) return fail(CIR_EINVAL, "more than 2^32-1 need files");
  if (nsrc > 0xFFFFFFFEull) return fail(CIR_EINVAL, "too many sources");
  if (work_bytes < dev::match_files_work_bytes(need.nfiles, pool.nfiles))
    return fail(CIR_EINVAL, "work_bytes is below cir_match_files_work_bytes(...)");
  CIR_HIP(dev::launch_match_files(need, pool, d_src_first, nsrc, bs, d_pool_verify, seed,
                                  (uint64_t*)d_work, d_cand_src, d_cand_file, d_res,
                                  (hipStream_t)stream));
  return CIR_OK;
}

// ---- the whole call ------------------------------------------------------------

struct Outs {
  uint64_t** file_out;
  uint32_t** src_out;
  size_t* n_out;
  size_t* nskipped_out;
  uint64_t* stats;
};

// With a context: on its first device, under that device's lock.  Returns a
// CIR_* code, or kHostFlow with *why set and nothing reported.
int file_sources_dev(cir_ctx* ctx, const uint8_t* index, size_t len,
                     const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                     const Outs& o, bool trace, uint64_t* why) {
  if (ctx->devs.empty()) return fail(CIR_EINVAL, "context without a device");
  const auto t0 = Clock::now();
  // host memory that asynchronous copies read or write: declared before the call
  FileStage st;
  std::vector<uint32_t> cand;
  uint64_t m_res[files::kResFields] = {0, 0, 0, 0};
  TraceEvents<5> mev;
  int rc;
  if ((rc = st.frame(index, len, src_index, src_len, nsrc, why))) return rc;

  DeviceCall c(ctx);
  hipStream_t s = c.s;
  if ((rc = c.begin()) || (rc = st.count(c, trace, why))) return rc;
  const auto t1 = st.ts.t_bufs, t2 = st.ts.t_up, t3 = st.ts.t_counted;
  const uint64_t need_files = st.need_files(), pool_files = st.pool_files;
  const size_t used = st.used;
  uint64_t* d_mwork = nullptr;
  uint32_t* d_csrc = nullptr;
  uint64_t* d_cfile = nullptr;
  uint64_t* d_mres = nullptr;
  if ((rc = st.alloc(c)) ||
      (rc = c.alloc(&d_mwork, dev::match_files_work_bytes(need_files, pool_files))) ||
      (rc = c.alloc(&d_csrc, 4 * need_files)) || (rc = c.alloc(&d_cfile, 8 * need_files)) ||
      (rc = c.alloc(&d_mres, sizeof m_res)))
    return rc;
  if (trace && (rc = mev.create())) return rc;
  if ((rc = st.emit(c))) return rc;
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t4 = Clock::now();
  CIR_HIP(dev::launch_match_files(st.need(), st.pool(), st.d_first, used, st.h.block_size, nullptr,
                                  draw_seed(), d_mwork, d_csrc, d_cfile, d_mres, s,
                                  trace ? mev.ev : nullptr));
  cand.resize(need_files);
  if ((rc = st.queue_verdicts(c))) return rc;
  CIR_HIP(hipMemcpyAsync(m_res, d_mres, sizeof m_res, hipMemcpyDeviceToHost, s));
  if (need_files)
    CIR_HIP(hipMemcpyAsync(cand.data(), d_csrc, 4 * need_files, hipMemcpyDeviceToHost, s));
  if ((rc = st.ts.finish(c, false))) return rc;  // (the run tables stay on the device)
  const auto t5 = Clock::now();
  if ((rc = st.verdicts_ok(m_res[0] == files::kOk, why))) return rc;
  const uint64_t n = m_res[1];
  uint64_t* fo = nullptr;
  uint32_t* so = nullptr;
  if (n) {
    fo = (uint64_t*)malloc(n * sizeof(uint64_t));
    so = (uint32_t*)malloc(n * sizeof(uint32_t));
    uint64_t at = 0;
    if (fo && so)
      for (uint64_t i = 0; i < need_files; ++i)
        if (cand[i] != files::kNoSrc && cand[i] < used && at < n) {
          fo[at] = i;
          so[at++] = st.tx[1 + cand[i]].ordinal;
        }
    if (!fo || !so || at != n) {
      free(fo);
      free(so);
      return !fo || !so ? fail(CIR_ENOMEM, "malloc") : fail(CIR_EHIP, "candidate count mismatch");
    }
  }
  *o.file_out = fo;
  *o.src_out = so;
  *o.n_out = n;
  if (o.nskipped_out) *o.nskipped_out = nsrc - used;
  o.stats[0] = need_files;
  o.stats[1] = n;
  o.stats[2] = m_res[2];
  o.stats[3] = pool_files;
  o.stats[4] = used;
  o.stats[5] = dev::join_table_slots(pool_files);
  o.stats[6] = 1;
  o.stats[7] = 0;
  if (trace) {
    const float lap[4] = {mev.lap(0), mev.lap(1), mev.lap(2), mev.lap(3)};
    fprintf(stderr,
            "cir file_sources: %llu files (%llu blocks) against %llu pool files (%llu blocks) of %zu "
            "source(s), device; frame and buffers %.2f ms, text upload %.2f ms (%llu bytes), count "
            "kernels %.2f ms, emit kernels %.2f ms, fold kernels %.3f ms, build kernel %.3f ms, "
            "probe kernel %.3f ms, verify kernel %.3f ms, join and download %.2f ms, compact %.2f "
            "ms; %llu candidates\n",
            (unsigned long long)need_files, (unsigned long long)st.need_blocks(),
            (unsigned long long)pool_files, (unsigned long long)st.pool_blocks, used,
            ms_between(t0, t1), ms_between(t1, t2), (unsigned long long)st.ts.text_bytes,
            ms_between(t2, t3), ms_between(t3, t4), lap[0], lap[1], lap[2], lap[3],
            ms_between(t4, t5), ms_between(t5, Clock::now()), (unsigned long long)n);
  }
  return CIR_OK;
}

int file_sources_impl(cir_ctx* ctx, const uint8_t* index, size_t len,
                      const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                      const Outs& o) {
  if (!index || !o.file_out || !o.src_out || !o.n_out || !o.stats ||
      (nsrc && (!src_index || !src_len)))
    return fail(CIR_EINVAL, "null pointer");
  *o.file_out = nullptr;
  *o.src_out = nullptr;
  *o.n_out = 0;
  if (o.nskipped_out) *o.nskipped_out = 0;
  for (int i = 0; i < CIR_FILE_SOURCES_STATS_FIELDS; ++i) o.stats[i] = 0;
  const bool trace = trace_enabled();
  uint64_t why = 0;
  if (ctx) {
    if (match_on_host()) {
      why = CIR_FILE_WHY_ENV;
    } else {
      const int rc = file_sources_dev(ctx, index, len, src_index, src_len, nsrc, o, trace, &why);
      if (rc != kHostFlow) return rc;  // (nothing was reported yet)
    }
  }
  const auto t0 = Clock::now();
  uint64_t counts[5] = {0, 0, 0, 0, 0};
  const int rc = candidates_impl(index, len, src_index, src_len, nsrc, o.file_out, o.src_out,
                                 o.n_out, o.nskipped_out, counts);
  if (rc) return rc;
  for (int i = 0; i < 5; ++i) o.stats[i] = counts[i];
  o.stats[7] = why;
  if (trace)
    fprintf(stderr,
            "cir file_sources: %llu files against %llu pool files of %llu source(s), host (why %llu); "
            "%.2f ms; %llu candidates\n",
            (unsigned long long)counts[0], (unsigned long long)counts[3],
            (unsigned long long)counts[4], (unsigned long long)why, ms_between(t0, Clock::now()),
            (unsigned long long)counts[1]);
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" uint64_t cir_index_files_work_bytes(uint64_t len) {
  return cir::dev::files_work_bytes(len);
}

extern "C" uint64_t cir_match_files_work_bytes(uint64_t n_need_files, uint64_t n_pool_files) {
  if (n_pool_files > cir::files::kMaxPoolFiles || n_need_files > cir::files::kMaxNeedFiles) return 0;
  return cir::dev::match_files_work_bytes(n_need_files, n_pool_files);
}

extern "C" int cir_index_files_dev(cir_ctx* ctx, const uint8_t* d_text, uint64_t len,
                                   uint64_t body_off, uint64_t body_end, uint64_t block_size,
                                   uint64_t off_bias, uint64_t block_bias, uint64_t* d_files,
                                   uint64_t cap_files, void* d_work, uint64_t work_bytes,
                                   uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::index_files_dev_impl(d_text, len, body_off, body_end, block_size, off_bias,
                                   block_bias, d_files, cap_files, d_work, work_bytes, d_res,
                                   stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_match_files_dev(cir_ctx* ctx, const uint8_t* d_need_text, uint64_t need_text_len,
                                   const uint64_t* d_need_files, uint64_t n_need_files,
                                   const uint8_t* d_need_digests, uint64_t n_need_blocks,
                                   const uint8_t* d_pool_text, uint64_t pool_text_len,
                                   const uint64_t* d_pool_files, uint64_t n_pool_files,
                                   const uint8_t* d_pool_digests, uint64_t n_pool_blocks,
                                   const uint64_t* d_src_first, uint64_t nsrc, uint64_t block_size,
                                   const uint8_t* d_pool_verify, uint64_t seed, void* d_work,
                                   uint64_t work_bytes, uint32_t* d_cand_src,
                                   uint64_t* d_cand_file, uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch, no side streams
  const cir::dev::FilesSide need{d_need_text, need_text_len, d_need_files,
                                 n_need_files, d_need_digests, n_need_blocks};
  const cir::dev::FilesSide pool{d_pool_text, pool_text_len, d_pool_files,
                                 n_pool_files, d_pool_digests, n_pool_blocks};
  return cir::match_files_dev_impl(need, pool, d_src_first, nsrc, block_size, d_pool_verify, seed,
                                   d_work, work_bytes, d_cand_src, d_cand_file, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_file_sources(cir_ctx* ctx, const uint8_t* index, size_t len,
                                const uint8_t* const* src_index, const size_t* src_len,
                                size_t nsrc, uint64_t** file_out, uint32_t** src_out,
                                size_t* n_out, size_t* nskipped_out,
                                uint64_t stats[CIR_FILE_SOURCES_STATS_FIELDS]) try {
  const cir::Outs o{file_out, src_out, n_out, nskipped_out, stats};
  return cir::file_sources_impl(ctx, index, len, src_index, src_len, nsrc, o);
} CIR_CATCH_BOUNDARY
