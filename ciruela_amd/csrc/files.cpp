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
// answered by the host rule, unchanged.  The hold on the device and the
// two-pass parse of the texts are devcall.hpp's (DeviceCall, TextSet); the
// file records' scratch and results, and the policy -- any text declined sends
// the whole call to the host rule, with a reason -- are here.
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

enum Why : uint64_t { kWhyNone = 0, kWhyDeclined = 1, kWhyCollision = 2, kWhyLimit = 3, kWhyEnv = 4 };
static_assert(CIR_FILE_WHY_DECLINED == kWhyDeclined && CIR_FILE_WHY_COLLISION == kWhyCollision &&
                  CIR_FILE_WHY_LIMIT == kWhyLimit && CIR_FILE_WHY_ENV == kWhyEnv,
              "the header's reasons");

constexpr int kHostFlow = 2;  // (no CIR_* code is positive) the host rule decides this call

// CIR_LINKS_MATCH=host, read per call: cir_file_sources with a context answers
// with the host rule (A/B measurement).
bool match_on_host() {
  const char* v = getenv("CIR_LINKS_MATCH");
  return v && strcmp(v, "host") == 0;
}

struct Outs {
  uint64_t** file_out;
  uint32_t** src_out;
  size_t* n_out;
  size_t* nskipped_out;
  uint64_t* stats;
};

// One text of the call on the device, beside its TextSet item.
struct Text {
  uint32_t ordinal = 0;  // the source's, as the caller counts
  uint64_t fwork_off = 0;
  uint64_t nfiles = 0, nblk = 0;
};

// With a context: on its first device, under that device's lock.  Returns a
// CIR_* code, or kHostFlow with *why set and nothing reported.
int file_sources_dev(cir_ctx* ctx, const uint8_t* index, size_t len,
                     const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                     const Outs& o, bool trace, uint64_t* why) {
  if (ctx->devs.empty()) return fail(CIR_EINVAL, "context without a device");
  if (nsrc > 0xFFFFFFFEull) return fail(CIR_EINVAL, "too many sources");
  const auto t0 = Clock::now();
  dirsig::Header h;
  std::string err;
  // host memory that asynchronous copies read or write: declared before the call
  TextSet ts;  // the new index, then the sources that take part
  std::vector<Text> tx(1);  // (tx[k] goes with ts.item[k])
  size_t body_off = 0, body_end = 0;
  *why = kWhyDeclined;  // (a frame that does not parse is the host parser's to report)
  if (!dirsig::frame(index, len, &h, &body_off, &body_end, &err)) return kHostFlow;
  ts.add(index, len, body_off, body_end);
  bool fits = device_takes(len);
  uint64_t fwork_bytes = dev::files_work_bytes(len);
  for (size_t j = 0; j < nsrc; ++j) {
    Text t;
    dirsig::Header sh;
    std::string serr;
    if (!src_index[j] || !dirsig::frame(src_index[j], src_len[j], &sh, &body_off, &body_end, &serr) ||
        sh.hash != h.hash || sh.block_size != h.block_size)
      continue;  // skipped, and not uploaded
    ts.add(src_index[j], src_len[j], body_off, body_end);
    t.ordinal = (uint32_t)j;
    t.fwork_off = fwork_bytes;
    fwork_bytes += dev::files_work_bytes(src_len[j]);
    fits = fits && device_takes(src_len[j]);
    tx.push_back(t);
  }
  *why = kWhyLimit;
  if (!fits) return kHostFlow;
  const uint64_t bs = h.block_size, text_bytes = ts.text_bytes;
  const size_t nt = tx.size(), used = nt - 1;
  std::vector<uint64_t> f_res(files::kResFields * nt);
  std::vector<uint64_t> src_first(used + 1);
  std::vector<uint32_t> cand;
  uint64_t m_res[files::kResFields] = {0, 0, 0, 0};
  TraceEvents<5> mev;

  DeviceCall c(ctx);
  hipStream_t s = c.s;
  uint8_t* d_fwork = nullptr;
  uint64_t* d_fres = nullptr;
  int rc;
  // (the text buffer with 16 bytes to spare, as cir_index_files_dev's callers give it)
  if ((rc = c.begin()) || (rc = ts.count(c, bs, 16, trace))) return rc;
  const auto t1 = ts.t_bufs, t2 = ts.t_up, t3 = ts.t_counted;
  uint8_t* const d_text = ts.d_text;
  uint64_t pool_files = 0, pool_blocks = 0;
  for (size_t k = 0; k < nt; ++k) {
    const uint64_t* r = ts.item[k].cnt;
    if (r[0] != CIR_INDEX_OK) {
      *why = kWhyDeclined;
      return kHostFlow;
    }
    tx[k].nfiles = r[1];
    tx[k].nblk = r[3];
    if (k) {
      src_first[k - 1] = pool_files;
      pool_files += r[1];
      pool_blocks += r[3];
    }
  }
  src_first[used] = pool_files;
  const uint64_t need_files = tx[0].nfiles, need_blocks = tx[0].nblk;
  if (pool_files > files::kMaxPoolFiles || need_files > files::kMaxNeedFiles ||
      pool_blocks > 0xFFFFFFFFull)
    return kHostFlow;  // (*why is kWhyLimit)
  // the join's buffers; the digests and the records are written straight into them.
  // The record kernels' small scratch and results are allocated here and not
  // in front of the texts: with them first, case (c) of DESIGN 4.5h was 0.15 to
  // 0.3 ms slower (profiles/index_calls/ab.json, alloc_order).
  uint8_t* d_ndig = nullptr;
  uint8_t* d_pdig = nullptr;
  uint64_t* d_nrec = nullptr;
  uint64_t* d_prec = nullptr;
  uint64_t* d_first = nullptr;
  uint64_t* d_mwork = nullptr;
  uint32_t* d_csrc = nullptr;
  uint64_t* d_cfile = nullptr;
  uint64_t* d_mres = nullptr;
  if ((rc = c.alloc(&d_fwork, fwork_bytes)) || (rc = c.alloc(&d_fres, 8 * f_res.size())) ||
      (rc = c.alloc(&d_ndig, 32 * need_blocks + 32)) ||
      (rc = c.alloc(&d_pdig, 32 * pool_blocks + 32)) ||
      (rc = c.alloc(&d_nrec, 32 * need_files)) || (rc = c.alloc(&d_prec, 32 * pool_files)) ||
      (rc = c.alloc(&d_first, 8 * (used + 1))) ||
      (rc = c.alloc(&d_mwork, dev::match_files_work_bytes(need_files, pool_files))) ||
      (rc = c.alloc(&d_csrc, 4 * need_files)) || (rc = c.alloc(&d_cfile, 8 * need_files)) ||
      (rc = c.alloc(&d_mres, sizeof m_res)))
    return rc;
  if (trace && (rc = mev.create())) return rc;
  CIR_HIP(hipMemcpyAsync(d_first, src_first.data(), 8 * (used + 1), hipMemcpyHostToDevice, s));
  uint64_t file_at = 0, block_at = 0;  // pool ordinals of the next source's first file and block
  for (size_t k = 0; k < nt; ++k) {
    const Text& t = tx[k];
    const TextSet::Item& it = ts.item[k];
    uint8_t* dig = k ? d_pdig + 32 * block_at : d_ndig;
    uint64_t* rec = k ? d_prec + files::kFileWords * file_at : d_nrec;
    if ((rc = ts.emit(c, k, dig, t.nblk))) return rc;
    CIR_HIP(dev::launch_index_files(d_text + it.text_off, it.len, it.body_off, it.body_end, bs,
                                    it.text_off, k ? block_at : 0, rec, t.nfiles,
                                    (uint64_t*)(d_fwork + t.fwork_off),
                                    d_fres + files::kResFields * k, s, false));
    if (k) {
      file_at += t.nfiles;
      block_at += t.nblk;
    }
  }
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t4 = Clock::now();
  const dev::FilesSide need{d_text, text_bytes, d_nrec, need_files, d_ndig, need_blocks};
  const dev::FilesSide pool{d_text, text_bytes, d_prec, pool_files, d_pdig, pool_blocks};
  CIR_HIP(dev::launch_match_files(need, pool, d_first, used, bs, nullptr, draw_seed(), d_mwork,
                                  d_csrc, d_cfile, d_mres, s, trace ? mev.ev : nullptr));
  cand.resize(need_files);
  CIR_HIP(hipMemcpyAsync(f_res.data(), d_fres, 8 * f_res.size(), hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(m_res, d_mres, sizeof m_res, hipMemcpyDeviceToHost, s));
  if (need_files)
    CIR_HIP(hipMemcpyAsync(cand.data(), d_csrc, 4 * need_files, hipMemcpyDeviceToHost, s));
  if ((rc = ts.finish(c, false))) return rc;  // (the run tables stay on the device)
  const auto t5 = Clock::now();
  // every verdict is in: a bad token shows only after the decode pass
  for (size_t k = 0; k < nt; ++k) {
    const uint64_t* fr = f_res.data() + files::kResFields * k;
    if (ts.status(k) != CIR_INDEX_OK || fr[0] != CIR_INDEX_OK ||
        fr[1] != tx[k].nfiles || fr[2] != tx[k].nblk) {
      *why = kWhyDeclined;
      return kHostFlow;
    }
  }
  if (m_res[0] != files::kOk) {
    *why = kWhyCollision;
    return kHostFlow;
  }
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
          so[at++] = tx[1 + cand[i]].ordinal;
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
  o.stats[7] = kWhyNone;
  if (trace) {
    const float lap[4] = {mev.lap(0), mev.lap(1), mev.lap(2), mev.lap(3)};
    fprintf(stderr,
            "cir file_sources: %llu files (%llu blocks) against %llu pool files (%llu blocks) of %zu "
            "source(s), device; frame and buffers %.2f ms, text upload %.2f ms (%llu bytes), count "
            "kernels %.2f ms, emit kernels %.2f ms, fold kernels %.3f ms, build kernel %.3f ms, "
            "probe kernel %.3f ms, verify kernel %.3f ms, join and download %.2f ms, compact %.2f "
            "ms; %llu candidates\n",
            (unsigned long long)need_files, (unsigned long long)need_blocks,
            (unsigned long long)pool_files, (unsigned long long)pool_blocks, used,
            ms_between(t0, t1), ms_between(t1, t2), (unsigned long long)text_bytes,
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
  uint64_t why = kWhyNone;
  if (ctx) {
    if (match_on_host()) {
      why = kWhyEnv;
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
