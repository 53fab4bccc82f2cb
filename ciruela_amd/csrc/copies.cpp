// cir_file_copies: which files of a new image an older image holds unchanged
// at any path (a renamed directory, a moved or twice vendored file), matched
// by content on the device; cir_match_copies_dev, the device-resident join
// behind it.
//
// The reference matches by path only (scan_links,
// src/daemon/metadata/hardlink_sources.rs:121-146) and has no counterpart:
// below a renamed directory every file loses its hardlink and is copied
// instead.  The rule, the key of the table and the argument that the device's
// answer is the rule's are copies.hpp; the kernels are files.hip.  The device
// flow is cir_file_sources' (files.cpp), the steps of devcall.hpp's FileStage:
// the texts framed on the host and uploaded once, the count pass, the emit and
// decode passes with cir_index_files_dev's kernels and biases; then, here, the
// skip bitmap, the join, and the candidates' places downloaded with the
// verdicts and compacted by copies::compact.  Whatever
// the device cannot answer exactly is answered by the host rule here, which
// restates copies.hpp over dirsig::parse.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "copies.hpp"
#include "devcall.hpp"
#include "dirsig.hpp"
#include "files.hpp"
#include "idxscan.hpp"
#include "runtime.hpp"

namespace cir {
namespace {

static_assert(CIR_FILE_COPIES_STATS_FIELDS == 10, "the header's stats");

uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

int match_copies_dev_impl(const dev::FilesSide& need, const dev::FilesSide& pool,
                          const uint64_t* d_src_first, uint64_t nsrc, uint64_t bs,
                          const uint64_t* d_skip, const uint8_t* d_pool_verify, uint64_t seed,
                          void* d_work, uint64_t work_bytes, uint32_t* d_cand_src,
                          uint64_t* d_cand_file, uint64_t* d_cand_place, uint64_t* d_res,
                          void* stream) {
  for (const dev::FilesSide* s : {&need, &pool}) {
    if ((s->nfiles && !s->recs) || (s->nblocks && !s->digests))
      return fail(CIR_EINVAL, "null device pointer");
    if (addr(s->digests) & 15u) return fail(CIR_EINVAL, "digest arrays must be 16-byte aligned");
    if (addr(s->recs) & 7u) return fail(CIR_EINVAL, "file records must be 8-byte aligned");
    if (s->nblocks > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 blocks on a side");
  }
  if (!d_src_first || !d_work || !d_res ||
      (need.nfiles && (!d_cand_src || !d_cand_file || !d_cand_place)))
    return fail(CIR_EINVAL, "null device pointer");
  if (addr(d_pool_verify) & 15u) return fail(CIR_EINVAL, "digest arrays must be 16-byte aligned");
  if ((addr(d_src_first) | addr(d_skip) | addr(d_work) | addr(d_cand_file) | addr(d_cand_place) |
       addr(d_res)) & 7u)
    return fail(CIR_EINVAL,
                "d_src_first, d_skip, scratch, d_cand_file, d_cand_place and result must be 8-byte "
                "aligned");
  if (addr(d_cand_src) & 3u) return fail(CIR_EINVAL, "d_cand_src must be 4-byte aligned");
  if (bs == 0) return fail(CIR_EINVAL, "block_size is 0");
  if (pool.nfiles > files::kMaxPoolFiles) return fail(CIR_EINVAL, "more than 2^31-1 pool files");
  if (need.nfiles > files::kMaxNeedFiles) return fail(CIR_EINVAL, "more than 2^32-1 need files");
  if (nsrc > 0xFFFFFFFEull) return fail(CIR_EINVAL, "too many sources");
  if (work_bytes < dev::match_files_work_bytes(need.nfiles, pool.nfiles))
    return fail(CIR_EINVAL, "work_bytes is below cir_match_copies_work_bytes(...)");
  CIR_HIP(dev::launch_match_copies(need, pool, d_src_first, nsrc, bs, d_skip, d_pool_verify, seed,
                                   (uint64_t*)d_work, d_cand_src, d_cand_file, d_cand_place, d_res,
                                   (hipStream_t)stream));
  return CIR_OK;
}

// ---- the whole call ------------------------------------------------------------

struct Outs {
  uint64_t** file_out;
  uint32_t** src_out;
  uint64_t** src_file_out;
  uint64_t** path_off_out;
  uint8_t** paths_out;
  size_t* n_out;
  size_t* nskipped_out;
  uint64_t* stats;
};

using copies::Found;

int report(const Found& f, const Outs& o) {
  if (!f.give(o.file_out, o.src_out, o.src_file_out, o.path_off_out, o.paths_out))
    return fail(CIR_ENOMEM, "malloc");
  *o.n_out = f.file.size();
  return CIR_OK;
}

// The host rule: copies.hpp's over dirsig::parse.  A content is {exe, size,
// digests}; the map holds the first pool file of each, in pool order.
struct Content {
  const dirsig::Entry* e;
  bool operator==(const Content& b) const {
    return e->exe == b.e->exe && e->size == b.e->size && e->hashes == b.e->hashes;
  }
};
struct ContentHash {
  size_t operator()(const Content& c) const {
    uint64_t x = files::mix64(c.e->size, c.e->exe);
    const uint8_t* p = c.e->hashes.data();
    for (size_t i = 0, n = c.e->hashes.size() / 8; i < n; ++i) {
      uint64_t w;
      memcpy(&w, p + 8 * i, 8);
      x = files::mix64(x, w);
    }
    return (size_t)x;
  }
};

int file_copies_host(const uint8_t* index, size_t len, const uint8_t* const* src_index,
                     const size_t* src_len, size_t nsrc, const uint64_t* skip, const Outs& o) {
  dirsig::Index idx;
  std::string err;
  if (!dirsig::parse(index, len, &idx, &err))
    return idx.bad_hash_size ? fail(CIR_EHASHSIZE, "hash size is unsupported: " + err)
                             : fail(CIR_EPARSE, "error parsing index: " + err);
  struct Source {
    uint32_t ordinal;
    dirsig::Index idx;
  };
  std::vector<Source> sources;
  sources.reserve(nsrc);
  for (size_t j = 0; j < nsrc; ++j) {
    Source s;
    s.ordinal = (uint32_t)j;
    std::string serr;
    if (!src_index[j] || !dirsig::parse(src_index[j], src_len[j], &s.idx, &serr) ||
        s.idx.header.hash != idx.header.hash || s.idx.header.block_size != idx.header.block_size)
      continue;
    sources.push_back(std::move(s));
  }
  struct Place {
    uint32_t src;
    uint64_t file;
  };
  std::unordered_map<Content, Place, ContentHash> first;
  uint64_t pool_files = 0;
  for (const Source& s : sources) {
    uint64_t f = 0;
    for (const dirsig::Entry& en : s.idx.entries) {
      if (en.kind != dirsig::EntryKind::kFile) continue;
      if (en.size) first.emplace(Content{&en}, Place{s.ordinal, f});  // (the first stays)
      ++f;
    }
    pool_files += f;
  }
  Found found;
  uint64_t ordinal = 0, bytes = 0, left_out = 0, same = 0;
  for (const dirsig::Entry& en : idx.entries) {
    if (en.kind != dirsig::EntryKind::kFile) continue;
    const uint64_t i = ordinal++;
    if (copies::skipped(skip, i)) {
      ++left_out;
      continue;
    }
    if (en.size == 0) continue;
    const auto hit = first.find(Content{&en});
    if (hit == first.end()) continue;
    found.paths += hit->first.e->path;
    found.add(i, hit->second.src, hit->second.file);
    bytes += en.size;
    same += hit->first.e->path == en.path;
  }
  if (const int rc = report(found, o)) return rc;
  if (o.nskipped_out) *o.nskipped_out = nsrc - sources.size();
  o.stats[0] = ordinal;
  o.stats[1] = found.file.size();
  o.stats[2] = bytes;
  o.stats[3] = pool_files;
  o.stats[4] = sources.size();
  o.stats[8] = left_out;
  o.stats[9] = same;
  return CIR_OK;
}

// With a context: on its first device, under that device's lock.  Returns a
// CIR_* code, or kHostFlow with *why set and nothing reported.
int file_copies_dev(cir_ctx* ctx, const uint8_t* index, size_t len,
                    const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                    const uint64_t* skip, const Outs& o, bool trace, uint64_t* why) {
  if (ctx->devs.empty()) return fail(CIR_EINVAL, "context without a device");
  const auto t0 = Clock::now();
  // host memory that asynchronous copies read or write: declared before the call
  FileStage st;
  std::vector<uint32_t> cand;
  std::vector<uint64_t> cfile, cplace;
  std::vector<files::Rec> nrec;
  uint64_t m_res[files::kResFields] = {0, 0, 0, 0};
  TraceEvents<5> mev;
  int rc;
  if ((rc = st.frame(index, len, src_index, src_len, nsrc, why))) return rc;

  DeviceCall c(ctx);
  hipStream_t s = c.s;
  if ((rc = c.begin()) || (rc = st.count(c, trace, why))) return rc;
  const auto t1 = st.ts.t_bufs, t2 = st.ts.t_up, t3 = st.ts.t_counted;
  const uint64_t need_files = st.need_files(), pool_files = st.pool_files;
  const uint64_t skip_words = (need_files + 63) / 64;
  const size_t used = st.used;
  uint64_t* d_skip = nullptr;
  uint64_t* d_mwork = nullptr;
  uint32_t* d_csrc = nullptr;
  uint64_t* d_cfile = nullptr;
  uint64_t* d_cplace = nullptr;
  uint64_t* d_mres = nullptr;
  if ((rc = st.alloc(c)) || (skip && (rc = c.alloc(&d_skip, 8 * skip_words))) ||
      (rc = c.alloc(&d_mwork, dev::match_files_work_bytes(need_files, pool_files))) ||
      (rc = c.alloc(&d_csrc, 4 * need_files)) || (rc = c.alloc(&d_cfile, 8 * need_files)) ||
      (rc = c.alloc(&d_cplace, 16 * need_files)) || (rc = c.alloc(&d_mres, sizeof m_res)))
    return rc;
  if (trace && (rc = mev.create())) return rc;
  if ((rc = st.emit(c))) return rc;
  if (skip && skip_words)
    CIR_HIP(hipMemcpyAsync(d_skip, skip, 8 * skip_words, hipMemcpyHostToDevice, s));
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t4 = Clock::now();
  CIR_HIP(dev::launch_match_copies(st.need(), st.pool(), st.d_first, used, st.h.block_size,
                                   skip_words ? d_skip : nullptr, nullptr, draw_seed(), d_mwork,
                                   d_csrc, d_cfile, d_cplace, d_mres, s, trace ? mev.ev : nullptr));
  cand.resize(need_files);
  cfile.resize(need_files);
  cplace.resize(copies::kPlaceWords * need_files);
  nrec.resize(need_files);
  if ((rc = st.queue_verdicts(c))) return rc;
  CIR_HIP(hipMemcpyAsync(m_res, d_mres, sizeof m_res, hipMemcpyDeviceToHost, s));
  if (need_files) {
    CIR_HIP(hipMemcpyAsync(cand.data(), d_csrc, 4 * need_files, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipMemcpyAsync(cfile.data(), d_cfile, 8 * need_files, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipMemcpyAsync(cplace.data(), d_cplace, 16 * need_files, hipMemcpyDeviceToHost, s));
    // (the need records: where each entry's own path stands, for stats[9])
    CIR_HIP(hipMemcpyAsync(nrec.data(), st.d_nrec, 32 * need_files, hipMemcpyDeviceToHost, s));
  }
  if ((rc = st.ts.finish(c, false))) return rc;  // (the run tables stay on the device)
  const auto t5 = Clock::now();
  if ((rc = st.verdicts_ok(m_res[0] == files::kOk, why))) return rc;
  // compact, and decode each candidate's path from the source text held here
  Found found;
  found.reserve(m_res[1] <= need_files ? m_res[1] : 0);
  switch (copies::compact(cand.data(), cfile.data(), cplace.data(), nrec.data(), need_files,
                          st.placed().data(), used, skip, &found)) {
    case copies::kBadSource: return fail(CIR_EHIP, "candidate source out of range");
    case copies::kBadPlace: return fail(CIR_EHIP, "candidate place out of range");
    case copies::kCompacted: break;
  }
  if (found.file.size() != m_res[1]) return fail(CIR_EHIP, "candidate count mismatch");
  if ((rc = report(found, o))) return rc;
  const uint64_t n = m_res[1];
  if (o.nskipped_out) *o.nskipped_out = nsrc - used;
  o.stats[0] = need_files;
  o.stats[1] = n;
  o.stats[2] = m_res[2];
  o.stats[3] = pool_files;
  o.stats[4] = used;
  o.stats[5] = dev::join_table_slots(pool_files);
  o.stats[6] = 1;
  o.stats[7] = 0;
  o.stats[8] = found.left_out;
  o.stats[9] = found.same;
  if (trace) {
    const float lap[4] = {mev.lap(0), mev.lap(1), mev.lap(2), mev.lap(3)};
    fprintf(stderr,
            "cir file_copies: %llu files (%llu blocks) against %llu pool files (%llu blocks) of %zu "
            "source(s), device; frame and buffers %.2f ms, text upload %.2f ms (%llu bytes), count "
            "kernels %.2f ms, emit kernels %.2f ms, fold kernels %.3f ms, build kernel %.3f ms, "
            "probe kernel %.3f ms, verify kernel %.3f ms, join and download %.2f ms, compact and "
            "decode %.2f ms; %llu candidates, %llu skipped, %llu at their own path\n",
            (unsigned long long)need_files, (unsigned long long)st.need_blocks(),
            (unsigned long long)pool_files, (unsigned long long)st.pool_blocks, used,
            ms_between(t0, t1), ms_between(t1, t2), (unsigned long long)st.ts.text_bytes,
            ms_between(t2, t3), ms_between(t3, t4), lap[0], lap[1], lap[2], lap[3],
            ms_between(t4, t5), ms_between(t5, Clock::now()), (unsigned long long)n,
            (unsigned long long)found.left_out, (unsigned long long)found.same);
  }
  return CIR_OK;
}

int file_copies_impl(cir_ctx* ctx, const uint8_t* index, size_t len,
                     const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                     const uint64_t* skip, const Outs& o) {
  if (!index || !o.file_out || !o.src_out || !o.src_file_out || !o.path_off_out || !o.paths_out ||
      !o.n_out || !o.stats || (nsrc && (!src_index || !src_len)))
    return fail(CIR_EINVAL, "null pointer");
  *o.file_out = nullptr;
  *o.src_out = nullptr;
  *o.src_file_out = nullptr;
  *o.path_off_out = nullptr;
  *o.paths_out = nullptr;
  *o.n_out = 0;
  if (o.nskipped_out) *o.nskipped_out = 0;
  for (int i = 0; i < CIR_FILE_COPIES_STATS_FIELDS; ++i) o.stats[i] = 0;
  const bool trace = trace_enabled();
  uint64_t why = 0;
  if (ctx) {
    if (match_on_host()) {
      why = CIR_FILE_WHY_ENV;
    } else {
      const int rc =
          file_copies_dev(ctx, index, len, src_index, src_len, nsrc, skip, o, trace, &why);
      if (rc != kHostFlow) return rc;  // (nothing was reported yet)
    }
  }
  const auto t0 = Clock::now();
  const int rc = file_copies_host(index, len, src_index, src_len, nsrc, skip, o);
  if (rc) return rc;
  o.stats[7] = why;
  if (trace)
    fprintf(stderr,
            "cir file_copies: %llu files against %llu pool files of %llu source(s), host (why "
            "%llu); %.2f ms; %llu candidates, %llu skipped, %llu at their own path\n",
            (unsigned long long)o.stats[0], (unsigned long long)o.stats[3],
            (unsigned long long)o.stats[4], (unsigned long long)why, ms_between(t0, Clock::now()),
            (unsigned long long)o.stats[1], (unsigned long long)o.stats[8],
            (unsigned long long)o.stats[9]);
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" uint64_t cir_match_copies_work_bytes(uint64_t n_need_files, uint64_t n_pool_files) {
  if (n_pool_files > cir::files::kMaxPoolFiles || n_need_files > cir::files::kMaxNeedFiles) return 0;
  return cir::dev::match_files_work_bytes(n_need_files, n_pool_files);
}

extern "C" int cir_match_copies_dev(cir_ctx* ctx, const uint64_t* d_need_files,
                                    uint64_t n_need_files, const uint8_t* d_need_digests,
                                    uint64_t n_need_blocks, const uint64_t* d_pool_files,
                                    uint64_t n_pool_files, const uint8_t* d_pool_digests,
                                    uint64_t n_pool_blocks, const uint64_t* d_src_first,
                                    uint64_t nsrc, uint64_t block_size, const uint64_t* d_skip,
                                    const uint8_t* d_pool_verify, uint64_t seed, void* d_work,
                                    uint64_t work_bytes, uint32_t* d_cand_src,
                                    uint64_t* d_cand_file, uint64_t* d_cand_place, uint64_t* d_res,
                                    void* stream) try {
  (void)ctx;  // no scratch, no side streams
  const cir::dev::FilesSide need{nullptr, 0, d_need_files, n_need_files, d_need_digests,
                                 n_need_blocks};
  const cir::dev::FilesSide pool{nullptr, 0, d_pool_files, n_pool_files, d_pool_digests,
                                 n_pool_blocks};
  return cir::match_copies_dev_impl(need, pool, d_src_first, nsrc, block_size, d_skip,
                                    d_pool_verify, seed, d_work, work_bytes, d_cand_src,
                                    d_cand_file, d_cand_place, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_file_copies(cir_ctx* ctx, const uint8_t* index, size_t len,
                               const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                               const uint64_t* skip, uint64_t** file_out, uint32_t** src_out,
                               uint64_t** src_file_out, uint64_t** path_off_out,
                               uint8_t** paths_out, size_t* n_out, size_t* nskipped_out,
                               uint64_t stats[CIR_FILE_COPIES_STATS_FIELDS]) try {
  const cir::Outs o{file_out,  src_out, src_file_out, path_off_out,
                    paths_out, n_out,   nskipped_out, stats};
  return cir::file_copies_impl(ctx, index, len, src_index, src_len, nsrc, skip, o);
} CIR_CATCH_BOUNDARY
