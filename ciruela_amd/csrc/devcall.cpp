// The device flow of the whole-call entry points over index texts
// (devcall.hpp): the two parses, the file-level stage and the extent tail.
#include "devcall.hpp"

#include <string>

#include "files.hpp"
#include "sources.hpp"

namespace cir {

size_t TextSet::add(const uint8_t* p, size_t len, size_t body_off, size_t body_end) {
  Item t{};
  t.p = p;
  t.len = len;
  t.body_off = body_off;
  t.body_end = body_end;
  t.text_off = text_bytes;
  t.work_off = work_bytes;
  t.runs_off = run_recs;
  text_bytes += (len + 15) & ~(uint64_t)15;
  work_bytes += dev::idx_work_bytes(len);
  run_recs += len / idxscan::kMinRunLine;
  item.push_back(t);
  return item.size() - 1;
}

int TextSet::count(DeviceCall& c, uint64_t bs, size_t text_slack, bool trace) {
  const size_t k = item.size(), res_bytes = sizeof(uint64_t) * CIR_INDEX_RES_FIELDS * k;
  bs_ = bs;
  res.assign(CIR_INDEX_RES_FIELDS * k + 1, 0);
  if (k) {
    int rc;
    if ((rc = c.alloc(&d_text, text_bytes + text_slack)) || (rc = c.alloc(&d_work, work_bytes)) ||
        (rc = c.alloc(&d_res, res_bytes)) || (rc = c.alloc(&d_runs, 32 * run_recs)))
      return rc;
  }
  t_bufs = Clock::now();
  for (const Item& t : item)
    CIR_HIP(hipMemcpyAsync(d_text + t.text_off, t.p, t.len, hipMemcpyHostToDevice, c.s));
  if (trace) CIR_HIP(hipStreamSynchronize(c.s));
  t_up = Clock::now();
  for (size_t i = 0; i < k; ++i) {
    const Item& t = item[i];
    CIR_HIP(dev::launch_index_count(d_text + t.text_off, t.len, t.body_off, t.body_end, bs,
                                    t.len / idxscan::kTokenBytes, t.len / idxscan::kMinRunLine,
                                    (uint64_t*)(d_work + t.work_off),
                                    d_res + CIR_INDEX_RES_FIELDS * i, c.s));
  }
  if (k) CIR_HIP(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, c.s));
  CIR_HIP(hipStreamSynchronize(c.s));
  t_counted = Clock::now();
  for (size_t i = 0; i < k; ++i)
    memcpy(item[i].cnt, res.data() + CIR_INDEX_RES_FIELDS * i, sizeof item[i].cnt);
  return CIR_OK;
}

int TextSet::emit(DeviceCall& c, size_t i, uint8_t* d_digests, uint64_t max_blocks) {
  const Item& t = item[i];
  CIR_HIP(dev::launch_index_emit(d_text + t.text_off, t.len, t.body_off, t.body_end, bs_,
                                 d_digests, max_blocks, d_runs + 4 * t.runs_off,
                                 t.len / idxscan::kMinRunLine, (uint64_t*)(d_work + t.work_off),
                                 d_res + CIR_INDEX_RES_FIELDS * i, c.s));
  return CIR_OK;
}

int TextSet::finish(DeviceCall& c, bool with_runs) {
  if (!item.empty())
    CIR_HIP(hipMemcpyAsync(res.data(), d_res, sizeof(uint64_t) * CIR_INDEX_RES_FIELDS * item.size(),
                           hipMemcpyDeviceToHost, c.s));
  for (size_t i = 0; with_runs && i < item.size(); ++i) {
    Item& t = item[i];
    if (!counted_ok(i)) continue;
    t.runs.resize(t.cnt[2]);
    if (t.cnt[2])
      CIR_HIP(hipMemcpyAsync(t.runs.data(), d_runs + 4 * t.runs_off, 32 * t.cnt[2],
                             hipMemcpyDeviceToHost, c.s));
  }
  CIR_HIP(hipStreamSynchronize(c.s));
  return CIR_OK;
}

int FileStage::frame(const uint8_t* index, size_t len, const uint8_t* const* src_index,
                     const size_t* src_len, size_t nsrc, uint64_t* why) {
  if (nsrc > 0xFFFFFFFEull) return fail(CIR_EINVAL, "too many sources");
  std::string err;
  size_t body_off = 0, body_end = 0;
  *why = CIR_FILE_WHY_DECLINED;  // (a frame that does not parse is the host parser's to report)
  if (!dirsig::frame(index, len, &h, &body_off, &body_end, &err)) return kHostFlow;
  ts.add(index, len, body_off, body_end);
  tx.assign(1, Text{});
  bool fits = device_takes(len);
  fwork_bytes_ = dev::files_work_bytes(len);
  for (size_t j = 0; j < nsrc; ++j) {
    Text t;
    dirsig::Header sh;
    std::string serr;
    if (!src_index[j] ||
        !dirsig::frame(src_index[j], src_len[j], &sh, &body_off, &body_end, &serr) ||
        sh.hash != h.hash || sh.block_size != h.block_size)
      continue;  // skipped, and not uploaded
    ts.add(src_index[j], src_len[j], body_off, body_end);
    t.ordinal = (uint32_t)j;
    t.fwork_off = fwork_bytes_;
    fwork_bytes_ += dev::files_work_bytes(src_len[j]);
    fits = fits && device_takes(src_len[j]);
    tx.push_back(t);
  }
  *why = CIR_FILE_WHY_LIMIT;
  if (!fits) return kHostFlow;
  used = tx.size() - 1;
  f_res.assign(files::kResFields * tx.size(), 0);
  src_first.assign(used + 1, 0);
  return CIR_OK;
}

int FileStage::count(DeviceCall& c, bool trace, uint64_t* why) {
  // (the text buffer with 16 bytes to spare, as cir_index_files_dev's callers give it)
  if (const int rc = ts.count(c, h.block_size, 16, trace)) return rc;
  for (size_t k = 0; k < tx.size(); ++k) {
    const uint64_t* r = ts.item[k].cnt;
    if (r[0] != CIR_INDEX_OK) {
      *why = CIR_FILE_WHY_DECLINED;
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
  *why = CIR_FILE_WHY_LIMIT;
  if (pool_files > files::kMaxPoolFiles || need_files() > files::kMaxNeedFiles ||
      pool_blocks > 0xFFFFFFFFull)
    return kHostFlow;
  return CIR_OK;
}

// The digests and the records are written straight into the joins' buffers.
// The record kernels' small scratch and results are allocated here and not in
// front of the texts: with them first, case (c) of DESIGN 4.5h was 0.15 to 0.3
// ms slower (profiles/index_calls/ab.json, alloc_order).
int FileStage::alloc(DeviceCall& c) {
  int rc;
  (rc = c.alloc(&d_fwork, fwork_bytes_)) || (rc = c.alloc(&d_fres, 8 * f_res.size())) ||
      (rc = c.alloc(&d_ndig, 32 * need_blocks() + 32)) ||
      (rc = c.alloc(&d_pdig, 32 * pool_blocks + 32)) ||
      (rc = c.alloc(&d_nrec, 32 * need_files())) || (rc = c.alloc(&d_prec, 32 * pool_files)) ||
      (rc = c.alloc(&d_first, 8 * (used + 1)));
  return rc;
}

int FileStage::emit(DeviceCall& c) {
  CIR_HIP(hipMemcpyAsync(d_first, src_first.data(), 8 * (used + 1), hipMemcpyHostToDevice, c.s));
  uint64_t file_at = 0, block_at = 0;  // pool ordinals of the next source's first file and block
  for (size_t k = 0; k < tx.size(); ++k) {
    const Text& t = tx[k];
    const TextSet::Item& it = ts.item[k];
    uint8_t* dig = k ? d_pdig + 32 * block_at : d_ndig;
    uint64_t* rec = k ? d_prec + files::kFileWords * file_at : d_nrec;
    if (const int rc = ts.emit(c, k, dig, t.nblk)) return rc;
    CIR_HIP(dev::launch_index_files(ts.d_text + it.text_off, it.len, it.body_off, it.body_end,
                                    h.block_size, it.text_off, k ? block_at : 0, rec, t.nfiles,
                                    (uint64_t*)(d_fwork + t.fwork_off),
                                    d_fres + files::kResFields * k, c.s, false));
    if (k) {
      file_at += t.nfiles;
      block_at += t.nblk;
    }
  }
  return CIR_OK;
}

int FileStage::verdicts_ok(bool joins_ok, uint64_t* why) const {
  for (size_t k = 0; k < tx.size(); ++k) {
    const uint64_t* fr = f_res.data() + files::kResFields * k;
    if (ts.status(k) != CIR_INDEX_OK || fr[0] != CIR_INDEX_OK || fr[1] != tx[k].nfiles ||
        fr[2] != tx[k].nblk) {
      *why = CIR_FILE_WHY_DECLINED;
      return kHostFlow;
    }
  }
  if (!joins_ok) {
    *why = CIR_FILE_WHY_COLLISION;
    return kHostFlow;
  }
  return CIR_OK;
}

std::vector<copies::PlacedText> FileStage::placed() const {
  std::vector<copies::PlacedText> out;
  out.reserve(tx.size());
  for (size_t k = 0; k < tx.size(); ++k)
    out.push_back({ts.item[k].p, ts.item[k].len, ts.item[k].text_off, tx[k].nfiles, tx[k].ordinal});
  return out;
}

int parse_one_text(DeviceCall& c, const uint8_t* text, size_t len, uint64_t body_off,
                   uint64_t body_end, uint64_t bs, uint64_t res[CIR_INDEX_RES_FIELDS],
                   uint8_t** d_digests, uint64_t** d_runs) {
  const uint64_t cap_blocks = len / idxscan::kTokenBytes, cap_runs = len / idxscan::kMinRunLine;
  const size_t res_bytes = sizeof(uint64_t) * CIR_INDEX_RES_FIELDS;
  uint8_t* d_text = nullptr;
  uint64_t* d_work = nullptr;
  uint64_t* d_res = nullptr;
  int rc;
  if ((rc = c.alloc(&d_text, len + 16)) || (rc = c.alloc(d_digests, 32 * cap_blocks + 32)) ||
      (rc = c.alloc(d_runs, 32 * cap_runs + 32)) ||
      (rc = c.alloc(&d_work, dev::idx_work_bytes(len))) || (rc = c.alloc(&d_res, res_bytes)))
    return rc;
  CIR_HIP(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, c.s));
  CIR_HIP(dev::launch_index_digests(d_text, len, body_off, body_end, bs, *d_digests, cap_blocks,
                                    *d_runs, cap_runs, d_work, d_res, c.s));
  CIR_HIP(hipMemcpyAsync(res, d_res, res_bytes, hipMemcpyDeviceToHost, c.s));
  CIR_HIP(hipStreamSynchronize(c.s));
  return CIR_OK;
}

int device_extent_tail(DeviceCall& c, const dev::ExtentArgs& a, uint64_t count, uint64_t* d_work,
                       uint64_t* d_xres, const uint64_t* d_fetch, bool lap_emit, uint64_t** rec_out,
                       uint64_t** fetch_out, Clock::time_point* t_emit) {
  const uint64_t nwords = (a.n_need + 63) / 64;
  uint64_t* fetch = (uint64_t*)malloc(nwords * sizeof(uint64_t));
  uint64_t* rec = count ? (uint64_t*)malloc(count * sizeof(sources::Extent)) : nullptr;
  auto drop = [&](int code) {
    (void)hipStreamSynchronize(c.s);  // (no copy is in flight into what is freed)
    free(fetch);
    free(rec);
    return code;
  };
  if (!fetch || (count && !rec)) return drop(fail(CIR_ENOMEM, "malloc"));
  hipError_t e = hipSuccess;
  if (count) {
    uint64_t* d_ext = nullptr;
    const int rc = c.alloc(&d_ext, count * sizeof(sources::Extent));
    if (rc) return drop(rc);
    if ((e = dev::launch_extent_emit(a, d_ext, count, count, d_work, d_xres, c.s)) != hipSuccess)
      return drop(hip_fail(e, "launch_extent_emit"));
    if (lap_emit && (e = hipStreamSynchronize(c.s)) != hipSuccess) return drop(hip_fail(e, "emit"));
    *t_emit = Clock::now();
    if ((e = hipMemcpyAsync(rec, d_ext, count * sizeof(sources::Extent), hipMemcpyDeviceToHost,
                            c.s)) != hipSuccess)
      return drop(hip_fail(e, "download of the extents"));
  }
  if ((e = hipMemcpyAsync(fetch, d_fetch, 8 * nwords, hipMemcpyDeviceToHost, c.s)) != hipSuccess ||
      (e = hipStreamSynchronize(c.s)) != hipSuccess)
    return drop(hip_fail(e, "download of the fetch bitmap"));
  *rec_out = rec;
  *fetch_out = fetch;
  return CIR_OK;
}

}  // namespace cir
