// cir_index_frame, cir_index_digests_dev, cir_index_digests: an index's block
// digests as an array -- index text in, a flat digest list and a run record
// per non-empty file out.
//
// Reference: every consumer of an index there parses its text on a host
// thread (dir_signature::v1::Parser; ThreadedBlockReader::register_dir,
// src/blocks.rs:150-183; scan_links, src/daemon/metadata/hardlink_sources.rs:
// 107-153).  Here the text is parsed where the digests are used: the kernels
// are idxscan.hip, the rule which lines they take is idxscan.hpp, and a text
// they decline goes through dirsig::parse as before.  cir_index_digests' hold
// on the device and its one-shot parse are devcall.hpp's (DeviceCall,
// parse_one_text).
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "devcall.hpp"
#include "dirsig.hpp"
#include "idxscan.hpp"
#include "runtime.hpp"

namespace cir {
namespace {

static_assert(CIR_INDEX_RES_FIELDS == dev::kIdxResFields && CIR_INDEX_OK == dev::kIdxOk &&
                  CIR_INDEX_CAPACITY == dev::kIdxCapacity &&
                  CIR_INDEX_DECLINED == dev::kIdxDeclined,
              "the header's constants are the kernels'");
static_assert(sizeof(idxscan::Run) == 32, "a run record is four u64");

// The run records of a parsed index, hash_off found in its text: every entry
// is one body line, in order; a file line's first hash token follows its
// third token (name, type, size), however many spaces separate them.
void host_runs(const uint8_t* text, size_t len, const dirsig::Index& idx,
               std::vector<idxscan::Run>* runs, uint64_t* nblk, size_t* nfiles) {
  size_t p = (const uint8_t*)memchr(text, '\n', len) - text + 1;
  uint64_t first = 0, file = 0;
  for (const dirsig::Entry& e : idx.entries) {
    const size_t end = (const uint8_t*)memchr(text + p, '\n', len - p) - text;
    if (e.kind == dirsig::EntryKind::kFile) {
      if (!e.hashes.empty()) {
        size_t i = p + 2;
        for (int tok = 0; tok < 3; ++tok) {
          while (text[i] == ' ') ++i;
          while (i < end && text[i] != ' ') ++i;
        }
        runs->push_back(idxscan::Run{first, e.size, file, i});
        first += e.hashes.size() / 32;
      }
      ++file;
    }
    p = end + 1;
  }
  *nblk = first;
  *nfiles = file;
}

struct Arrays {
  uint8_t* digests = nullptr;
  uint64_t* runs = nullptr;
  ~Arrays() {
    free(digests);
    free(runs);
  }
};

// parse_one_text on ctx's first device, download.  *status = res[0]; on
// CIR_INDEX_OK the arrays are filled (malloc'd, null when empty).  out and res
// are the caller's, declared before the call: they outlive its drain.
int device_parse(cir_ctx* ctx, const uint8_t* index, size_t len, uint64_t body_off,
                 uint64_t body_end, uint64_t bs, Arrays* out, uint64_t res[CIR_INDEX_RES_FIELDS]) {
  DeviceCall c(ctx);
  uint8_t* d_dig = nullptr;
  uint64_t* d_runs = nullptr;
  int rc;
  if ((rc = c.begin()) ||
      (rc = parse_one_text(c, index, len, body_off, body_end, bs, res, &d_dig, &d_runs)))
    return rc;
  if (res[0] != CIR_INDEX_OK) return CIR_OK;
  if (res[3]) {
    out->digests = (uint8_t*)malloc(32 * res[3]);
    out->runs = (uint64_t*)malloc(32 * res[2]);
    if (!out->digests || !out->runs) return fail(CIR_ENOMEM, "malloc");
    CIR_HIP(hipMemcpyAsync(out->digests, d_dig, 32 * res[3], hipMemcpyDeviceToHost, c.s));
    CIR_HIP(hipMemcpyAsync(out->runs, d_runs, 32 * res[2], hipMemcpyDeviceToHost, c.s));
    CIR_HIP(hipStreamSynchronize(c.s));
  }
  return CIR_OK;
}

int index_digests_impl(cir_ctx* ctx, const uint8_t* index, size_t len, int* hash_type,
                       uint64_t* block_size, uint8_t** digests_out, uint64_t* nblk_out,
                       uint64_t** runs_out, size_t* nruns_out, size_t* nfiles_out,
                       uint64_t* stats) {
  if (!index || !hash_type || !block_size || !digests_out || !nblk_out || !runs_out ||
      !nruns_out || !nfiles_out || !stats)
    return fail(CIR_EINVAL, "null pointer");
  *hash_type = 0;
  *block_size = 0;
  *digests_out = nullptr;
  *nblk_out = 0;
  *runs_out = nullptr;
  *nruns_out = 0;
  *nfiles_out = 0;
  stats[0] = stats[1] = stats[3] = 0;
  stats[2] = ~0ull;
  if (ctx) {
    if (ctx->devs.empty()) return fail(CIR_EINVAL, "context without a device");
    dirsig::Header h;
    size_t body_off = 0, body_end = 0;
    std::string err;
    // (a frame that does not parse is the host parser's to report)
    if (device_takes(len) && dirsig::frame(index, len, &h, &body_off, &body_end, &err)) {
      Arrays a;
      uint64_t res[CIR_INDEX_RES_FIELDS];
      const int rc = device_parse(ctx, index, len, body_off, body_end, h.block_size, &a, res);
      if (rc) return rc;
      stats[3] = len;
      if (res[0] == CIR_INDEX_OK) {
        stats[0] = 1;
        *hash_type = (int)h.hash;
        *block_size = h.block_size;
        *digests_out = a.digests;
        *runs_out = a.runs;
        a.digests = nullptr;
        a.runs = nullptr;
        *nblk_out = res[3];
        *nruns_out = (size_t)res[2];
        *nfiles_out = (size_t)res[1];
        return CIR_OK;
      }
      stats[1] = 1;
      stats[2] = res[0] == CIR_INDEX_DECLINED ? res[4] : ~0ull;
    }
  }
  dirsig::Index idx;
  std::string err;
  if (!dirsig::parse(index, len, &idx, &err)) return parse_fail(idx.bad_hash_size, err);
  std::vector<idxscan::Run> runs;
  uint64_t nblk = 0;
  size_t nfiles = 0;
  host_runs(index, len, idx, &runs, &nblk, &nfiles);
  Arrays a;
  if (nblk) {
    a.digests = (uint8_t*)malloc(32 * nblk);
    a.runs = (uint64_t*)malloc(32 * runs.size());
    if (!a.digests || !a.runs) return fail(CIR_ENOMEM, "malloc");
    uint8_t* o = a.digests;
    for (const dirsig::Entry& e : idx.entries) {
      if (e.kind != dirsig::EntryKind::kFile || e.hashes.empty()) continue;
      memcpy(o, e.hashes.data(), e.hashes.size());
      o += e.hashes.size();
    }
    memcpy(a.runs, runs.data(), 32 * runs.size());
  }
  *hash_type = (int)idx.header.hash;
  *block_size = idx.header.block_size;
  *digests_out = a.digests;
  *runs_out = a.runs;
  a.digests = nullptr;
  a.runs = nullptr;
  *nblk_out = nblk;
  *nruns_out = runs.size();
  *nfiles_out = nfiles;
  return CIR_OK;
}

int index_digests_dev_impl(const uint8_t* d_text, uint64_t len, uint64_t body_off,
                           uint64_t body_end, uint64_t block_size, uint8_t* d_digests,
                           uint64_t cap_blocks, uint64_t* d_runs, uint64_t cap_runs, void* d_work,
                           uint64_t work_bytes, uint64_t* d_res, void* stream) {
  if ((len && !d_text) || (cap_blocks && !d_digests) || (cap_runs && !d_runs) || !d_work || !d_res)
    return fail(CIR_EINVAL, "null device pointer");
  if (reinterpret_cast<uintptr_t>(d_digests) & 15u)
    return fail(CIR_EINVAL, "the digest array must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_text) | reinterpret_cast<uintptr_t>(d_runs) |
       reinterpret_cast<uintptr_t>(d_work) | reinterpret_cast<uintptr_t>(d_res)) & 7u)
    return fail(CIR_EINVAL, "text, runs, scratch and result must be 8-byte aligned");
  if (body_off > body_end || body_end > len)
    return fail(CIR_EINVAL, "the body must lie inside the text");
  if (block_size == 0) return fail(CIR_EINVAL, "block_size is 0");
  if (len > dev::kIdxMaxLen) return fail(CIR_EINVAL, "an index text of more than 2^36 bytes");
  if (work_bytes < dev::idx_work_bytes(len))
    return fail(CIR_EINVAL, "work_bytes is below cir_index_work_bytes(len)");
  if (cap_blocks > 0xFFFFFFFFull) return fail(CIR_EINVAL, "cap_blocks of more than 2^32-1 blocks");
  CIR_HIP(dev::launch_index_digests(d_text, len, body_off, body_end, block_size, d_digests,
                                    cap_blocks, d_runs, cap_runs, (uint64_t*)d_work, d_res,
                                    (hipStream_t)stream));
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" uint64_t cir_index_work_bytes(uint64_t len) { return cir::dev::idx_work_bytes(len); }

extern "C" uint64_t cir_debug_index_tile_bytes(void) { return cir::dev::kIdxTile; }

extern "C" int cir_index_frame(const uint8_t* index, size_t len, int* hash_type,
                               uint64_t* block_size, uint64_t* body_off, uint64_t* body_end) try {
  if (!index || !hash_type || !block_size || !body_off || !body_end)
    return cir::fail(CIR_EINVAL, "null pointer");
  cir::dirsig::Header h;
  size_t b0 = 0, b1 = 0;
  std::string err;
  if (!cir::dirsig::frame(index, len, &h, &b0, &b1, &err))
    return cir::fail(CIR_EPARSE, "error parsing index: " + err);
  *hash_type = (int)h.hash;
  *block_size = h.block_size;
  *body_off = b0;
  *body_end = b1;
  return CIR_OK;
} CIR_CATCH_BOUNDARY

extern "C" int cir_index_digests_dev(cir_ctx* ctx, const uint8_t* d_text, uint64_t len,
                                     uint64_t body_off, uint64_t body_end, uint64_t block_size,
                                     uint8_t* d_digests, uint64_t cap_blocks, uint64_t* d_runs,
                                     uint64_t cap_runs, void* d_work, uint64_t work_bytes,
                                     uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::index_digests_dev_impl(d_text, len, body_off, body_end, block_size, d_digests,
                                     cap_blocks, d_runs, cap_runs, d_work, work_bytes, d_res,
                                     stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_index_digests(cir_ctx* ctx, const uint8_t* index, size_t len, int* hash_type,
                                 uint64_t* block_size, uint8_t** digests_out, uint64_t* nblk_out,
                                 uint64_t** runs_out, size_t* nruns_out, size_t* nfiles_out,
                                 uint64_t stats[CIR_INDEX_STATS_FIELDS]) try {
  return cir::index_digests_impl(ctx, index, len, hash_type, block_size, digests_out, nblk_out,
                                 runs_out, nruns_out, nfiles_out, stats);
} CIR_CATCH_BOUNDARY
