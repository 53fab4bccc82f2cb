// cir_index_emit_layout, cir_index_emit_tables, cir_index_emit,
// cir_index_emit_dev, cir_index_memory_dev: a DIRSIGNATURE.v1 index and its
// ImageId for files that are not in a file system -- a flat list of paths with
// host digests (cir_index_emit) or with their bytes in device memory
// (cir_index_memory_dev).  The rule is emit.hpp, the kernels are emit.hip.
//
// Reference: an index comes from a directory scan (dir_signature::v1::scan,
// src/client/sync/uploads.rs:49-59) or from a parsed index re-emitted
// (MutableIndex::to_raw_data, src/cluster/download.rs:266-319); bytes that a
// process holds in device memory reach neither without a trip through a file
// system.  The text here is the scan's for a directory holding the same files.
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "blake2b_host.hpp"
#include "devcall.hpp"
#include "dirsig.hpp"
#include "emit.hpp"
#include "memindex.hpp"
#include "runtime.hpp"
#include "sha512_host.hpp"

namespace cir {
namespace {

static_assert(CIR_EMIT_PIECE_WORDS == emit::kPieceWords && CIR_EMIT_RES_FIELDS == dev::kEmitResFields,
              "the header's constants are the rule's and the kernels'");

// CIR_EMIT=host, read per call: cir_index_memory_dev hashes on the device,
// downloads the digests and emits on the host (A/B measurement).
bool emit_on_host() {
  const char* v = getenv("CIR_EMIT");
  return v && strcmp(v, "host") == 0;
}

std::string header_line(const dirsig::Header& h) {
  return std::string("DIRSIGNATURE.v1 ") + dirsig::hash_type_name(h.hash) +
         " block_size=" + std::to_string(h.block_size) + "\n";
}

// The index buffer of a body of body_len bytes: header, room for the body in
// whole 16-byte lanes, and the footer line, which overwrites the padding.
uint8_t* index_buffer(const std::string& header, uint64_t body_len, size_t* cap) {
  *cap = header.size() + (size_t)emit::round_up16(body_len) + 65;
  uint8_t* buf = (uint8_t*)malloc(*cap);
  if (buf) memcpy(buf, header.data(), header.size());
  return buf;
}

// Footer = H(body); appends its line.  Returns the index length.
size_t finish_index(uint8_t* buf, size_t hlen, uint64_t body_len, const dirsig::Header& h,
                    uint8_t image_id[32]) {
  uint8_t id[32];
  if (h.hash == dirsig::HashType::kSha512_256) {
    host::Sha512_256 f;
    f.update(buf + hlen, (size_t)body_len);
    f.final(id);
  } else {
    host::Blake2b256 f;
    f.update(buf + hlen, (size_t)body_len);
    f.final(id);
  }
  const std::string hex = dirsig::to_hex(id, 32);
  memcpy(buf + hlen + body_len, hex.data(), 64);
  buf[hlen + body_len + 64] = '\n';
  if (image_id) memcpy(image_id, id, 32);
  return hlen + (size_t)body_len + 65;
}

int emit_layout_impl(uint64_t bs, const uint8_t* paths, const uint64_t* path_off,
                     const uint64_t* sizes, const uint8_t* exe, size_t nfiles,
                     uint64_t** pieces_out, size_t* npieces, uint8_t** lits_out, size_t* lits_len,
                     uint64_t* first_block_out, uint64_t* nblocks, uint64_t* body_len) {
  if (!pieces_out || !npieces || !lits_out || !lits_len || !nblocks || !body_len)
    return fail(CIR_EINVAL, "null pointer");
  *pieces_out = nullptr;
  *lits_out = nullptr;
  *npieces = *lits_len = 0;
  *nblocks = *body_len = 0;
  int rc = check_files(paths, path_off, sizes, nfiles);
  if (rc) return rc;
  if (bs == 0 || bs > 0xffffffffull) return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  emit::Layout lay;
  std::string err;
  if (!emit::build(emit::Files{paths, path_off, sizes, exe, nfiles}, bs, (uint64_t)INT32_MAX, &lay,
                   &err))
    return fail(CIR_EINVAL, err);
  uint64_t* p = (uint64_t*)malloc(8 * lay.pieces.size());
  uint8_t* l = (uint8_t*)malloc(lay.lits.size());
  if (!p || !l) {
    free(p);
    free(l);
    return fail(CIR_ENOMEM, "malloc");
  }
  memcpy(p, lay.pieces.data(), 8 * lay.pieces.size());
  memcpy(l, lay.lits.data(), lay.lits.size());
  if (first_block_out && nfiles) memcpy(first_block_out, lay.first_block.data(), 8 * nfiles);
  *pieces_out = p;
  *npieces = (size_t)lay.npieces();
  *lits_out = l;
  *lits_len = lay.lits.size();
  *nblocks = lay.nblocks;
  *body_len = lay.body_len;
  return CIR_OK;
}

int check_tables(const void* digests, uint64_t ndigests, const void* pieces, uint64_t npieces,
                 const void* lits, uint64_t lits_len, const void* body, uint64_t body_len,
                 const void* res) {
  if ((ndigests && !digests) || (npieces && !pieces) || (lits_len && !lits) ||
      (body_len && !body) || !res)
    return fail(CIR_EINVAL, "null pointer");
  if (npieces > emit::kMaxPieces) return fail(CIR_EINVAL, "more than 2^32-1 pieces");
  if (body_len > dev::kEmitMaxBody) return fail(CIR_EINVAL, "body longer than 2^40 bytes");
  if (ndigests > dev::kEmitMaxDigests) return fail(CIR_EINVAL, "more than 2^40 digests");
  return CIR_OK;
}

int emit_tables_impl(const uint8_t* digests, uint64_t ndigests, const uint64_t* pieces,
                     uint64_t npieces, const uint8_t* lits, uint64_t lits_len, uint8_t* body,
                     uint64_t body_len, uint64_t* res) {
  int rc = check_tables(digests, ndigests, pieces, npieces, lits, lits_len, body, body_len, res);
  if (rc) return rc;
  res[0] = emit::emit_host(emit::Tables{pieces, npieces, lits, lits_len, digests, ndigests,
                                        body_len}, body);
  return CIR_OK;
}

int emit_dev_impl(const uint8_t* d_digests, uint64_t ndigests, const uint64_t* d_pieces,
                  uint64_t npieces, const uint8_t* d_lits, uint64_t lits_len, uint8_t* d_body,
                  uint64_t body_len, uint64_t* d_res, void* stream) {
  int rc = check_tables(d_digests, ndigests, d_pieces, npieces, d_lits, lits_len, d_body, body_len,
                        d_res);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(d_body) & 15u)
    return fail(CIR_EINVAL, "d_body must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_pieces) | reinterpret_cast<uintptr_t>(d_res)) & 7u)
    return fail(CIR_EINVAL, "d_pieces and d_res must be 8-byte aligned");
  CIR_HIP(dev::launch_emit_text(emit::Tables{d_pieces, npieces, d_lits, lits_len, d_digests,
                                             ndigests, body_len},
                                d_body, d_res, (hipStream_t)stream));
  return CIR_OK;
}

int index_emit_impl(int hash_type, uint64_t bs, const uint8_t* paths, const uint64_t* path_off,
                    const uint64_t* sizes, const uint8_t* exe, size_t nfiles,
                    const uint8_t* digests, size_t ndigests, uint8_t** index_out, size_t* len_out,
                    uint8_t* image_id) {
  if (!index_out || !len_out) return fail(CIR_EINVAL, "null pointer");
  *index_out = nullptr;
  *len_out = 0;
  int rc = check_files(paths, path_off, sizes, nfiles);
  if (rc) return rc;
  if (ndigests && !digests) return fail(CIR_EINVAL, "null pointer");
  if (!valid_hash_type(hash_type)) return fail(CIR_EINVAL, "unknown hash type");
  dirsig::Header h;
  if (!header_of(hash_type, bs, &h)) return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  emit::Layout lay;
  std::string err;
  if (!emit::build(emit::Files{paths, path_off, sizes, exe, nfiles}, bs, dev::kEmitMaxDigests, &lay,
                   &err))
    return fail(CIR_EINVAL, err);
  if (lay.nblocks != ndigests)
    return fail(CIR_EINVAL, "the digest count does not match the sizes: " +
                                std::to_string(ndigests) + " given, " +
                                std::to_string(lay.nblocks) + " needed");
  if (lay.body_len > dev::kEmitMaxBody) return fail(CIR_EINVAL, "body longer than 2^40 bytes");
  return emit_index_host(lay, h, digests, index_out, len_out, image_id);
}

struct HostBuf {
  uint8_t* p = nullptr;
  ~HostBuf() { free(p); }
  uint8_t* release() {
    uint8_t* q = p;
    p = nullptr;
    return q;
  }
};

int index_memory_impl(cir_ctx* ctx, int hash_type, uint64_t bs, const uint8_t* paths,
                      const uint64_t* path_off, const uint64_t* sizes, const uint8_t* exe,
                      size_t nfiles, const void* const* d_data, void* stream, uint8_t** index_out,
                      size_t* len_out, uint8_t* image_id, uint64_t* stats) {
  if (!index_out || !len_out || !stats) return fail(CIR_EINVAL, "null pointer");
  *index_out = nullptr;
  *len_out = 0;
  for (int i = 0; i < CIR_MEMINDEX_STATS_FIELDS; ++i) stats[i] = 0;
  if (!ctx) return fail(CIR_EINVAL, "null ctx");
  int rc = check_files(paths, path_off, sizes, nfiles);
  if (rc) return rc;
  if (nfiles && !d_data) return fail(CIR_EINVAL, "null pointer");
  if (!valid_hash_type(hash_type)) return fail(CIR_EINVAL, "unknown hash type");
  dirsig::Header h;
  if (!header_of(hash_type, bs, &h)) return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  const bool trace = trace_enabled();
  const auto t0 = Clock::now();
  // the tree, the pieces and the literals, before anything is allocated or launched
  emit::Layout lay;
  std::string err;
  if (!emit::build(emit::Files{paths, path_off, sizes, exe, nfiles}, bs, (uint64_t)INT32_MAX, &lay,
                   &err))
    return fail(CIR_EINVAL, err);
  if (lay.body_len > dev::kEmitMaxBody) return fail(CIR_EINVAL, "body longer than 2^40 bytes");
  // the table of non-empty files over one arena: the lowest pointer
  uintptr_t arena = UINTPTR_MAX;
  for (size_t i = 0; i < nfiles; ++i) {
    if (!sizes[i]) continue;
    if (!d_data[i]) return fail(CIR_EINVAL, "null device pointer of a non-empty file");
    const uintptr_t p = reinterpret_cast<uintptr_t>(d_data[i]);
    if (p < arena) arena = p;
  }
  std::vector<uint64_t> files;
  for (size_t i = 0; i < nfiles; ++i)
    if (sizes[i]) {
      files.push_back(lay.first_block[i]);
      files.push_back(reinterpret_cast<uintptr_t>(d_data[i]) - arena);
      files.push_back(sizes[i]);
    }
  const uint64_t nfile_recs = files.size() / emit::kFileWords, nblk = lay.nblocks;
  hipStream_t s = (hipStream_t)stream;
  Device* d = stream_device(ctx, s);
  if (!d) return fail(CIR_EINVAL, "stream device is not part of the context");
  const bool on_host = emit_on_host();
  const std::string header = header_line(h);
  size_t cap = 0;
  HostBuf buf;  // (before the drain: the body's download writes into it)
  buf.p = index_buffer(header, lay.body_len, &cap);
  if (!buf.p) return fail(CIR_ENOMEM, "malloc");
  std::vector<uint8_t> h_digests;
  uint64_t res[CIR_EMIT_RES_FIELDS] = {};
  const auto t1 = Clock::now();

  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d->id));
  DevSet b;
  StreamDrain drain{s};
  uint64_t *d_files = nullptr, *d_pieces = nullptr, *d_off = nullptr, *d_res = nullptr;
  uint32_t* d_len = nullptr;
  uint8_t *d_lits = nullptr, *d_dig = nullptr, *d_body = nullptr;
  const uint64_t body_cap = emit::round_up16(lay.body_len);
  if ((rc = b.alloc((void**)&d_files, 8 * files.size())) ||
      (rc = b.alloc((void**)&d_off, 8 * nblk)) || (rc = b.alloc((void**)&d_len, 4 * nblk)) ||
      (rc = b.alloc((void**)&d_dig, 32 * nblk)))
    return rc;
  if (!on_host && ((rc = b.alloc((void**)&d_pieces, 8 * lay.pieces.size())) ||
                   (rc = b.alloc((void**)&d_lits, lay.lits.size())) ||
                   (rc = b.alloc((void**)&d_body, body_cap)) ||
                   (rc = b.alloc((void**)&d_res, sizeof res))))
    return rc;
  uint64_t up = 0, down = 0;
  // everything from here on is queued on the caller's stream, behind whatever
  // still produces the data there
  if (!files.empty()) {
    CIR_HIP(hipMemcpyAsync(d_files, files.data(), 8 * files.size(), hipMemcpyHostToDevice, s));
    up += 8 * files.size();
  }
  if (!on_host) {
    CIR_HIP(hipMemcpyAsync(d_pieces, lay.pieces.data(), 8 * lay.pieces.size(),
                           hipMemcpyHostToDevice, s));
    CIR_HIP(hipMemcpyAsync(d_lits, lay.lits.data(), lay.lits.size(), hipMemcpyHostToDevice, s));
    up += 8 * lay.pieces.size() + lay.lits.size();
  }
  CIR_HIP(dev::launch_mem_desc(d_files, nfile_recs, bs, nblk, d_off, d_len, s));
  if ((rc = hash_desc_ordered(*d, reinterpret_cast<const uint8_t*>(arena), d_off, d_len, nblk,
                              d_dig, s, hash_type)))
    return rc;
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t2 = Clock::now();
  auto t3 = t2;
  uint8_t* body = buf.p + header.size();
  if (on_host) {
    h_digests.resize((size_t)(32 * nblk));
    if (nblk)
      CIR_HIP(hipMemcpyAsync(h_digests.data(), d_dig, 32 * nblk, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipStreamSynchronize(s));
    down = 32 * nblk;
    t3 = Clock::now();
    emit::emit_host(lay.tables(h_digests.data()), body);
  } else {
    CIR_HIP(dev::launch_emit_text(emit::Tables{d_pieces, lay.npieces(), d_lits, lay.lits.size(),
                                               d_dig, nblk, lay.body_len},
                                  d_body, d_res, s));
    if (trace) {
      CIR_HIP(hipStreamSynchronize(s));
      t3 = Clock::now();
    }
    CIR_HIP(hipMemcpyAsync(body, d_body, body_cap, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipStreamSynchronize(s));
    down = body_cap + sizeof res;
    if (res[0]) return fail(CIR_EIO, "the emit kernel met a piece outside its arrays");
  }
  const auto t4 = Clock::now();
  *len_out = finish_index(buf.p, header.size(), lay.body_len, h, image_id);
  *index_out = buf.release();
  const auto t5 = Clock::now();
  stats[0] = nblk;
  stats[1] = on_host ? 0 : 1;
  stats[2] = nfiles;
  stats[3] = lay.body_len;
  stats[4] = up;
  stats[5] = down;
  if (trace) {
    // laps: hash, emit, download, footer (host path: the download comes before the emit)
    const double emit_ms = on_host ? ms_between(t3, t4) : ms_between(t2, t3);
    const double down_ms = on_host ? ms_between(t2, t3) : ms_between(t3, t4);
    fprintf(stderr,
            "cir index_memory: %llu files, %llu blocks, %s emitter; layout %.2f ms, upload and "
            "hash %.2f ms, emit %.2f ms, download %.2f ms (%llu bytes), footer %.2f ms; body "
            "%llu bytes\n",
            (unsigned long long)nfiles, (unsigned long long)nblk, on_host ? "host" : "device",
            ms_between(t0, t1), ms_between(t1, t2), emit_ms, down_ms, (unsigned long long)down,
            ms_between(t4, t5), (unsigned long long)lay.body_len);
  }
  return CIR_OK;
}

}  // namespace

// ---- shared with cir_store_blocks (memindex.hpp) -----------------------------

int check_files(const uint8_t* paths, const uint64_t* path_off, const uint64_t* sizes,
                size_t nfiles) {
  if (nfiles && (!path_off || !sizes || (!paths && path_off[nfiles] != path_off[0])))
    return fail(CIR_EINVAL, "null pointer");
  return CIR_OK;
}

bool header_of(int hash_type, uint64_t bs, dirsig::Header* h) {
  if (bs == 0 || bs > 0xffffffffull) return false;
  h->block_size = bs;
  h->hash = hash_type == CIR_HASH_SHA512_256 ? dirsig::HashType::kSha512_256
                                             : dirsig::HashType::kBlake2b256;
  return true;
}

int emit_index_host(const emit::Layout& lay, const dirsig::Header& h, const uint8_t* digests,
                    uint8_t** index_out, size_t* len_out, uint8_t* image_id) {
  const std::string header = header_line(h);
  size_t cap = 0;
  uint8_t* buf = index_buffer(header, lay.body_len, &cap);
  if (!buf) return fail(CIR_ENOMEM, "malloc");
  emit::emit_host(lay.tables(digests), buf + header.size());
  *len_out = finish_index(buf, header.size(), lay.body_len, h, image_id);
  *index_out = buf;
  return CIR_OK;
}

}  // namespace cir

extern "C" int cir_index_emit_layout(uint64_t block_size, const uint8_t* paths,
                                     const uint64_t* path_off, const uint64_t* sizes,
                                     const uint8_t* exe, size_t nfiles, uint64_t** pieces_out,
                                     size_t* npieces, uint8_t** lits_out, size_t* lits_len,
                                     uint64_t* first_block_out, uint64_t* nblocks,
                                     uint64_t* body_len) try {
  return cir::emit_layout_impl(block_size, paths, path_off, sizes, exe, nfiles, pieces_out, npieces,
                               lits_out, lits_len, first_block_out, nblocks, body_len);
} CIR_CATCH_BOUNDARY

extern "C" int cir_index_emit_tables(const uint8_t* digests, uint64_t ndigests,
                                     const uint64_t* pieces, uint64_t npieces, const uint8_t* lits,
                                     uint64_t lits_len, uint8_t* body, uint64_t body_len,
                                     uint64_t res[CIR_EMIT_RES_FIELDS]) try {
  return cir::emit_tables_impl(digests, ndigests, pieces, npieces, lits, lits_len, body, body_len,
                               res);
} CIR_CATCH_BOUNDARY

extern "C" int cir_index_emit(int hash_type, uint64_t block_size, const uint8_t* paths,
                              const uint64_t* path_off, const uint64_t* sizes, const uint8_t* exe,
                              size_t nfiles, const uint8_t* digests, size_t ndigests,
                              uint8_t** index_out, size_t* len_out,
                              uint8_t image_id[CIR_DIGEST_BYTES]) try {
  return cir::index_emit_impl(hash_type, block_size, paths, path_off, sizes, exe, nfiles, digests,
                              ndigests, index_out, len_out, image_id);
} CIR_CATCH_BOUNDARY

extern "C" int cir_index_emit_dev(cir_ctx* ctx, const uint8_t* d_digests, uint64_t ndigests,
                                  const uint64_t* d_pieces, uint64_t npieces,
                                  const uint8_t* d_lits, uint64_t lits_len, uint8_t* d_body,
                                  uint64_t body_len, uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::emit_dev_impl(d_digests, ndigests, d_pieces, npieces, d_lits, lits_len, d_body,
                            body_len, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_index_memory_dev(cir_ctx* ctx, int hash_type, uint64_t block_size,
                                    const uint8_t* paths, const uint64_t* path_off,
                                    const uint64_t* sizes, const uint8_t* exe, size_t nfiles,
                                    const void* const* d_data, void* stream, uint8_t** index_out,
                                    size_t* len_out, uint8_t image_id[CIR_DIGEST_BYTES],
                                    uint64_t stats[CIR_MEMINDEX_STATS_FIELDS]) try {
  return cir::index_memory_impl(ctx, hash_type, block_size, paths, path_off, sizes, exe, nfiles,
                                d_data, stream, index_out, len_out, image_id, stats);
} CIR_CATCH_BOUNDARY
