// cir_sketch_key, cir_sketch_rank, cir_sketch_digests_dev, cir_index_sketch: a
// fixed-size content sketch per image and the ranking of candidate sources
// from sketches alone.  The rule is sketch.hpp, the kernels are sketch.hip.
//
// Reference: a new image's sources are the 37 most recent images of its base
// directory by timestamp, whatever they hold (src/daemon/metadata/
// hardlink_sources.rs:66-90); every planning call here takes the sources' full
// texts, and those texts are its cost.  A sketch is made once per index, where
// the device parse leaves the digests, and kept beside it; the ranking reads
// sketches only.  cir_index_sketch's hold on the device and its parse are
// devcall.hpp's (DeviceCall, parse_one_text); a text or a sketch the device
// declines goes through dirsig::parse and sketch::bottom_k.
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "devcall.hpp"
#include "dirsig.hpp"
#include "runtime.hpp"
#include "sketch.hpp"

namespace cir {
namespace {

static_assert(CIR_SKETCH_RES_FIELDS == dev::kSketchResFields && CIR_SKETCH_OK == dev::kSketchOk &&
                  CIR_SKETCH_DECLINED == dev::kSketchDeclined &&
                  CIR_SKETCH_MAX_K == sketch::kMaxK && CIR_SKETCH_DEFAULT_K == sketch::kDefaultK,
              "the header's constants are the kernels' and the rule's");

// CIR_SKETCH=host, read per call: cir_index_sketch with a context answers with
// the host rule (A/B measurement).
bool sketch_on_host() {
  const char* v = getenv("CIR_SKETCH");
  return v && strcmp(v, "host") == 0;
}

int sketch_digests_dev_impl(const uint8_t* d_digests, uint64_t n, uint32_t k, uint64_t* d_keys,
                            void* d_work, uint64_t work_bytes, uint64_t* d_res, void* stream) {
  if ((n && !d_digests) || !d_keys || !d_work || !d_res)
    return fail(CIR_EINVAL, "null device pointer");
  if (reinterpret_cast<uintptr_t>(d_digests) & 15u)
    return fail(CIR_EINVAL, "the digest array must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_keys) | reinterpret_cast<uintptr_t>(d_work) |
       reinterpret_cast<uintptr_t>(d_res)) & 7u)
    return fail(CIR_EINVAL, "keys, scratch and result must be 8-byte aligned");
  if (k < 1 || k > sketch::kMaxK) return fail(CIR_EINVAL, "k must be 1 .. 4096");
  if (n > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 digests");
  if (work_bytes < dev::sketch_work_bytes(n))
    return fail(CIR_EINVAL, "work_bytes is below cir_sketch_work_bytes(n, k)");
  CIR_HIP(dev::launch_sketch(d_digests, n, k, d_keys, (uint64_t*)d_work, d_res,
                             (hipStream_t)stream));
  return CIR_OK;
}

struct DeviceAnswer {
  std::vector<uint64_t> keys;  // as downloaded: min(k, blocks) words
  uint64_t res[CIR_SKETCH_RES_FIELDS] = {};
  uint64_t idx_res[CIR_INDEX_RES_FIELDS] = {};
  uint64_t why = 0, down_bytes = 0;
  double parse_ms = 0, sketch_ms = 0;
  float kernels_ms = 0;
};

// parse_one_text and launch_sketch on ctx's first device.  a->why stays 0 when
// the device answered: a->res and a->keys are then the sketch.  `a` is the
// caller's, declared before the call: it outlives the drain.
int device_sketch(cir_ctx* ctx, const uint8_t* index, size_t len, uint64_t body_off,
                  uint64_t body_end, uint64_t bs, uint32_t k, bool trace, DeviceAnswer* a) {
  TraceEvents<2> tev;
  DeviceCall c(ctx);
  uint8_t* d_dig = nullptr;
  uint64_t* d_runs = nullptr;
  int rc;
  const auto t0 = Clock::now();
  if ((rc = c.begin()) || (trace && (rc = tev.create())) ||
      (rc = parse_one_text(c, index, len, body_off, body_end, bs, a->idx_res, &d_dig, &d_runs)))
    return rc;
  const auto t1 = Clock::now();
  a->parse_ms = ms_between(t0, t1);
  a->down_bytes = sizeof a->idx_res;
  if (a->idx_res[0] != CIR_INDEX_OK) {
    a->why = CIR_SKETCH_WHY_TEXT;
    return CIR_OK;
  }
  const uint64_t n = a->idx_res[3];
  const uint64_t want = n < k ? n : k;
  uint64_t *d_keys = nullptr, *d_work = nullptr, *d_res = nullptr;
  a->keys.resize((size_t)want);
  if ((rc = c.alloc(&d_keys, 8ull * k)) || (rc = c.alloc(&d_work, dev::sketch_work_bytes(n))) ||
      (rc = c.alloc(&d_res, sizeof a->res)))
    return rc;
  CIR_HIP(dev::launch_sketch(d_dig, n, k, d_keys, d_work, d_res, c.s, trace ? tev.ev : nullptr));
  CIR_HIP(hipMemcpyAsync(a->res, d_res, sizeof a->res, hipMemcpyDeviceToHost, c.s));
  if (want)
    CIR_HIP(hipMemcpyAsync(a->keys.data(), d_keys, 8 * want, hipMemcpyDeviceToHost, c.s));
  CIR_HIP(hipStreamSynchronize(c.s));
  a->down_bytes += sizeof a->res + 8 * want;
  a->sketch_ms = ms_between(t1, Clock::now());
  if (trace) a->kernels_ms = tev.lap(0);
  if (a->res[0] != CIR_SKETCH_OK || a->res[1] > want || a->res[2] != n)
    a->why = CIR_SKETCH_WHY_DECLINED;
  else
    a->keys.resize((size_t)a->res[1]);
  return CIR_OK;
}

int make_blob(const dirsig::Header& h, uint32_t k, uint64_t nblk, const std::vector<uint64_t>& keys,
              uint8_t** blob_out, size_t* blob_len) {
  const size_t bytes = sketch::blob_bytes(keys.size());
  uint8_t* blob = (uint8_t*)malloc(bytes);
  if (!blob) return fail(CIR_ENOMEM, "malloc");
  sketch::encode((uint32_t)h.hash, k, h.block_size, nblk, keys.data(), keys.size(), blob);
  *blob_out = blob;
  *blob_len = bytes;
  return CIR_OK;
}

int index_sketch_impl(cir_ctx* ctx, const uint8_t* index, size_t len, uint32_t k,
                      uint8_t** blob_out, size_t* blob_len, uint64_t* stats) {
  if (!index || !blob_out || !blob_len || !stats) return fail(CIR_EINVAL, "null pointer");
  *blob_out = nullptr;
  *blob_len = 0;
  for (int i = 0; i < CIR_SKETCH_STATS_FIELDS; ++i) stats[i] = 0;
  if (k < 1 || k > sketch::kMaxK) return fail(CIR_EINVAL, "k must be 1 .. 4096");
  const bool trace = trace_enabled();
  const auto t0 = Clock::now();
  uint64_t why = 0, uploaded = 0, downloaded = 0;
  if (ctx) {
    if (ctx->devs.empty()) return fail(CIR_EINVAL, "context without a device");
    dirsig::Header h;
    size_t body_off = 0, body_end = 0;
    std::string err;
    if (sketch_on_host()) {
      why = CIR_SKETCH_WHY_ENV;
    } else if (!device_takes(len)) {
      why = CIR_SKETCH_WHY_SIZE;
    } else if (dirsig::frame(index, len, &h, &body_off, &body_end, &err)) {
      // (a frame that does not parse is the host parser's to report)
      DeviceAnswer a;
      const auto t1 = Clock::now();
      int rc = device_sketch(ctx, index, len, body_off, body_end, h.block_size, k, trace, &a);
      if (rc) return rc;
      uploaded = len;
      downloaded = a.down_bytes;
      why = a.why;
      if (!why) {
        if ((rc = make_blob(h, k, a.res[2], a.keys, blob_out, blob_len))) return rc;
        stats[0] = 1;
        stats[2] = a.res[2];
        stats[3] = a.keys.size();
        stats[4] = uploaded;
        stats[5] = downloaded;
        if (trace)
          fprintf(stderr,
                  "cir index_sketch: %llu blocks, k %u, device; frame %.2f ms, upload and parse "
                  "%.2f ms, sketch kernels %.3f ms, sketch and download %.2f ms (%llu bytes); %llu "
                  "keys of %llu candidates\n",
                  (unsigned long long)a.res[2], k, ms_between(t0, t1), a.parse_ms, a.kernels_ms,
                  a.sketch_ms, (unsigned long long)downloaded, (unsigned long long)a.res[1],
                  (unsigned long long)a.res[3]);
        return CIR_OK;
      }
    }
  }
  dirsig::Index idx;
  std::string err;
  if (!dirsig::parse(index, len, &idx, &err)) return parse_fail(idx.bad_hash_size, err);
  std::vector<uint64_t> all = sketch::index_keys(idx);
  const uint64_t nblk = all.size();
  const std::vector<uint64_t> keys = sketch::bottom_k(&all, k);
  const int rc = make_blob(idx.header, k, nblk, keys, blob_out, blob_len);
  if (rc) return rc;
  stats[1] = why;
  stats[2] = nblk;
  stats[3] = keys.size();
  stats[4] = uploaded;
  stats[5] = downloaded;
  if (trace)
    fprintf(stderr, "cir index_sketch: %llu blocks, k %u, host (why %llu); %.2f ms; %zu keys\n",
            (unsigned long long)nblk, k, (unsigned long long)why, ms_between(t0, Clock::now()),
            keys.size());
  return CIR_OK;
}

int sketch_rank_impl(const uint8_t* need, size_t need_len, const uint8_t* const* src,
                     const size_t* src_len, size_t nsrc, uint64_t* order_out, uint64_t* shared_out,
                     uint64_t* examined_out, size_t* nranked_out, size_t* nskipped_out) {
  if (!need || !nranked_out || (nsrc && (!src || !src_len || !order_out || !shared_out ||
                                         !examined_out)))
    return fail(CIR_EINVAL, "null pointer");
  *nranked_out = 0;
  if (nskipped_out) *nskipped_out = 0;
  sketch::View nv;
  if (!sketch::view(need, need_len, &nv)) return fail(CIR_EPARSE, "the need sketch is not valid");
  size_t skipped = 0;
  const std::vector<sketch::Ranked> r = sketch::rank(nv, src, src_len, nsrc, &skipped);
  for (size_t i = 0; i < r.size(); ++i) {
    order_out[i] = r[i].ordinal;
    shared_out[i] = r[i].shared;
    examined_out[i] = r[i].examined;
  }
  *nranked_out = r.size();
  if (nskipped_out) *nskipped_out = skipped;
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" uint64_t cir_sketch_key(const uint8_t* digest) {
  return digest ? cir::sketch::key(digest) : 0;
}

extern "C" uint64_t cir_sketch_work_bytes(uint64_t n, uint32_t k) {
  (void)k;  // (the candidate buffer is sized for the largest k)
  return cir::dev::sketch_work_bytes(n);
}

extern "C" int cir_sketch_rank(const uint8_t* need, size_t need_len, const uint8_t* const* src,
                               const size_t* src_len, size_t nsrc, uint64_t* order_out,
                               uint64_t* shared_out, uint64_t* examined_out, size_t* nranked_out,
                               size_t* nskipped_out) try {
  return cir::sketch_rank_impl(need, need_len, src, src_len, nsrc, order_out, shared_out,
                               examined_out, nranked_out, nskipped_out);
} CIR_CATCH_BOUNDARY

extern "C" int cir_sketch_digests_dev(cir_ctx* ctx, const uint8_t* d_digests, uint64_t n,
                                      uint32_t k, uint64_t* d_keys, void* d_work,
                                      uint64_t work_bytes, uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::sketch_digests_dev_impl(d_digests, n, k, d_keys, d_work, work_bytes, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_index_sketch(cir_ctx* ctx, const uint8_t* index, size_t len, uint32_t k,
                                uint8_t** blob_out, size_t* blob_len,
                                uint64_t stats[CIR_SKETCH_STATS_FIELDS]) try {
  return cir::index_sketch_impl(ctx, index, len, k, blob_out, blob_len, stats);
} CIR_CATCH_BOUNDARY
