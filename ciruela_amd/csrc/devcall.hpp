// What the whole-call entry points over index texts share (sources.cpp,
// repeats.cpp, files.cpp, copies.cpp, plan.cpp, idxscan.cpp): the per-call
// seed and lap clock, the call's hold on the context's first device
// (DeviceCall), the trace events, the size test, the two device parses of
// index texts (TextSet: k framed texts in two passes; parse_one_text: one text
// in one shot), the file-level stage over a TextSet (FileStage: files.cpp,
// copies.cpp, plan.cpp) and the extent tail on the device.  The bodies are
// devcall.cpp.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <chrono>
#include <mutex>
#include <random>
#include <vector>

#include "copies.hpp"
#include "dirsig.hpp"
#include "idxscan.hpp"
#include "runtime.hpp"

namespace cir {

inline uint64_t draw_seed() {
  uint64_t s = 0;
  if (getrandom(&s, sizeof s, 0) == (ssize_t)sizeof s) return s;
  std::random_device rd;
  return ((uint64_t)rd() << 32) ^ rd();
}

using Clock = std::chrono::steady_clock;
inline double ms_between(Clock::time_point a, Clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// (no CIR_* code is positive) the host rule decides this call
constexpr int kHostFlow = 2;

// CIR_SOURCES_PARSE=host: with a context, parse every text on the host as
// before the device parse existed (A/B measurement).
inline bool parse_on_host() {
  const char* v = getenv("CIR_SOURCES_PARSE");
  return v && strcmp(v, "host") == 0;
}

// CIR_LINKS_MATCH=host, read per call: cir_file_sources and cir_file_copies
// with a context answer with the host rule (A/B measurement).
inline bool match_on_host() {
  const char* v = getenv("CIR_LINKS_MATCH");
  return v && strcmp(v, "host") == 0;
}

// May an index text of len bytes be parsed on the device?  (The kernels'
// limit, and u32 block ordinals.)
inline bool device_takes(size_t len) {
  return len <= dev::kIdxMaxLen && len / idxscan::kTokenBytes <= 0xFFFFFFFFull;
}

// N events for a traced call's kernel laps; none exists until create().
template <int N>
struct TraceEvents {
  hipEvent_t ev[N] = {};
  ~TraceEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int create() {
    for (hipEvent_t& e : ev) CIR_HIP(hipEventCreate(&e));
    return CIR_OK;
  }
  float lap(int i) const {  // ev[i] to ev[i + 1] in ms, 0 when it cannot be read
    float f = 0;
    return hipEventElapsedTime(&f, ev[i], ev[i + 1]) == hipSuccess ? f : 0;
  }
};

struct DevSet {
  std::vector<void*> p;
  ~DevSet() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
  int alloc(void** out, size_t bytes) {
    void* q = nullptr;
    if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CIR_ENOMEM, "hipMalloc of the call's buffers");
    }
    p.push_back(q);
    *out = q;
    return CIR_OK;
  }
};

// Waits for the stream on scope exit, so that no host buffer is destroyed and
// no device buffer freed with a copy in flight on an error return.
struct StreamDrain {
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// A call's hold on the context's first device (the caller has checked that
// there is one, where it checks).  The members' order is the call's epilogue
// in reverse: drain the stream, free the call's device memory, restore the
// caller's device, unlock.  Host buffers that asynchronous copies read or
// write are declared before it, so they outlive the drain.
struct DeviceCall {
  Device& d;
  std::unique_lock<std::mutex> lk;
  DeviceGuard guard;
  hipStream_t s;
  DevSet b;
  StreamDrain drain;
  explicit DeviceCall(cir_ctx* ctx) : d(*ctx->devs[0]), lk(d.mu), s(d.compute), drain{s} {}
  int begin() {  // first, and once
    CIR_HIP(hipSetDevice(d.id));
    return CIR_OK;
  }
  // Around the host parse of a text the device declined: the stream is idle
  // then and the buffers are this call's own.
  void unlock() { lk.unlock(); }
  void lock() { lk.lock(); }
  template <class T>
  int alloc(T** out, size_t bytes) {
    return b.alloc((void**)out, bytes);
  }
};

// The two-pass device parse of k framed texts that share a block size, into
// digest buffers of exactly the counted size.  It owns the host memory its
// copies write, so it is declared before the DeviceCall it works on.
struct TextSet {
  struct Item {
    const uint8_t* p;
    size_t len, body_off, body_end;
    uint64_t text_off, work_off, runs_off;  // bytes / bytes / records in the buffers
    uint64_t cnt[CIR_INDEX_RES_FIELDS];     // the count pass's result words
    std::vector<idxscan::Run> runs;         // after finish(c, true)
  };
  std::vector<Item> item;
  uint64_t text_bytes = 0, work_bytes = 0, run_recs = 0;
  uint8_t* d_text = nullptr;
  uint8_t* d_work = nullptr;
  uint64_t* d_res = nullptr;
  uint64_t* d_runs = nullptr;
  std::vector<uint64_t> res;                  // the result words as last downloaded
  Clock::time_point t_bufs, t_up, t_counted;  // buffers there / texts up / counts in

  size_t add(const uint8_t* p, size_t len, size_t body_off, size_t body_end);
  // Allocates the texts' buffers (the text buffer with text_slack bytes to
  // spare), uploads, runs the count pass, downloads item[i].cnt, synchronises.
  // An empty set allocates and copies nothing.
  int count(DeviceCall& c, uint64_t bs, size_t text_slack, bool trace);
  bool counted_ok(size_t i) const { return item[i].cnt[0] == CIR_INDEX_OK; }
  // Queues text i's emit pass: max_blocks digests to d_digests.
  int emit(DeviceCall& c, size_t i, uint8_t* d_digests, uint64_t max_blocks);
  // Queues the download of the verdicts, with the run table of every text the
  // count pass took if with_runs, and synchronises.
  int finish(DeviceCall& c, bool with_runs);
  uint64_t status(size_t i) const { return res[CIR_INDEX_RES_FIELDS * i]; }

 private:
  uint64_t bs_ = 0;
};

// The file-level stage over a TextSet, which cir_file_sources, cir_file_copies
// and cir_fetch_plan share: the new index and the sources that take part are
// counted, then emitted with their file records (launch_index_files) into one
// need side and one pool side, the inputs of the file joins.  A text the
// device declines, at any step, sends the whole call to the host rule: every
// step returns a CIR_* code, or kHostFlow with *why set to a CIR_FILE_WHY_*
// reason.  The steps run once each, in the order declared; the caller's own
// allocations, uploads, launches and downloads go between them.  Like TextSet
// it owns host memory that asynchronous copies read and write, so it is
// declared before the DeviceCall it works on.
struct FileStage {
  struct Text {            // beside ts.item[k]
    uint32_t ordinal = 0;  // the source's, as the caller counts
    uint64_t fwork_off = 0;
    uint64_t nfiles = 0, nblk = 0;
  };
  TextSet ts;  // the new index, then the sources that take part
  std::vector<Text> tx;
  dirsig::Header h;                        // the new index's
  size_t used = 0;                         // sources that take part
  std::vector<uint64_t> src_first, f_res;  // used + 1 pool ordinals; kResFields words per text
  uint64_t pool_files = 0, pool_blocks = 0;
  // the record kernels' scratch and results; the joins' inputs: digests and
  // records of either side, and src_first
  uint8_t *d_fwork = nullptr, *d_ndig = nullptr, *d_pdig = nullptr;
  uint64_t *d_fres = nullptr, *d_nrec = nullptr, *d_prec = nullptr, *d_first = nullptr;

  // Frames the new index and every source; a source that is null, does not
  // frame, or has another hash or block size is skipped and not uploaded.
  int frame(const uint8_t* index, size_t len, const uint8_t* const* src_index,
            const size_t* src_len, size_t nsrc, uint64_t* why);
  // TextSet::count (the first synchronise), then the counts per text, the
  // sources' first pool ordinals and the joins' limits.
  int count(DeviceCall& c, bool trace, uint64_t* why);
  // d_fwork, d_fres, d_ndig, d_pdig, d_nrec, d_prec, d_first, in that order
  // (devcall.cpp says why), behind the texts' and in front of the caller's own.
  int alloc(DeviceCall& c);
  // Queues the upload of src_first, then per text the emit pass and the record
  // kernels, into the need side or the pool side's next slice.
  int emit(DeviceCall& c);
  // Queues the download of f_res.  The caller queues its own downloads behind
  // it and calls ts.finish(c, with_runs), which synchronises.
  int queue_verdicts(DeviceCall& c) {
    CIR_HIP(hipMemcpyAsync(f_res.data(), d_fres, 8 * f_res.size(), hipMemcpyDeviceToHost, c.s));
    return CIR_OK;
  }
  // Every verdict is in: a bad token shows only after the decode pass.
  // joins_ok: did every file join of the caller end with files::kOk?
  int verdicts_ok(bool joins_ok, uint64_t* why) const;

  uint64_t need_files() const { return tx[0].nfiles; }
  uint64_t need_blocks() const { return tx[0].nblk; }
  dev::FilesSide need() const {
    return {ts.d_text, ts.text_bytes, d_nrec, need_files(), d_ndig, need_blocks()};
  }
  dev::FilesSide pool() const {
    return {ts.d_text, ts.text_bytes, d_prec, pool_files, d_pdig, pool_blocks};
  }
  // The texts as copies::compact reads them: the need's, then the sources'.
  std::vector<copies::PlacedText> placed() const;

 private:
  uint64_t fwork_bytes_ = 0;
};

// The one-shot device parse of one framed text: upload, launch_index_digests
// into capacity-sized buffers of c, res downloaded, one synchronise.
int parse_one_text(DeviceCall& c, const uint8_t* text, size_t len, uint64_t body_off,
                   uint64_t body_end, uint64_t bs, uint64_t res[CIR_INDEX_RES_FIELDS],
                   uint8_t** d_digests, uint64_t** d_runs);

// The extent tail on the device, behind launch_extent_map(a, ..., d_fetch, ~0,
// d_work, d_xres) and the synchronise that learnt `count`, its x_res[5]: the
// records are allocated exactly, emitted and downloaded with the fetch
// bitmap.  *rec (null when count is 0) and *fetch are malloc'd and the
// caller's; on failure the stream is drained before they are freed.
// lap_emit: synchronise behind the emit kernels, for *t_emit (a traced call).
int device_extent_tail(DeviceCall& c, const dev::ExtentArgs& a, uint64_t count, uint64_t* d_work,
                       uint64_t* d_xres, const uint64_t* d_fetch, bool lap_emit, uint64_t** rec,
                       uint64_t** fetch, Clock::time_point* t_emit);

}  // namespace cir
