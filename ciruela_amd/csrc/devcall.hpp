// What the whole-call entry points over index texts share (sources.cpp,
// repeats.cpp, files.cpp): the per-call seed, the call's device memory, the stream drain
// and the lap clock.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <chrono>
#include <random>
#include <vector>

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

// CIR_SOURCES_PARSE=host: with a context, parse every text on the host as
// before the device parse existed (A/B measurement).
inline bool parse_on_host() {
  const char* v = getenv("CIR_SOURCES_PARSE");
  return v && strcmp(v, "host") == 0;
}

struct DevSet {
  std::vector<void*> p;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~DevSet() {
    for (void* q : p)
      if (q) (void)hipFree(q);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
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

// Waits for the stream on scope exit: declared behind the host buffers that
// asynchronous copies write, so none is destroyed with a copy in flight on an
// error return.
struct StreamDrain {
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

}  // namespace cir
