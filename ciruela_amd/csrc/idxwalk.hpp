// The walk over an index text that the device parsers share (idxscan.hip,
// files.hip): which lane owns which line, the head of a line, and the
// workgroup's exclusive scan.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "idxscan.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

using idxscan::Head;

constexpr uint32_t kSpan = 16;  // bytes of text per lane
static_assert(kIdxTile == kThreads * kSpan, "a tile is one span per lane");

// The lines the lane with the span [s, s + 16) owns, in byte order: the one
// at body_off when the span holds body_off, and the one behind every '\n' at
// q in the span with body_off <= q < body_end - 1.  f(p) is called once per
// line start p (one inlined copy of f).  Reads text[s .. s+16) as two adjacent
// 8-byte loads when the span lies inside [0, len) -- the text is only promised
// 8-byte alignment; the compiler issues them as one global_load_dwordx4, which
// gfx950 takes at that alignment (tests/test_index_kernel_resources.py reads
// the instruction off the code object) -- and bytewise up to len otherwise.
template <class F>
__device__ __forceinline__ void walk_span(const uint8_t* __restrict__ text, uint64_t len,
                                          uint64_t s, uint64_t body_off, uint64_t body_end,
                                          F&& f) {
  if (s >= body_end || s + kSpan <= body_off) return;
  uint32_t w[4] = {0, 0, 0, 0};
  if (s + kSpan <= len) {
    const uint2* p = reinterpret_cast<const uint2*>(text + s);
    const uint2 a = p[0], b = p[1];
    w[0] = a.x;
    w[1] = a.y;
    w[2] = b.x;
    w[3] = b.y;
  } else {
    for (uint32_t i = 0; i < kSpan; ++i)
      if (s + i < len) w[i >> 2] |= (uint32_t)text[s + i] << (8 * (i & 3));
  }
  uint32_t mask = 0;  // bit i: text[s + i] == '\n'
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = w[k] ^ 0x0a0a0a0au;
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 per zero byte
    mask |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
  }
  // keep body_off <= s + i < body_end - 1  (body_end > s >= 0 here)
  const uint64_t lo = body_off > s ? body_off - s : 0;
  const uint64_t hi = body_end - 1 - s < kSpan ? body_end - 1 - s : kSpan;
  mask &= (uint32_t)((1u << hi) - 1u) & ~(uint32_t)((1u << lo) - 1u);
  bool first = body_off >= s && body_off < s + kSpan && body_off < body_end;
  for (;;) {
    uint64_t p;
    if (first) {
      p = body_off;
      first = false;
    } else if (mask) {
      p = s + (uint32_t)__builtin_ctz(mask) + 1;
      mask &= mask - 1;
    } else {
      break;
    }
    f(p);
  }
}

// The head of the line at p, with the rule for the body's first line.
__device__ __forceinline__ Head head_at(const uint8_t* __restrict__ text, uint64_t p,
                                        uint64_t body_off, uint64_t body_end, uint64_t bs) {
  Head h = idxscan::parse_head(text, p, body_end, bs);
  if (p == body_off && text[p] != '/') h.kind = idxscan::kDecline;
  return h;
}

struct Pair {
  uint64_t fr;   // file entries in the low half, non-empty files in the high half
  uint64_t blk;  // blocks
};

// Exclusive scan of v over the workgroup in thread order; *total = the sum.
// lds: kThreads / 64 + 1 entries.  Safe to call in a loop.
__device__ __forceinline__ Pair block_excl_scan(Pair v, Pair* total, Pair* lds) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Pair inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t a = __shfl_up((unsigned long long)inc.fr, d, 64);
    const uint64_t b = __shfl_up((unsigned long long)inc.blk, d, 64);
    if ((int)lane >= d) {
      inc.fr += a;
      inc.blk += b;
    }
  }
  __syncthreads();  // (the previous call's readers are done with lds)
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  Pair base = {0, 0}, sum = {0, 0};
#pragma unroll
  for (uint32_t k = 0; k < kThreads / 64; ++k) {
    const Pair t = lds[k];
    if (k < wave) {
      base.fr += t.fr;
      base.blk += t.blk;
    }
    sum.fr += t.fr;
    sum.blk += t.blk;
  }
  *total = sum;
  return Pair{base.fr + inc.fr - v.fr, base.blk + inc.blk - v.blk};
}

}  // namespace dev
}  // namespace cir
