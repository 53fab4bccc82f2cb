// The kernels of cir_index_emit_dev and cir_index_memory_dev: from digests in
// device memory to the body text of a DIRSIGNATURE.v1 index, the inverse of
// idxscan.hip.  The rule is emit.hpp; the reference has no counterpart (its
// emitter, dir-signature's v1::Emitter behind MutableIndex::to_raw_data,
// src/cluster/download.rs:266-319, runs on one host thread over host digests).
//
//   k_emit_text : output-driven, one lane per 16 aligned bytes of the body.
//                 The lane bisects the piece table by out_off (emit::piece_at,
//                 at most 32 steps, bounded by the piece count), walks forward
//                 piece by piece inside its 16 bytes (emit::fill16), taking
//                 literal bytes from the arena and hex digits from the digests,
//                 and stores its 16 bytes with one dwordx4 store.  The last
//                 lane pads with zero bytes, so the launch writes every byte of
//                 [0, round_up(body_len, 16)) and nothing else, whatever the
//                 tables hold: a lane never stores outside its own 16 bytes.
//                 Reads are guarded: a piece whose literal or block range lies
//                 outside the arrays yields zero bytes and is counted in *res,
//                 one atomicAdd per wave that met any, behind the launcher's
//                 memset on the same stream.
//   k_mem_desc  : one lane per block: bisects the table of non-empty files
//                 {first_block, base offset, size} (emit::desc_of) and writes
//                 the block's (off, len) descriptor, so the host builds and
//                 uploads 24 bytes per file instead of 12 per block.
//
// No LDS, no scratch, no lane waits for another; the wave sum of the bad-piece
// counts is five ballots that every lane of the wave reaches.
#include "emit.hpp"
#include "kernels.hpp"

namespace cir {
namespace dev {

using ull = unsigned long long;

__global__ void k_emit_text(emit::Tables t, uint8_t* __restrict__ body, ull* __restrict__ res) {
  const uint64_t lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t off = lane * emit::kLaneBytes;
  uint32_t nbad = 0;
  if (off < t.body_len) {
    uint64_t p = emit::piece_at(t.pieces, t.npieces, off);
    uint32_t w[4];
    emit::fill16(t, off, &p, w, &nbad);
    *reinterpret_cast<uint4*>(body + off) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  // the wave's sum, bit by bit: a lane meets at most 16 pieces (one per byte)
  uint32_t sum = 0;
#pragma unroll
  for (int b = 0; b < 5; ++b) sum += (uint32_t)__popcll(__ballot((nbad >> b) & 1u)) << b;
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(res, (ull)sum);
}

__global__ void k_mem_desc(const uint64_t* __restrict__ files, uint64_t nfiles, uint64_t bs,
                           uint64_t nblocks, uint64_t* __restrict__ off,
                           uint32_t* __restrict__ len) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= nblocks) return;
  uint64_t o;
  uint32_t l;
  emit::desc_of(files, nfiles, bs, g, &o, &l);
  off[g] = o;
  len[g] = l;
}

hipError_t launch_emit_text(const emit::Tables& t, uint8_t* body, uint64_t* res, hipStream_t s) {
  hipError_t e = hipMemsetAsync(res, 0, sizeof(uint64_t) * kEmitResFields, s);
  if (e != hipSuccess || t.body_len == 0) return e;
  const uint64_t lanes = emit::round_up16(t.body_len) / emit::kLaneBytes;
  const dim3 grid((unsigned)((lanes + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_emit_text, grid, dim3(kThreads), 0, s, t, body, reinterpret_cast<ull*>(res));
  return hipGetLastError();
}

hipError_t launch_mem_desc(const uint64_t* files, uint64_t nfiles, uint64_t bs, uint64_t nblocks,
                           uint64_t* off, uint32_t* len, hipStream_t s) {
  if (nblocks == 0) return hipSuccess;
  const dim3 grid((unsigned)((nblocks + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k_mem_desc, grid, dim3(kThreads), 0, s, files, nfiles, bs, nblocks, off, len);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace cir
