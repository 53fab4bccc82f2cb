// The rule of cir_index_sketch and cir_sketch_rank, written once: a fixed-size
// content sketch of an index (the k smallest distinct 64-bit keys of its block
// digests) and the ranking of candidate sources by how much of a new image
// each one holds, read from sketches alone.  Header-only and free of HIP (the
// way plan.hpp and copies.hpp hold theirs): the kernels' host side
// (sketch.hip), the host path (sketch.cpp) and the fuzz (tools/sketch_fuzz.cpp)
// all use this text.
//
// Key of a digest: x = kSeed; for the four little-endian u64 words w of the 32
// bytes, in order: x = (x ^ w) * 0x9E3779B97F4A7C15, x ^= x >> 32; the key is
// the full x.  This is join.hip's mix (digest_slot.hpp), unmasked, under a
// fixed seed: sketches are stored and compared across calls, so every call
// must give a digest the same key.  All 32 bytes take part, and every step is
// invertible, so for any three leading words a last word exists that gives any
// chosen key.  An index's author can therefore choose the keys of their own
// digests.  That can only mislead the ranking -- which images a caller hands to
// cir_fetch_plan -- never the plan, which is exact over the texts it is given.
//
// Sketch of size k (1 <= k <= kMaxK): the k smallest distinct keys of the
// digests of all blocks of all file entries (cir_index_digests' block list),
// ascending; all of them when there are fewer than k.  Distinct by key.
//
// Blob, little-endian: magic "CIRSKv1\0", u32 hash_type, u32 k, u64 block_size,
// u64 n_blocks, u64 count, count u64 keys.  Valid iff the magic matches, 1 <= k
// <= kMaxK, count <= k, count <= n_blocks, the length is exactly 40 + 8 count
// and the keys are strictly ascending.  Everything that reads a blob validates
// it first (view()).
//
// Overlap of a need sketch N and a source sketch S: t(X) = X's last key if X is
// full (count == k), else 2^64 - 1; tau = min(t(N), t(S)).  Both sketches are
// complete below tau, so over keys <= tau the comparison is exact: examined =
// N's keys <= tau, shared = how many of those S holds.
//
// Rank: sources by shared / examined descending (cross-multiplied in integers;
// examined == 0 counts as 0), ties to the lower ordinal.  A source that is
// null, invalid or of another hash type or block size is left out and counted.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dirsig.hpp"

namespace cir {
namespace sketch {

constexpr uint64_t kSeed = 0x243F6A8885A308D3ull;
constexpr uint64_t kMul = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kMaxK = 4096;
constexpr uint32_t kDefaultK = 1024;
constexpr size_t kHeaderBytes = 40;
constexpr char kMagic[8] = {'C', 'I', 'R', 'S', 'K', 'v', '1', '\0'};

inline uint64_t load_le64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
  return v;
}
inline uint32_t load_le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline void store_le64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
inline void store_le32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

inline uint64_t mix(uint64_t x, uint64_t w) {
  x = (x ^ w) * kMul;
  return x ^ (x >> 32);
}

// The key of one 32-byte digest.
inline uint64_t key(const uint8_t* digest) {
  uint64_t x = kSeed;
  for (int i = 0; i < 4; ++i) x = mix(x, load_le64(digest + 8 * i));
  return x;
}

// The k smallest distinct of `keys`, ascending (keys is reordered).
inline std::vector<uint64_t> bottom_k(std::vector<uint64_t>* keys, uint32_t k) {
  std::vector<uint64_t>& v = *keys;
  // Distinct keys among the m smallest values can fall short of k when values
  // repeat: widen m until they do not, or until every value is in.
  size_t m = std::min(v.size(), (size_t)k);
  for (;;) {
    std::partial_sort(v.begin(), v.begin() + m, v.end());
    std::vector<uint64_t> out(v.begin(), v.begin() + m);
    out.erase(std::unique(out.begin(), out.end()), out.end());
    if (out.size() >= k || m == v.size()) {
      if (out.size() > k) out.resize(k);
      return out;
    }
    m = v.size() - m < m ? v.size() : 2 * m;
  }
}

// The sketch of n digests of 32 bytes.
inline std::vector<uint64_t> of_digests(const uint8_t* digests, uint64_t n, uint32_t k) {
  std::vector<uint64_t> keys((size_t)n);
  for (uint64_t i = 0; i < n; ++i) keys[(size_t)i] = key(digests + 32 * i);
  return bottom_k(&keys, k);
}

// The keys of all blocks of all file entries of a parsed index, in index order
// (repeats included): cir_index_digests' block list.
inline std::vector<uint64_t> index_keys(const dirsig::Index& idx) {
  std::vector<uint64_t> keys;
  for (const dirsig::Entry& e : idx.entries) {
    if (e.kind != dirsig::EntryKind::kFile) continue;
    for (size_t o = 0; o + 32 <= e.hashes.size(); o += 32) keys.push_back(key(e.hashes.data() + o));
  }
  return keys;
}

inline size_t blob_bytes(size_t count) { return kHeaderBytes + 8 * count; }

// out: blob_bytes(count) bytes.
inline void encode(uint32_t hash_type, uint32_t k, uint64_t block_size, uint64_t n_blocks,
                   const uint64_t* keys, size_t count, uint8_t* out) {
  memcpy(out, kMagic, 8);
  store_le32(out + 8, hash_type);
  store_le32(out + 12, k);
  store_le64(out + 16, block_size);
  store_le64(out + 24, n_blocks);
  store_le64(out + 32, count);
  for (size_t i = 0; i < count; ++i) store_le64(out + kHeaderBytes + 8 * i, keys[i]);
}

// A validated blob.  Nothing outside [blob, blob + len) is read.
struct View {
  uint32_t hash_type = 0, k = 0;
  uint64_t block_size = 0, n_blocks = 0, count = 0;
  const uint8_t* keys = nullptr;  // count little-endian u64, not aligned
  uint64_t at(uint64_t i) const { return load_le64(keys + 8 * i); }
  bool full() const { return count == k; }
  // t(X)
  uint64_t reach() const { return full() ? at(count - 1) : ~0ull; }
};

inline bool view(const uint8_t* blob, size_t len, View* v) {
  if (!blob || len < kHeaderBytes || memcmp(blob, kMagic, 8) != 0) return false;
  v->hash_type = load_le32(blob + 8);
  v->k = load_le32(blob + 12);
  v->block_size = load_le64(blob + 16);
  v->n_blocks = load_le64(blob + 24);
  v->count = load_le64(blob + 32);
  v->keys = blob + kHeaderBytes;
  if (v->k < 1 || v->k > kMaxK || v->count > v->k || v->count > v->n_blocks) return false;
  if (len != kHeaderBytes + 8 * (size_t)v->count) return false;
  for (uint64_t i = 1; i < v->count; ++i)
    if (v->at(i - 1) >= v->at(i)) return false;
  return true;
}

// One merge over the two ascending key lists.
inline void overlap(const View& need, const View& src, uint64_t* shared, uint64_t* examined) {
  const uint64_t tau = std::min(need.reach(), src.reach());
  uint64_t sh = 0, ex = 0, j = 0;
  for (uint64_t i = 0; i < need.count; ++i) {
    const uint64_t x = need.at(i);
    if (x > tau) break;
    ++ex;
    while (j < src.count && src.at(j) < x) ++j;
    if (j < src.count && src.at(j) == x) ++sh;
  }
  *shared = sh;
  *examined = ex;
}

struct Ranked {
  uint64_t ordinal, shared, examined;
};

// Is a's fraction above b's?  shared <= examined <= kMaxK: the products fit.
inline bool better(const Ranked& a, const Ranked& b) {
  const uint64_t l = a.examined ? a.shared * (b.examined ? b.examined : 1) : 0;
  const uint64_t r = b.examined ? b.shared * (a.examined ? a.examined : 1) : 0;
  return l > r;
}

// need: a valid view.  Sources that take part, best first; *nskipped = the rest.
inline std::vector<Ranked> rank(const View& need, const uint8_t* const* src, const size_t* src_len,
                                size_t nsrc, size_t* nskipped) {
  std::vector<Ranked> out;
  size_t skipped = 0;
  for (size_t s = 0; s < nsrc; ++s) {
    View v;
    if (!src[s] || !view(src[s], src_len[s], &v) || v.hash_type != need.hash_type ||
        v.block_size != need.block_size) {
      ++skipped;
      continue;
    }
    Ranked r{s, 0, 0};
    overlap(need, v, &r.shared, &r.examined);
    out.push_back(r);
  }
  // (stable: ties keep the caller's order)
  std::stable_sort(out.begin(), out.end(), better);
  *nskipped = skipped;
  return out;
}

}  // namespace sketch
}  // namespace cir
