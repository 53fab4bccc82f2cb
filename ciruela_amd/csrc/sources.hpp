// cir_block_sources' host side, header-only and free of HIP: the need list and
// the pool of two or more parsed indexes, the host join and the mapping of a
// pool ordinal back to (source, file, block), and the merge of those into
// extents (cir_block_extents; the continuation rule is extents.hpp), handed
// over as malloc'd arrays by extents_owned (the host tail of cir_block_extents
// and cir_block_repeats), and pack_runs, the run tables as the kernels read
// them.  Compiled alone by tools/sources_fuzz.cpp, tools/extents_fuzz.cpp and
// tools/repeats_fuzz.cpp (with dirsig.cpp) under the sanitizers.
//
// The rule (include/ciruela_blockhash.h, cir_block_sources): the need list is
// the new index's file entries in index order, blocks ascending; the pool is
// the sources in the order given, each source's file entries in index order,
// blocks ascending, pool ordinal j counting across all sources; block g
// matches the smallest j with an equal 32-byte digest (the first source in the
// caller's ranking, then the first place in index order: the flavour of
// scan_links' break, src/daemon/metadata/hardlink_sources.rs:143); a match
// whose two blocks differ in length is dropped and no second one looked for.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "dirsig.hpp"
#include "extents.hpp"

namespace cir {
namespace sources {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kNone64 = ~0ull;
constexpr uint64_t kMaxPool = 0x7FFFFFFFull;  // pool ordinals are u32 below kNone's half

// May a pool hold n blocks?  (u32 ordinals; the device join's limit.)
inline bool pool_count_ok(uint64_t n) { return n <= kMaxPool; }

// Length of block b of a file of `size` bytes in blocks of bs: min(bs, size - b bs).
inline uint64_t block_len(uint64_t size, uint64_t bs, uint64_t b) {
  const uint64_t off = b * bs;
  return size - off < bs ? size - off : bs;
}

// One non-empty file of a block list: its first ordinal in the list, and
// where it comes from.  The list of these, ascending in `first`, is the
// per-file prefix table: no per-block side table is kept.
struct FileRun {
  uint64_t first;  // ordinal (global block number, or pool ordinal) of its block 0
  uint64_t size;   // the entry's size in bytes
  uint64_t file;   // file ordinal in its index (file entries only, from 0)
  uint32_t src;    // source ordinal in the order the caller gave (0 for a need list)
};

struct BlockList {
  std::vector<FileRun> runs;  // the non-empty files, `first` strictly increasing
  uint64_t n = 0;             // blocks in all
};

// The non-empty file entries of idx appended to list as source `src`; returns
// the blocks added.  Digests are 32 bytes each (every v1 hash type).
inline uint64_t append_runs(const dirsig::Index& idx, uint32_t src, BlockList* list) {
  uint64_t file = 0, added = 0;
  for (const dirsig::Entry& en : idx.entries) {
    if (en.kind != dirsig::EntryKind::kFile) continue;
    const uint64_t nb = en.hashes.size() / 32;
    if (nb) {
      list->runs.push_back(FileRun{list->n, en.size, file, src});
      list->n += nb;
      added += nb;
    }
    ++file;
  }
  return added;
}

// Blocks of idx's file entries (what append_runs would add), without a list.
inline uint64_t count_blocks(const dirsig::Index& idx) {
  uint64_t n = 0;
  for (const dirsig::Entry& en : idx.entries)
    if (en.kind == dirsig::EntryKind::kFile) n += en.hashes.size() / 32;
  return n;
}

// The digests of idx's file entries, back to back in list order, to out
// (32 x count_blocks(idx) bytes).
inline void copy_digests(const dirsig::Index& idx, uint8_t* out) {
  for (const dirsig::Entry& en : idx.entries) {
    if (en.kind != dirsig::EntryKind::kFile || en.hashes.empty()) continue;
    memcpy(out, en.hashes.data(), en.hashes.size());
    out += en.hashes.size();
  }
}

// The run that holds ordinal j (j < list.n): the last one with first <= j.
inline const FileRun& run_of(const BlockList& list, uint64_t j) {
  size_t lo = 0, hi = list.runs.size();  // invariant: runs[lo].first <= j < runs[hi].first
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (list.runs[mid].first <= j)
      lo = mid;
    else
      hi = mid;
  }
  return list.runs[lo];
}

// A 32-byte digest as a hash-map key (like the registry's Key32).
struct Key32 {
  uint8_t b[32];
  bool operator==(const Key32& o) const { return memcmp(b, o.b, 32) == 0; }
};
struct Key32Hash {
  uint64_t seed = 0x243F6A8885A308D3ull;  // (a caller that joins untrusted digests draws one)
  size_t operator()(const Key32& k) const {
    uint64_t w[4];
    memcpy(w, k.b, 32);
    uint64_t x = seed;
    for (int i = 0; i < 4; ++i) {
      x = (x ^ w[i]) * 0x9E3779B97F4A7C15ull;
      x ^= x >> 32;
    }
    return (size_t)x;
  }
};

// The join on the host: match[i] = the smallest j < n_pool with pool[j] ==
// need[i], or kNone, for the wanted i (want: a bitmap, nullptr = all; the
// others get kNone).  Inserting in ascending order, the first entry wins.
// Returns the number of matches.
inline uint64_t host_join(const uint8_t* need, uint64_t n_need, const uint8_t* pool,
                          uint64_t n_pool, const uint64_t* want, uint32_t* match,
                          uint64_t seed = 0x243F6A8885A308D3ull) {
  std::unordered_map<Key32, uint32_t, Key32Hash> map(16, Key32Hash{seed});
  map.reserve((size_t)n_pool);
  Key32 k;
  for (uint64_t j = 0; j < n_pool; ++j) {
    memcpy(k.b, pool + 32 * j, 32);
    map.emplace(k, (uint32_t)j);  // (an equal key is already there: the smaller j stays)
  }
  uint64_t hits = 0;
  for (uint64_t i = 0; i < n_need; ++i) {
    match[i] = kNone;
    if (want && !(want[i >> 6] >> (i & 63) & 1)) continue;
    memcpy(k.b, need + 32 * i, 32);
    const auto it = map.find(k);
    if (it != map.end()) {
      match[i] = it->second;
      ++hits;
    }
  }
  return hits;
}

struct MapStats {
  uint64_t wanted = 0, found = 0, bytes = 0, dropped = 0;
};

// match[g] (a pool ordinal or kNone, for every block g of the need list) to
// the result arrays, with the length check; a block that is not wanted is
// "not found" whatever match[g] holds.  src / file / block: need.n entries.
inline MapStats map_matches(const BlockList& need, const BlockList& pool, uint64_t bs,
                            const uint64_t* want, const uint32_t* match, uint32_t* src,
                            uint64_t* file, uint64_t* block) {
  MapStats st;
  for (const FileRun& r : need.runs) {
    const uint64_t nb = r.size / bs + (r.size % bs != 0);
    for (uint64_t b = 0; b < nb; ++b) {
      const uint64_t g = r.first + b;
      src[g] = kNone;
      file[g] = kNone64;
      block[g] = kNone64;
      if (want && !(want[g >> 6] >> (g & 63) & 1)) continue;
      ++st.wanted;
      const uint32_t j = match[g];
      if (j == kNone || j >= pool.n) continue;
      const FileRun& p = run_of(pool, j);
      const uint64_t pb = j - p.first;
      const uint64_t mine = block_len(r.size, bs, b);
      if (block_len(p.size, bs, pb) != mine) {
        ++st.dropped;  // the source index lies, or a digest collided
        continue;
      }
      src[g] = p.src;
      file[g] = p.file;
      block[g] = pb;
      ++st.found;
      st.bytes += mine;
    }
  }
  return st;
}

// One extent of cir_block_extents: `count` consecutive blocks of one need file
// whose copies are consecutive blocks of one source file (extents.hpp).
struct Extent {
  uint64_t first, count, need_file, need_block, src, src_file, src_block, bytes;
};
static_assert(sizeof(Extent) == 8 * extents::kRecWords, "an extent record is eight u64");

// map_matches' arrays to extents, in ascending `first`, and to the bitmap of
// the wanted blocks that were not found (fetch: ceil(need.n / 64) words, all
// written here; returns how many bits are set).  The continuation test is
// extents::cont, the one the kernels use.
inline uint64_t extents_of(const BlockList& need, uint64_t bs, const uint64_t* want,
                           const uint32_t* src, const uint64_t* file, const uint64_t* block,
                           std::vector<Extent>* out, uint64_t* fetch) {
  const uint64_t nwords = (need.n + 63) / 64;
  for (uint64_t w = 0; w < nwords; ++w) fetch[w] = 0;
  uint64_t left = 0;
  for (size_t r = 0; r < need.runs.size(); ++r) {
    const FileRun& run = need.runs[r];
    const uint64_t nb = extents::blocks_of(run.size, bs);
    bool open = false;  // out->back() ends at block b - 1 of this run
    for (uint64_t b = 0; b < nb; ++b) {
      const uint64_t g = run.first + b;
      const bool found = src[g] != kNone;
      const bool wanted = !want || (want[g >> 6] >> (g & 63) & 1);
      if (wanted && !found) {
        fetch[g >> 6] |= 1ull << (g & 63);
        ++left;
      }
      const uint64_t end = b * bs + block_len(run.size, bs, b);
      if (open && extents::cont(extents::kFound, r, src[g - 1], file[g - 1], block[g - 1],
                                found ? extents::kFound : 0, r, src[g], file[g], block[g])) {
        Extent& e = out->back();
        ++e.count;
        e.bytes = extents::extent_bytes(e.need_block, end, bs);
      } else if (found) {
        out->push_back(Extent{g, 1, run.file, b, src[g], file[g], block[g],
                              extents::extent_bytes(b, end, bs)});
      }
      open = found;
    }
  }
  return left;
}

// extents_of with its results handed over: *fetch (ceil(need.n / 64) words)
// and *rec (*count records; null when there is none) are malloc'd and the
// caller's, *left is extents_of's count.  False when memory ran out, with
// nothing allocated and nothing written to the four.
inline bool extents_owned(const BlockList& need, uint64_t bs, const uint64_t* want,
                          const uint32_t* src, const uint64_t* file, const uint64_t* block,
                          uint64_t** rec, size_t* count, uint64_t** fetch, uint64_t* left) {
  const uint64_t nwords = (need.n + 63) / 64;
  uint64_t* f = (uint64_t*)malloc((nwords ? nwords : 1) * sizeof(uint64_t));
  if (!f) return false;
  std::vector<Extent> ex;
  uint64_t l = 0;
  try {
    l = extents_of(need, bs, want, src, file, block, &ex, f);
  } catch (...) {
    free(f);
    throw;
  }
  uint64_t* r = nullptr;
  if (!ex.empty()) {
    r = (uint64_t*)malloc(ex.size() * sizeof(Extent));
    if (!r) {
      free(f);
      return false;
    }
    memcpy(r, ex.data(), ex.size() * sizeof(Extent));
  }
  *rec = r;
  *count = ex.size();
  *fetch = f;
  *left = l;
  return true;
}

// The run table of list as the kernels read it: four u64 per run {first,
// size, file, src} to out (4 x list.runs.size() words).
inline void pack_runs(const BlockList& list, uint64_t* out) {
  for (const FileRun& r : list.runs) {
    *out++ = r.first;
    *out++ = r.size;
    *out++ = r.file;
    *out++ = r.src;
  }
}

}  // namespace sources
}  // namespace cir
