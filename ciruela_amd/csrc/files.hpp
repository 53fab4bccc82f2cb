// The rule of cir_file_sources / cir_index_files_dev / cir_match_files_dev,
// written once for the host and the device: a file entry's record, its path
// decoded byte by byte, the path hash, the per-block fold term, and the host
// loops over the same rule.  No HIP runtime call; compiled by files.hip (the
// kernels), files.cpp and, with dirsig.cpp and links.cpp's rule under the
// sanitizers, by tools/files_fuzz.cpp.
//
// A file record is four u64 {name_off, dir_off, size, first | exe << 63}:
// name_off the text offset of the name's first byte, dir_off the offset of the
// '/' that starts the entry's directory line, `first` the global block number
// of its block 0 (for an empty file the number the next block would get).
// Both offsets point into an arena of texts; a path is never copied.
//
// Two file entries have the same path (dirsig.cpp: the decoded directory, a
// '/' unless the directory is "/", the decoded name) exactly when their
// decoded directories are equal and their decoded names are equal: a name
// holds no '/', and only the directory "/" ends the part before the last '/'
// empty.  Escapes are compared decoded: \x41 equals A.
//
// The candidate rule (links.cpp): for a need file the sources in order; a
// source matches when the first file entry it lists at that path has equal exe
// flag, size and digests.  The device compares a fold of the digests instead
// of the digests, and verifies the digests of every candidate afterwards: the
// fold only decides where the search stops, a difference found by the verify
// is status kCollision and the caller takes the host rule.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "idxscan.hpp"

namespace cir {
namespace files {

constexpr int kFileWords = 4;
constexpr int kResFields = 4;
constexpr int kFoldWords = 2;  // a file's fold is 128 bits
constexpr uint64_t kExeBit = 1ull << 63;
constexpr uint64_t kOk = 0, kCollision = 1;
constexpr uint32_t kNoSrc = 0xFFFFFFFFu;
constexpr uint64_t kNoFile = ~0ull;
constexpr uint64_t kMaxPoolFiles = 0x7FFFFFFFull;  // the table holds u32 ordinals + 1
constexpr uint64_t kMaxNeedFiles = 0xFFFFFFFFull;

struct Rec {
  uint64_t name_off, dir_off, size, first;  // first: with kExeBit
};

CIR_HD inline uint64_t mix64(uint64_t x, uint64_t w) {
  x = (x ^ w) * 0x9E3779B97F4A7C15ull;
  return x ^ (x >> 32);
}

// The decoded byte at *i of the token that ends before lim, *i advanced; -1 at
// the token's end (' ', '\n', lim, or an escape cut by lim).  A malformed
// escape (never in a text the acceptance rule took) decodes to some byte: no
// read leaves [0, lim).
CIR_HD inline int next_byte(const uint8_t* t, uint64_t* i, uint64_t lim) {
  if (*i >= lim) return -1;
  const uint8_t c = t[*i];
  if (c == ' ' || c == '\n') return -1;
  if (c == '\\') {
    if (lim - *i < 4) return -1;
    const int a = idxscan::hexval(t[*i + 2]), b = idxscan::hexval(t[*i + 3]);
    *i += 4;
    return ((a & 15) << 4) | (b & 15);
  }
  ++*i;
  return c;
}

// Where a walk from `off` stops at the latest: kMaxHead bytes on, or the
// arena's end.
CIR_HD inline uint64_t walk_lim(uint64_t off, uint64_t arena_len) {
  if (off >= arena_len) return off;  // nothing is read
  return arena_len - off > idxscan::kMaxHead ? off + idxscan::kMaxHead : arena_len;
}

// The path hash under a seed: the decoded directory bytes, a separator no byte
// equals, the decoded name bytes.
CIR_HD inline uint64_t path_hash(const uint8_t* t, uint64_t arena_len, uint64_t dir_off,
                                 uint64_t name_off, uint64_t seed) {
  uint64_t x = seed;
  uint64_t i = dir_off, lim = walk_lim(dir_off, arena_len);
  for (int c; (c = next_byte(t, &i, lim)) >= 0;) x = mix64(x, (uint64_t)c);
  x = mix64(x, 0x100);
  i = name_off;
  lim = walk_lim(name_off, arena_len);
  for (int c; (c = next_byte(t, &i, lim)) >= 0;) x = mix64(x, (uint64_t)c);
  return x;
}

// The home slot of (source ordinal, path) in a table of mask + 1 slots.
CIR_HD inline uint64_t home_slot(uint64_t phash, uint64_t src, uint64_t mask) {
  return mix64(phash, src + 0x517cc1b727220a95ull) & mask;
}

// Are the tokens at a (in ta) and b (in tb) equal once decoded?
CIR_HD inline bool same_token(const uint8_t* ta, uint64_t la, uint64_t a, const uint8_t* tb,
                              uint64_t lb, uint64_t b) {
  const uint64_t lima = walk_lim(a, la), limb = walk_lim(b, lb);
  for (;;) {
    const int x = next_byte(ta, &a, lima), y = next_byte(tb, &b, limb);
    if (x != y) return false;
    if (x < 0) return true;
  }
}

CIR_HD inline bool same_path(const uint8_t* ta, uint64_t la, uint64_t dir_a, uint64_t name_a,
                             const uint8_t* tb, uint64_t lb, uint64_t dir_b, uint64_t name_b) {
  return same_token(ta, la, name_a, tb, lb, name_b) && same_token(ta, la, dir_a, tb, lb, dir_b);
}

// Word w (0 or 1) of the fold term of a block: its position k in its file and
// its 32-byte digest (four little-endian u64) mixed under the seed.  A file's
// fold is the sum of its blocks' terms, per word, mod 2^64: the order of the
// additions does not matter, the order of the digests does.
CIR_HD inline uint64_t fold_term(uint64_t seed, uint64_t k, const uint64_t d[4], int w) {
  uint64_t x = mix64(w ? ~seed : seed, k + (w ? 0x6a09e667f3bcc908ull : 0xbb67ae8584caa73bull));
  x = mix64(x, d[0]);
  x = mix64(x, d[1]);
  x = mix64(x, d[2]);
  x = mix64(x, d[3]);
  return mix64(x, k);
}

CIR_HD inline uint64_t blocks_of(uint64_t size, uint64_t bs) { return size / bs + (size % bs != 0); }

// The exe flag of a file line whose head ends at hash_off (parse_head took
// it): behind the name stand ' ', the type, ' ' and the size digits.
CIR_HD inline bool exe_of(const uint8_t* t, uint64_t hash_off) {
  uint64_t q = hash_off;
  while (t[q - 1] >= '0' && t[q - 1] <= '9') --q;  // (at most 20 digits, a ' ' before them)
  return t[q - 2] == 'x';
}

struct Counts {
  uint64_t files = 0, blocks = 0;
  uint64_t declined = idxscan::kBad;  // start of the first declined line
};

// The host loop over the same rule: every body line through parse_head, in
// text order, a record per file entry (out may be null: count only).  Stops at
// the first declined line.  Tokens are not decoded here.
inline Counts scan_host(const uint8_t* t, uint64_t body_off, uint64_t body_end, uint64_t bs,
                        uint64_t off_bias, uint64_t block_bias, Rec* out) {
  Counts c;
  uint64_t p = body_off, dir = 0;
  if (p < body_end && t[p] != '/') {
    c.declined = p;
    return c;
  }
  while (p < body_end) {
    const idxscan::Head h = idxscan::parse_head(t, p, body_end, bs);
    if (h.kind == idxscan::kDecline) {
      c.declined = p;
      return c;
    }
    if (h.kind == idxscan::kFile) {
      if (out)
        out[c.files] = Rec{p + 2 + off_bias, dir + off_bias, h.size,
                           (c.blocks + block_bias) | (exe_of(t, h.hash_off) ? kExeBit : 0)};
      ++c.files;
      c.blocks += h.nblk;
      p = h.hash_off + idxscan::kTokenBytes * h.nblk + 1;
    } else {
      if (h.kind == idxscan::kDir) dir = p;
      while (t[p] != '\n') ++p;  // (parse_head saw the '\n' before body_end)
      ++p;
    }
  }
  return c;
}

inline uint64_t table_slots(uint64_t n_pool_files) {
  uint64_t s = 64;
  while (s < 2 * n_pool_files) s <<= 1;
  return s;
}

// One side of the join: an arena of texts, the file records over it and the
// flat digests the records' `first` count into.
struct Side {
  const uint8_t* text;
  uint64_t text_len;
  const Rec* recs;
  uint64_t nfiles;
  const uint8_t* digests;
  uint64_t nblocks;
};

// The source of pool file j: the last s with src_first[s] <= j (nsrc >= 1).
CIR_HD inline uint64_t src_of(const uint64_t* src_first, uint64_t nsrc, uint64_t j) {
  uint64_t lo = 0, hi = nsrc;  // invariant: src_first[lo] <= j < src_first[hi] where it holds at all
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (src_first[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

inline void load_digest(const uint8_t* base, uint64_t g, uint64_t d[4]) {
  __builtin_memcpy(d, base + 32 * g, 32);
}

// The host form of the device join: fold, build, probe, verify with the same
// hash, fold term and table discipline, one step after the other.  cand_src /
// cand_file: one entry per need file.  res: kResFields words.
inline void host_match(const Side& need, const Side& pool, const uint64_t* src_first, uint64_t nsrc,
                       uint64_t bs, const uint8_t* pool_verify, uint64_t seed, uint32_t* cand_src,
                       uint64_t* cand_file, uint64_t* res) {
  auto fold_side = [&](const Side& s, std::vector<uint64_t>* fold) {
    fold->assign(kFoldWords * s.nfiles, 0);
    for (uint64_t f = 0; f < s.nfiles; ++f) {
      const uint64_t first = s.recs[f].first & ~kExeBit, n = blocks_of(s.recs[f].size, bs);
      for (uint64_t k = 0; k < n && first + k < s.nblocks; ++k) {
        uint64_t d[4];
        load_digest(s.digests, first + k, d);
        for (int w = 0; w < kFoldWords; ++w) (*fold)[kFoldWords * f + w] += fold_term(seed, k, d, w);
      }
    }
  };
  std::vector<uint64_t> nf, pf;
  fold_side(need, &nf);
  fold_side(pool, &pf);
  const uint64_t slots = table_slots(pool.nfiles), mask = slots - 1;
  std::vector<uint32_t> table(slots, 0);  // pool ordinal + 1; 0 = empty
  for (uint64_t j = 0; j < pool.nfiles; ++j) {
    const Rec& r = pool.recs[j];
    const uint64_t s = src_of(src_first, nsrc, j);
    uint64_t at = home_slot(path_hash(pool.text, pool.text_len, r.dir_off, r.name_off, seed), s, mask);
    for (;; at = (at + 1) & mask) {
      if (table[at] == 0) {
        table[at] = (uint32_t)j + 1;
        break;
      }
      const uint64_t v = table[at] - 1;
      const Rec& o = pool.recs[v];
      if (src_of(src_first, nsrc, v) == s &&
          same_path(pool.text, pool.text_len, o.dir_off, o.name_off, pool.text, pool.text_len,
                    r.dir_off, r.name_off)) {
        if (v > j) table[at] = (uint32_t)j + 1;
        break;
      }
    }
  }
  res[0] = kOk;
  res[1] = res[2] = 0;
  res[3] = need.nfiles;
  for (uint64_t i = 0; i < need.nfiles; ++i) {
    const Rec& r = need.recs[i];
    const uint64_t ph = path_hash(need.text, need.text_len, r.dir_off, r.name_off, seed);
    cand_src[i] = kNoSrc;
    cand_file[i] = kNoFile;
    for (uint64_t s = 0; s < nsrc && cand_src[i] == kNoSrc; ++s) {
      uint64_t at = home_slot(ph, s, mask);
      for (uint64_t step = 0; step < slots && table[at]; ++step, at = (at + 1) & mask) {
        const uint64_t v = table[at] - 1;
        const Rec& o = pool.recs[v];
        if (src_of(src_first, nsrc, v) != s ||
            !same_path(pool.text, pool.text_len, o.dir_off, o.name_off, need.text, need.text_len,
                       r.dir_off, r.name_off))
          continue;
        if (o.size == r.size && ((o.first ^ r.first) & kExeBit) == 0 &&
            pf[kFoldWords * v] == nf[kFoldWords * i] &&
            pf[kFoldWords * v + 1] == nf[kFoldWords * i + 1]) {
          cand_src[i] = (uint32_t)s;
          cand_file[i] = v - src_first[s];
          ++res[1];
          res[2] += r.size;
        }
        break;  // the source's first entry at the path decides
      }
    }
    if (cand_src[i] == kNoSrc) continue;
    const uint64_t v = src_first[cand_src[i]] + cand_file[i];
    const uint64_t a = r.first & ~kExeBit, b = pool.recs[v].first & ~kExeBit;
    for (uint64_t k = 0, n = blocks_of(r.size, bs); k < n; ++k)
      if (a + k >= need.nblocks || b + k >= pool.nblocks ||
          __builtin_memcmp(need.digests + 32 * (a + k), pool_verify + 32 * (b + k), 32) != 0) {
        res[0] = kCollision;
        break;
      }
  }
}

}  // namespace files
}  // namespace cir
