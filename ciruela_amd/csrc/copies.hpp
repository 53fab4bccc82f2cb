// The rule of cir_file_copies / cir_match_copies_dev, written once for the
// host and the device: which need files take part, the key of the table, and
// the host form of the device join; and the compaction of the device's
// content candidates into the caller's arrays (Found, compact), the one piece
// of host code that trusts nothing the device wrote, shared by cir_file_copies
// and cir_fetch_plan.  No HIP runtime call; compiled by files.hip (the
// kernels), copies.cpp, plan.cpp and, under the sanitizers, by
// tools/copies_fuzz.cpp.  Records, fold term and src_of are files.hpp's.
//
// The rule.  Pool files are ordered by source in the order given, then in
// index order.  Need file i has a candidate only if its size is greater than 0
// and its bit in the caller's skip bitmap (u64 words over file ordinals; null:
// nothing skipped) is 0.  The candidate is the pool file with the smallest
// pool ordinal that has equal exe flag, equal size and an equal digest list,
// at any path: the first source that holds such a file and, inside it, its
// first place.  Empty files take part on neither side.
//
// How the device decides, and why that is the rule.  The table is keyed by
// {size, exe, the 128-bit fold of the digest list under the call's seed}
// (files::fold_term).  A slot is claimed by CAS on empty and lowered by
// atomicMin by every later pool file whose key equals the occupant's (compared
// through the occupant's record and fold), so every occupant a slot ever has
// carries the same key, and the slot ends holding the smallest ordinal among
// the pool files with that key -- whatever the order of arrival.  Files of
// equal content have equal keys, so the pool files equal to a need file are a
// subset of those that share its slot.  Every candidate is then verified
// digest by digest.  If every verify passes, each candidate is equal to its
// need file and is the minimum of a superset of the files equal to it, hence
// the minimum of those; and a need file whose key is in no slot has no equal
// pool file.  A fold collision can therefore only make a slot's minimum a file
// that fails the verify: status kCollision, and the caller takes the host
// rule.  With kOk the answer is exactly the host rule's, whatever the seed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "decode.hpp"
#include "files.hpp"

namespace cir {
namespace copies {

constexpr int kPlaceWords = 2;  // {name_off, dir_off} of a candidate's pool record
constexpr uint64_t kNoPlace = ~0ull;

// Is need file i left out by the caller's bitmap?
CIR_HD inline bool skipped(const uint64_t* skip, uint64_t i) {
  return skip && ((skip[i >> 6] >> (i & 63)) & 1);
}

// The home slot of a key in a table of mask + 1 slots.  exe: 0 or kExeBit.
CIR_HD inline uint64_t home_slot(uint64_t size, uint64_t exe, uint64_t f0, uint64_t f1,
                                 uint64_t seed, uint64_t mask) {
  uint64_t x = files::mix64(seed, size);
  x = files::mix64(x, f0 + (exe ? 0x243f6a8885a308d3ull : 0));
  return files::mix64(x, f1) & mask;
}

CIR_HD inline bool same_key(uint64_t size_a, uint64_t first_a, uint64_t a0, uint64_t a1,
                            uint64_t size_b, uint64_t first_b, uint64_t b0, uint64_t b1) {
  return size_a == size_b && ((first_a ^ first_b) & files::kExeBit) == 0 && a0 == b0 && a1 == b1;
}

// The host form of the device join: fold, build, probe, verify with the same
// key, fold term and table discipline, one step after the other.  The sides'
// texts are not read.  cand_src / cand_file: one entry per need file;
// cand_place: kPlaceWords per need file; res: files::kResFields words {status,
// candidates, their bytes, need files}.
inline void host_match(const files::Side& need, const files::Side& pool, const uint64_t* src_first,
                       uint64_t nsrc, uint64_t bs, const uint64_t* skip, const uint8_t* pool_verify,
                       uint64_t seed, uint32_t* cand_src, uint64_t* cand_file, uint64_t* cand_place,
                       uint64_t* res) {
  using files::kExeBit;
  using files::kFoldWords;
  auto fold_side = [&](const files::Side& s, std::vector<uint64_t>* fold) {
    fold->assign(kFoldWords * s.nfiles, 0);
    for (uint64_t f = 0; f < s.nfiles; ++f) {
      const uint64_t first = s.recs[f].first & ~kExeBit, n = files::blocks_of(s.recs[f].size, bs);
      for (uint64_t k = 0; k < n && first + k < s.nblocks; ++k) {
        uint64_t d[4];
        files::load_digest(s.digests, first + k, d);
        for (int w = 0; w < kFoldWords; ++w)
          (*fold)[kFoldWords * f + w] += files::fold_term(seed, k, d, w);
      }
    }
  };
  std::vector<uint64_t> nf, pf;
  fold_side(need, &nf);
  fold_side(pool, &pf);
  const uint64_t slots = files::table_slots(pool.nfiles), mask = slots - 1;
  std::vector<uint32_t> table(slots, 0);  // pool ordinal + 1; 0 = empty
  for (uint64_t j = 0; j < pool.nfiles && nsrc; ++j) {
    const files::Rec& r = pool.recs[j];
    if (r.size == 0) continue;
    uint64_t at = home_slot(r.size, r.first & kExeBit, pf[2 * j], pf[2 * j + 1], seed, mask);
    for (;; at = (at + 1) & mask) {
      if (table[at] == 0) {
        table[at] = (uint32_t)j + 1;
        break;
      }
      const uint64_t v = table[at] - 1;
      const files::Rec& o = pool.recs[v];
      if (same_key(o.size, o.first, pf[2 * v], pf[2 * v + 1], r.size, r.first, pf[2 * j],
                   pf[2 * j + 1])) {
        if (v > j) table[at] = (uint32_t)j + 1;
        break;
      }
    }
  }
  res[0] = files::kOk;
  res[1] = res[2] = 0;
  res[3] = need.nfiles;
  for (uint64_t i = 0; i < need.nfiles; ++i) {
    const files::Rec& r = need.recs[i];
    cand_src[i] = files::kNoSrc;
    cand_file[i] = files::kNoFile;
    cand_place[kPlaceWords * i] = cand_place[kPlaceWords * i + 1] = kNoPlace;
    if (r.size == 0 || skipped(skip, i) || nsrc == 0) continue;
    uint64_t at = home_slot(r.size, r.first & kExeBit, nf[2 * i], nf[2 * i + 1], seed, mask);
    for (uint64_t step = 0; step < slots && table[at]; ++step, at = (at + 1) & mask) {
      const uint64_t v = table[at] - 1;
      const files::Rec& o = pool.recs[v];
      if (!same_key(o.size, o.first, pf[2 * v], pf[2 * v + 1], r.size, r.first, nf[2 * i],
                    nf[2 * i + 1]))
        continue;
      const uint64_t s = files::src_of(src_first, nsrc, v);
      cand_src[i] = (uint32_t)s;
      cand_file[i] = v - src_first[s];
      cand_place[kPlaceWords * i] = o.name_off;
      cand_place[kPlaceWords * i + 1] = o.dir_off;
      ++res[1];
      res[2] += r.size;
      break;
    }
    if (cand_src[i] == files::kNoSrc) continue;
    const uint64_t v = src_first[cand_src[i]] + cand_file[i];
    const uint64_t a = r.first & ~kExeBit, b = pool.recs[v].first & ~kExeBit;
    for (uint64_t k = 0, n = files::blocks_of(r.size, bs); k < n; ++k)
      if (a + k >= need.nblocks || b + k >= pool.nblocks ||
          __builtin_memcmp(need.digests + 32 * (a + k), pool_verify + 32 * (b + k), 32) != 0) {
        res[0] = files::kCollision;
        break;
      }
  }
}

// A malloc'd copy of p[0, n) for the caller; null when n == 0.
template <class T>
bool dup(const T* p, size_t n, T** out) {
  *out = n ? (T*)malloc(n * sizeof(T)) : nullptr;
  if (*out) memcpy(*out, p, n * sizeof(T));
  return !n || *out != nullptr;
}

// The content candidates of a call, before they become the caller's arrays.
struct Found {
  std::vector<uint64_t> file, src_file, path_off{0};
  std::vector<uint32_t> src;
  std::string paths;
  uint64_t left_out = 0, same = 0;  // need files the bitmap skips; candidates at their own path
  void reserve(size_t n) {
    file.reserve(n);
    src.reserve(n);
    src_file.reserve(n);
    path_off.reserve(n + 1);
    paths.reserve(48 * n);
  }
  void add(uint64_t f, uint32_t s, uint64_t sf) {  // (its path was appended to `paths`)
    file.push_back(f);
    src.push_back(s);
    src_file.push_back(sf);
    path_off.push_back(paths.size());
  }
  // The five arrays malloc'd for the caller, all null when there is no
  // candidate; false, and all null, when a malloc fails.
  bool give(uint64_t** file_out, uint32_t** src_out, uint64_t** src_file_out,
            uint64_t** path_off_out, uint8_t** paths_out) const {
    const size_t n = file.size();
    *file_out = *src_file_out = *path_off_out = nullptr;
    *src_out = nullptr;
    *paths_out = nullptr;
    if (dup(file.data(), n, file_out) && dup(src.data(), n, src_out) &&
        dup(src_file.data(), n, src_file_out) &&
        dup(path_off.data(), n ? n + 1 : 0, path_off_out) &&
        dup((const uint8_t*)paths.data(), paths.size(), paths_out))
      return true;
    for (void* p : {(void*)*file_out, (void*)*src_out, (void*)*src_file_out, (void*)*path_off_out,
                    (void*)*paths_out})
      free(p);
    *file_out = *src_file_out = *path_off_out = nullptr;
    *src_out = nullptr;
    *paths_out = nullptr;
    return false;
  }
};

// One text of a call as compact() reads it: its bytes on the host, where it
// stands in the device's text arena (from whose start the records' offsets
// count), its file entries, and the source's ordinal as the caller counts.
struct PlacedText {
  const uint8_t* p;
  uint64_t len, text_off, nfiles;
  uint32_t ordinal;
};

enum Compacted { kCompacted = 0, kBadSource, kBadPlace };

// The join's downloaded answer (cand_src, cand_file, need_recs: one entry per
// need file; cand_place: kPlaceWords) into `found`, each candidate's path
// decoded from its source's text; found->left_out counts the 1-bits of `skip`
// (null: none).  text[0] is the need's, text[1 + s] source s of `used`.
// Nothing the device wrote is trusted: a source >= used is kBadSource, a file
// >= the source's nfiles or a place of either side outside its text kBadPlace,
// and nothing is read outside the texts and the arrays.
inline Compacted compact(const uint32_t* cand_src, const uint64_t* cand_file,
                         const uint64_t* cand_place, const files::Rec* need_recs,
                         uint64_t need_files, const PlacedText* text, size_t used,
                         const uint64_t* skip, Found* found) {
  const PlacedText& ni = text[0];
  for (uint64_t i = 0; i < need_files; ++i) {
    found->left_out += skipped(skip, i);
    if (cand_src[i] == files::kNoSrc) continue;
    if (cand_src[i] >= used) return kBadSource;
    const PlacedText& it = text[1 + cand_src[i]];
    const uint64_t name = cand_place[kPlaceWords * i] - it.text_off;
    const uint64_t dir = cand_place[kPlaceWords * i + 1] - it.text_off;
    const uint64_t nname = need_recs[i].name_off - ni.text_off;
    const uint64_t ndir = need_recs[i].dir_off - ni.text_off;
    if (name >= it.len || dir >= it.len || nname >= ni.len || ndir >= ni.len ||
        cand_file[i] >= it.nfiles)
      return kBadPlace;
    decode_path(it.p, it.len, dir, name, &found->paths);
    found->add(i, it.ordinal, cand_file[i]);
    found->same += files::same_path(ni.p, ni.len, ndir, nname, it.p, it.len, dir, name);
  }
  return kCompacted;
}

}  // namespace copies
}  // namespace cir
