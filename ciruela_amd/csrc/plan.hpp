// The rule of cir_fetch_plan, written once: the download plan of a new image as
// the composition of the four calls that each answer a part of it.  Header-only
// and free of HIP (the way copies.hpp, extents.hpp and repeats.hpp hold
// theirs): the kernels (plan.hip), the host path (plan.cpp) and the fuzz
// (tools/plan_fuzz.cpp) all use this text.  The composed rules themselves are
// files.hpp / links.hpp (cir_file_sources), copies.hpp (cir_file_copies),
// sources.hpp + extents.hpp (cir_block_extents) and repeats.hpp
// (cir_block_repeats); none of them changes here.
//
// Inputs: the new index, the sources in the caller's order, and two optional
// bitmaps in the usual layout (bit i & 63 of word i >> 6):
//   deny  over file ordinals: no whole-file link may be proposed for these;
//   have  over global blocks: already present and correct.
//
//   1. L1 = cir_file_sources' candidates, minus the files in deny.
//   2. L2 = cir_file_copies with skip = deny | files(L1).
//   3. linked = files(L1) | files(L2).  want1 = every block of a file entry
//      that is not linked, minus the 1-bits of have.
//   4. (E1, fetch1) = cir_block_extents with want = want1.
//   5. (E2, fetch2) = cir_block_repeats with want = fetch1 and present = every
//      block not in fetch1: the linked files' blocks, the have blocks and the
//      blocks E1 covers are all in place before any copy inside the image.
//
// The glue between the calls is what this header states: which candidates deny
// withdraws and the skip word of step 2 (k_plan_links), and the class of a
// block in step 3 (k_plan_want).  A block's file is found by bisecting the need
// run table (idxscan::Run / sources::pack_runs: four u64 per non-empty file
// {first, size, file, x}, `first` ascending).  A table that is sorted but lies
// gets the answer these functions define; nothing outside the arrays as sized
// by the arguments is read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CIR_PLAN_HD __host__ __device__ inline
#else
#define CIR_PLAN_HD inline
#endif

namespace cir {
namespace plan {

constexpr uint32_t kNoSrc = 0xFFFFFFFFu;  // files::kNoSrc
constexpr uint64_t kNoFile = ~0ull;       // files::kNoFile
constexpr int kRunWords = 4;
constexpr int kLinksResFields = 2;  // {candidates kept, withdrawn}
constexpr int kWantResFields = 3;   // {blocks wanted, blocks of linked files, left out by have}
constexpr uint64_t kNoRun = ~0ull;

// Bit i of a nullable bitmap (null: every bit is 0).
CIR_PLAN_HD bool bit(const uint64_t* map, uint64_t i) {
  return map && ((map[i >> 6] >> (i & 63)) & 1);
}

// Step 1: is same-path candidate `cand` of file i withdrawn by deny?
CIR_PLAN_HD bool withdrawn(const uint64_t* deny, uint64_t i, uint32_t cand) {
  return cand != kNoSrc && bit(deny, i);
}
// Step 2: file i's bit in cir_file_copies' skip: denied, or linked at its own path.
CIR_PLAN_HD bool skip_bit(const uint64_t* deny, uint64_t i, uint32_t cand) {
  return cand != kNoSrc || bit(deny, i);
}

// Blocks of a file of `size` bytes; no overflow at size = 2^64 - 1.
CIR_PLAN_HD uint64_t blocks_of(uint64_t size, uint64_t bs) { return size / bs + (size % bs != 0); }

// The last run with first <= g, or kNoRun.  At most 64 steps for any n_runs.
CIR_PLAN_HD uint64_t run_at(const uint64_t* runs, uint64_t n_runs, uint64_t g) {
  uint64_t lo = 0, hi = n_runs;  // runs[< lo].first <= g < runs[>= hi].first
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (runs[kRunWords * mid] <= g)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : kNoRun;
}

enum Class : int { kOutside = 0, kLinked = 1, kHave = 2, kWanted = 3 };

// Step 3: the class of block g.  cand_a / cand_b: the candidate source of every
// need file after steps 1 and 2 (n_files u32 each, kNoSrc: none); either may be
// null.  A run's file ordinal is checked against n_files before either is read.
CIR_PLAN_HD Class class_of(const uint64_t* runs, uint64_t n_runs, uint64_t bs, uint64_t n_files,
                           const uint32_t* cand_a, const uint32_t* cand_b, const uint64_t* have,
                           uint64_t g) {
  const uint64_t r = run_at(runs, n_runs, g);
  if (r == kNoRun) return kOutside;
  const uint64_t first = runs[kRunWords * r], size = runs[kRunWords * r + 1];
  const uint64_t f = runs[kRunWords * r + 2];
  if (g - first >= blocks_of(size, bs)) return kOutside;
  if (f < n_files && ((cand_a && cand_a[f] != kNoSrc) || (cand_b && cand_b[f] != kNoSrc)))
    return kLinked;
  return bit(have, g) ? kHave : kWanted;
}

// ---- the host forms of the two kernels ------------------------------------------

// k_plan_links: withdraws what deny forbids, writes every word of skip
// [0, ceil(n_files / 64)) with the bits at and past n_files 0, and counts.
inline void links_host(const uint64_t* deny, uint64_t n_files, uint32_t* cand_src,
                       uint64_t* cand_file, uint64_t* skip, uint64_t res[kLinksResFields]) {
  res[0] = res[1] = 0;
  for (uint64_t w = 0; w < (n_files + 63) / 64; ++w) skip[w] = 0;
  for (uint64_t i = 0; i < n_files; ++i) {
    if (skip_bit(deny, i, cand_src[i])) skip[i >> 6] |= 1ull << (i & 63);
    if (withdrawn(deny, i, cand_src[i])) {
      cand_src[i] = kNoSrc;
      cand_file[i] = kNoFile;
      ++res[1];
    } else if (cand_src[i] != kNoSrc) {
      ++res[0];
    }
  }
}

// k_plan_want: every word of want [0, ceil(n_blocks / 64)), bits at and past
// n_blocks 0, and the counts.
inline void want_host(const uint64_t* runs, uint64_t n_runs, uint64_t n_blocks, uint64_t bs,
                      uint64_t n_files, const uint32_t* cand_a, const uint32_t* cand_b,
                      const uint64_t* have, uint64_t* want, uint64_t res[kWantResFields]) {
  res[0] = res[1] = res[2] = 0;
  for (uint64_t w = 0; w < (n_blocks + 63) / 64; ++w) want[w] = 0;
  for (uint64_t g = 0; g < n_blocks; ++g) {
    const Class c = class_of(runs, n_runs, bs, n_files, cand_a, cand_b, have, g);
    if (c == kWanted) {
      want[g >> 6] |= 1ull << (g & 63);
      ++res[0];
    } else if (c == kLinked) {
      ++res[1];
    } else if (c == kHave) {
      ++res[2];
    }
  }
}

// Step 5's `present` on the host: every block below n that is not in fetch1.
// (On the device an all-ones bitmap serves: see plan.cpp.)
inline void present_host(const uint64_t* fetch1, uint64_t n_blocks, uint64_t* present) {
  for (uint64_t w = 0; w < (n_blocks + 63) / 64; ++w) present[w] = ~fetch1[w];
  if (n_blocks & 63) present[n_blocks >> 6] &= (1ull << (n_blocks & 63)) - 1;
}

}  // namespace plan
}  // namespace cir

#if !defined(__HIPCC__)
// The host side: the composition itself, over whatever answers the four calls.
#include <stdlib.h>

#include <vector>

namespace cir {
namespace plan {

constexpr int kStatsFields = 44;
// Where the composed calls' stats stand in the plan's, and the plan's own.
constexpr int kStatSources = 0, kStatCopies = 8, kStatExtents = 18, kStatRepeats = 28;
constexpr int kStatWithdrawn = 38, kStatLinked = 39, kStatLinkedBlocks = 40, kStatHave = 41;
constexpr int kStatDevice = 42, kStatWhy = 43;

// The new index as step 3 needs it: the packed need run table and the counts.
struct Layout {
  std::vector<uint64_t> runs;  // kRunWords per non-empty file
  uint64_t n_files = 0, n_blocks = 0, bs = 0;
};

// A plan's outputs; every pointer is malloc'd, null when its count is 0.
struct Result {
  uint64_t* link_file = nullptr;
  uint32_t* link_src = nullptr;
  size_t nlinks = 0;
  uint64_t* copy_file = nullptr;
  uint32_t* copy_src = nullptr;
  uint64_t* copy_src_file = nullptr;
  uint64_t* copy_path_off = nullptr;
  uint8_t* copy_paths = nullptr;
  size_t ncopies = 0;
  uint64_t* extents = nullptr;
  size_t nextents = 0;
  uint64_t* repeats = nullptr;
  size_t nrepeats = 0;
  uint64_t* fetch = nullptr;
  uint64_t nblk = 0;
  size_t nskipped = 0;
  uint64_t stats[kStatsFields] = {};
  void drop() {  // on error: every output null / 0 and the stats zero
    for (void* p : {(void*)link_file, (void*)link_src, (void*)copy_file, (void*)copy_src,
                    (void*)copy_src_file, (void*)copy_path_off, (void*)copy_paths, (void*)extents,
                    (void*)repeats, (void*)fetch})
      free(p);
    *this = Result();
  }
};

// The composition on the host.  `sib` answers the four calls (each as its C
// entry point with ctx = NULL does: 0 or a negative code, outputs malloc'd)
// and lays the new index out; the glue is links_host, want_host and
// present_host.  Errors are the first the composition meets; on error *r is
// dropped.
template <class Sib>
int plan_host(Sib& sib, const uint64_t* deny, const uint64_t* have, Result* r) {
  *r = Result();
  Layout lay;
  uint64_t* fetch1 = nullptr;
  auto fail_with = [&](int rc) {
    free(fetch1);
    r->drop();
    return rc;
  };
  int rc;
  if ((rc = sib.layout(&lay))) return fail_with(rc);
  const uint64_t nf = lay.n_files, nb = lay.n_blocks;
  // 1. the same-path candidates, minus deny
  if ((rc = sib.file_sources(&r->link_file, &r->link_src, &r->nlinks, &r->nskipped,
                             r->stats + kStatSources)))
    return fail_with(rc);
  std::vector<uint32_t> ca(nf, kNoSrc), cb(nf, kNoSrc);
  std::vector<uint64_t> cf(nf, kNoFile), skip((nf + 63) / 64 + 1);
  for (size_t k = 0; k < r->nlinks; ++k)
    if (r->link_file[k] < nf) ca[r->link_file[k]] = r->link_src[k];
  uint64_t lres[kLinksResFields];
  links_host(deny, nf, ca.data(), cf.data(), skip.data(), lres);
  size_t kept = 0;
  for (size_t k = 0; k < r->nlinks; ++k)
    if (r->link_file[k] < nf && ca[r->link_file[k]] != kNoSrc) {
      r->link_file[kept] = r->link_file[k];
      r->link_src[kept++] = r->link_src[k];
    }
  r->nlinks = kept;
  if (!kept) {
    free(r->link_file);
    free(r->link_src);
    r->link_file = nullptr;
    r->link_src = nullptr;
  }
  // 2. the content candidates of what is left
  size_t skipped2 = 0;
  if ((rc = sib.file_copies(skip.data(), &r->copy_file, &r->copy_src, &r->copy_src_file,
                            &r->copy_path_off, &r->copy_paths, &r->ncopies, &skipped2,
                            r->stats + kStatCopies)))
    return fail_with(rc);
  for (size_t k = 0; k < r->ncopies; ++k)
    if (r->copy_file[k] < nf) cb[r->copy_file[k]] = r->copy_src[k];
  // 3. the blocks still wanted
  std::vector<uint64_t> want((nb + 63) / 64 + 1), present((nb + 63) / 64 + 1);
  uint64_t wres[kWantResFields];
  want_host(lay.runs.data(), lay.runs.size() / kRunWords, nb, lay.bs ? lay.bs : 1, nf, ca.data(),
            cb.data(), have, want.data(), wres);
  // 4. their local copies
  uint64_t nblk1 = 0;
  size_t skipped3 = 0;
  if ((rc = sib.block_extents(want.data(), &r->extents, &r->nextents, &fetch1, &nblk1, &skipped3,
                              r->stats + kStatExtents)))
    return fail_with(rc);
  // 5. the repeats inside the image among what is still to fetch
  if (fetch1) present_host(fetch1, nb, present.data());
  if ((rc = sib.block_repeats(fetch1 ? fetch1 : want.data(), present.data(), &r->repeats,
                              &r->nrepeats, &r->fetch, &r->nblk, r->stats + kStatRepeats)))
    return fail_with(rc);
  free(fetch1);
  fetch1 = nullptr;
  r->stats[kStatWithdrawn] = lres[1];
  r->stats[kStatLinked] = lres[0] + r->ncopies;
  r->stats[kStatLinkedBlocks] = wres[1];
  r->stats[kStatHave] = wres[2];
  return 0;
}

}  // namespace plan
}  // namespace cir
#endif
