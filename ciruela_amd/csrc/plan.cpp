// cir_fetch_plan: what to link, what to copy and what to fetch for a new image,
// in one call; cir_plan_links_dev and cir_plan_want_dev, the device-resident
// glue behind it.
//
// The reference plans nothing: scan_links (src/daemon/metadata/
// hardlink_sources.rs:107-153) links whole files at their own path and
// fill_blocks (src/daemon/tracking/progress.rs:129-170) queues every block of
// every other file.  cir_file_sources, cir_file_copies, cir_block_extents and
// cir_block_repeats each answer a part of the question; a caller had to make
// the four calls and glue them with host loops, and every call framed,
// uploaded and parsed the same texts again.  The plan is defined as their
// composition (plan.hpp) and computed here with every text uploaded and parsed
// once: the four joins run back to back in device memory, with plan.hip's two
// kernels between them.
//
// The device flow goes through devcall.hpp like copies.cpp's: FileStage frames
// and uploads the texts, the count pass (first synchronise), the emit and
// decode passes into shared digest and record buffers; then, here,
// launch_match_files, k_plan_links, launch_match_copies, k_plan_want; the run
// tables, the verdicts and the candidates come down (second synchronise); the
// host packs the run tables; launch_join, launch_extent_map, launch_repeat_join and
// launch_extent_map again run behind one upload (third synchronise, for the two
// extent counts), and two extent tails bring the records down (fourth and
// fifth).  Whatever the device cannot answer exactly is answered by the host
// composition, plan::plan_host over the siblings with ctx = NULL.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "copies.hpp"
#include "devcall.hpp"
#include "dirsig.hpp"
#include "files.hpp"
#include "idxscan.hpp"
#include "plan.hpp"
#include "repeats.hpp"
#include "runtime.hpp"
#include "sources.hpp"

namespace cir {
namespace {

static_assert(CIR_PLAN_STATS_FIELDS == plan::kStatsFields, "the header's stats");
static_assert(CIR_PLAN_LINKS_RES_FIELDS == plan::kLinksResFields &&
                  CIR_PLAN_WANT_RES_FIELDS == plan::kWantResFields,
              "the header's result words");
static_assert(plan::kStatCopies == CIR_FILE_SOURCES_STATS_FIELDS &&
                  plan::kStatExtents == plan::kStatCopies + CIR_FILE_COPIES_STATS_FIELDS &&
                  plan::kStatRepeats == plan::kStatExtents + CIR_EXTENTS_STATS_FIELDS &&
                  plan::kStatWithdrawn == plan::kStatRepeats + CIR_REPEATS_STATS_FIELDS,
              "the siblings' stats stand one behind the other");
static_assert(plan::kNoSrc == files::kNoSrc && plan::kNoFile == files::kNoFile &&
                  plan::kRunWords * sizeof(uint64_t) == sizeof(idxscan::Run),
              "the rule's constants are the siblings'");

uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

int plan_links_dev_impl(const uint64_t* d_deny, uint64_t n_files, uint32_t* d_cand_src,
                        uint64_t* d_cand_file, uint64_t* d_skip, uint64_t* d_res, void* stream) {
  if (!d_res || (n_files && (!d_cand_src || !d_cand_file || !d_skip)))
    return fail(CIR_EINVAL, "null device pointer");
  if ((addr(d_deny) | addr(d_cand_file) | addr(d_skip) | addr(d_res)) & 7u)
    return fail(CIR_EINVAL, "d_deny, d_cand_file, d_skip and result must be 8-byte aligned");
  if (addr(d_cand_src) & 3u) return fail(CIR_EINVAL, "d_cand_src must be 4-byte aligned");
  if (n_files > files::kMaxNeedFiles) return fail(CIR_EINVAL, "more than 2^32-1 need files");
  CIR_HIP(dev::launch_plan_links(d_deny, n_files, d_cand_src, d_cand_file, d_skip, d_res,
                                 (hipStream_t)stream));
  return CIR_OK;
}

int plan_want_dev_impl(const uint64_t* d_need_runs, uint64_t n_need_runs, uint64_t n_blocks,
                       uint64_t bs, uint64_t n_files, const uint32_t* d_cand_a,
                       const uint32_t* d_cand_b, const uint64_t* d_have, uint64_t* d_want,
                       uint64_t* d_res, void* stream) {
  if (!d_res || (n_need_runs && !d_need_runs) || (n_blocks && !d_want))
    return fail(CIR_EINVAL, "null device pointer");
  if ((addr(d_need_runs) | addr(d_have) | addr(d_want) | addr(d_res)) & 7u)
    return fail(CIR_EINVAL, "run table, bitmaps and result must be 8-byte aligned");
  if ((addr(d_cand_a) | addr(d_cand_b)) & 3u)
    return fail(CIR_EINVAL, "candidate arrays must be 4-byte aligned");
  if (bs == 0) return fail(CIR_EINVAL, "block_size is 0");
  if (n_blocks > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 blocks");
  if (n_need_runs > 0xFFFFFFFFull) return fail(CIR_EINVAL, "more than 2^32-1 runs");
  if (n_files > files::kMaxNeedFiles) return fail(CIR_EINVAL, "more than 2^32-1 need files");
  CIR_HIP(dev::launch_plan_want(d_need_runs, n_need_runs, n_blocks, bs, n_files, d_cand_a, d_cand_b,
                                d_have, d_want, d_res, (hipStream_t)stream));
  return CIR_OK;
}

// ---- the whole call ------------------------------------------------------------

bool plan_on_host() {  // CIR_PLAN=host, read per call
  const char* v = getenv("CIR_PLAN");
  return v && strcmp(v, "host") == 0;
}

struct Inputs {
  const uint8_t* index;
  size_t len;
  const uint8_t* const* src_index;
  const size_t* src_len;
  size_t nsrc;
  const uint64_t* deny;
  const uint64_t* have;
};

// The four calls of the composition with ctx = NULL: their host rules.
struct HostSiblings {
  const Inputs& in;
  int layout(plan::Layout* lay) const {
    dirsig::Index idx;
    std::string err;
    if (!dirsig::parse(in.index, in.len, &idx, &err)) return parse_fail(idx.bad_hash_size, err);
    sources::BlockList need;
    sources::append_runs(idx, 0, &need);
    for (const dirsig::Entry& en : idx.entries) lay->n_files += en.kind == dirsig::EntryKind::kFile;
    lay->n_blocks = need.n;
    lay->bs = idx.header.block_size;
    lay->runs.resize(plan::kRunWords * need.runs.size());
    sources::pack_runs(need, lay->runs.data());
    return CIR_OK;
  }
  int file_sources(uint64_t** file, uint32_t** src, size_t* n, size_t* nskipped,
                   uint64_t* stats) const {
    return cir_file_sources(nullptr, in.index, in.len, in.src_index, in.src_len, in.nsrc, file, src,
                            n, nskipped, stats);
  }
  int file_copies(const uint64_t* skip, uint64_t** file, uint32_t** src, uint64_t** src_file,
                  uint64_t** path_off, uint8_t** paths, size_t* n, size_t* nskipped,
                  uint64_t* stats) const {
    return cir_file_copies(nullptr, in.index, in.len, in.src_index, in.src_len, in.nsrc, skip, file,
                           src, src_file, path_off, paths, n, nskipped, stats);
  }
  int block_extents(const uint64_t* want, uint64_t** ext, size_t* next, uint64_t** fetch,
                    uint64_t* nblk, size_t* nskipped, uint64_t* stats) const {
    return cir_block_extents(nullptr, in.index, in.len, in.src_index, in.src_len, in.nsrc, want,
                             ext, next, fetch, nblk, nskipped, stats);
  }
  int block_repeats(const uint64_t* want, const uint64_t* present, uint64_t** ext, size_t* next,
                    uint64_t** fetch, uint64_t* nblk, uint64_t* stats) const {
    return cir_block_repeats(nullptr, in.index, in.len, want, present, ext, next, fetch, nblk,
                             stats);
  }
};

using copies::dup;

// With a context: on its first device, under that device's lock.  Returns a
// CIR_* code (with *r dropped on failure), or kHostFlow (devcall.hpp: here the
// host composition decides the call) with *why set and nothing reported.
int fetch_plan_dev(cir_ctx* ctx, const Inputs& in, plan::Result* r, bool trace, uint64_t* why) {
  if (ctx->devs.empty()) return fail(CIR_EINVAL, "context without a device");
  const auto t0 = Clock::now();
  // host memory that asynchronous copies read or write: declared before the call
  FileStage stage;
  std::vector<uint32_t> c1src, c2src;
  std::vector<uint64_t> c2file, c2place, tabs;
  std::vector<files::Rec> nrec;
  uint64_t m1_res[files::kResFields] = {0, 0, 0, 0}, m2_res[files::kResFields] = {0, 0, 0, 0};
  uint64_t l_res[plan::kLinksResFields] = {0, 0}, w_res[plan::kWantResFields] = {0, 0, 0};
  uint64_t x1_res[extents::kResFields] = {0, 0, 0, 0, 0, 0};
  uint64_t x2_res[extents::kResFields] = {0, 0, 0, 0, 0, 0};
  TraceEvents<5> ev;   // around the two file joins and the glue behind each
  TraceEvents<5> xev;  // around the two block joins and their extent maps
  int rc;
  if ((rc = stage.frame(in.index, in.len, in.src_index, in.src_len, in.nsrc, why))) return rc;

  DeviceCall c(ctx);
  hipStream_t s = c.s;
  if ((rc = c.begin()) || (rc = stage.count(c, trace, why))) return rc;
  const TextSet& ts = stage.ts;
  const std::vector<FileStage::Text>& tx = stage.tx;
  const auto t1 = ts.t_bufs, t2 = ts.t_up, t3 = ts.t_counted;
  const uint64_t bs = stage.h.block_size, pool_files = stage.pool_files;
  const uint64_t pool_blocks = stage.pool_blocks, need_files = stage.need_files();
  const uint64_t n = stage.need_blocks(), need_runs = ts.item[0].cnt[2];
  const size_t nt = tx.size(), used = stage.used;
  const uint64_t file_words = (need_files + 63) / 64, nwords = (n + 63) / 64;
  // (the block joins' limits are narrower than the stage's: the pool's ordinals
  // are u32 below 2^31, and the repeats' pool is the need list twice)
  if (!sources::pool_count_ok(pool_blocks) || n > repeats::kMaxBlocks)
    return kHostFlow;  // (*why is CIR_FILE_WHY_LIMIT)
  if (n == 0) {  // nothing to join block by block: the composition ends in its host rules
    *why = CIR_PLAN_WHY_EMPTY;
    return kHostFlow;
  }
  uint64_t* d_deny = nullptr;
  uint64_t* d_have = nullptr;
  uint64_t* d_skip = nullptr;
  uint64_t* d_mwork = nullptr;
  uint32_t* d_c1src = nullptr;
  uint64_t* d_c1file = nullptr;
  uint32_t* d_c2src = nullptr;
  uint64_t* d_c2file = nullptr;
  uint64_t* d_c2place = nullptr;
  uint64_t* d_small = nullptr;  // m1_res, m2_res, l_res, w_res, x1_res, x2_res
  uint64_t* d_want = nullptr;
  constexpr size_t kSmall = 2 * files::kResFields + plan::kLinksResFields + plan::kWantResFields +
                            2 * extents::kResFields;
  if ((rc = stage.alloc(c)) || (in.deny && (rc = c.alloc(&d_deny, 8 * file_words))) ||
      (in.have && (rc = c.alloc(&d_have, 8 * nwords))) || (rc = c.alloc(&d_skip, 8 * file_words)) ||
      (rc = c.alloc(&d_mwork, dev::match_files_work_bytes(need_files, pool_files))) ||
      (rc = c.alloc(&d_c1src, 4 * need_files)) || (rc = c.alloc(&d_c1file, 8 * need_files)) ||
      (rc = c.alloc(&d_c2src, 4 * need_files)) || (rc = c.alloc(&d_c2file, 8 * need_files)) ||
      (rc = c.alloc(&d_c2place, 16 * need_files)) || (rc = c.alloc(&d_small, 8 * kSmall)) ||
      (rc = c.alloc(&d_want, 8 * nwords)))
    return rc;
  uint64_t* const d_m1res = d_small;
  uint64_t* const d_m2res = d_m1res + files::kResFields;
  uint64_t* const d_lres = d_m2res + files::kResFields;
  uint64_t* const d_wres = d_lres + plan::kLinksResFields;
  uint64_t* const d_x1res = d_wres + plan::kWantResFields;
  uint64_t* const d_x2res = d_x1res + extents::kResFields;
  if (trace && ((rc = ev.create()) || (rc = xev.create()))) return rc;
  // (both bitmaps go up in front of the stage's emit pass, as they always did;
  // since the stage, also in front of its src_first: DESIGN 4.5l)
  if (d_deny && file_words)
    CIR_HIP(hipMemcpyAsync(d_deny, in.deny, 8 * file_words, hipMemcpyHostToDevice, s));
  if (d_have) CIR_HIP(hipMemcpyAsync(d_have, in.have, 8 * nwords, hipMemcpyHostToDevice, s));
  if ((rc = stage.emit(c))) return rc;
  if (trace) CIR_HIP(hipStreamSynchronize(s));
  const auto t4 = Clock::now();
  // steps 1 to 3: the two file joins and the glue, back to back
  const dev::FilesSide need = stage.need(), pool = stage.pool();
  uint64_t* const d_first = stage.d_first;
  if (trace) CIR_HIP(hipEventRecord(ev.ev[0], s));
  CIR_HIP(dev::launch_match_files(need, pool, d_first, used, bs, nullptr, draw_seed(), d_mwork,
                                  d_c1src, d_c1file, d_m1res, s));
  if (trace) CIR_HIP(hipEventRecord(ev.ev[1], s));
  CIR_HIP(dev::launch_plan_links(d_deny, need_files, d_c1src, d_c1file, d_skip, d_lres, s));
  if (trace) CIR_HIP(hipEventRecord(ev.ev[2], s));
  CIR_HIP(dev::launch_match_copies(need, pool, d_first, used, bs, d_skip, nullptr, draw_seed(),
                                   d_mwork, d_c2src, d_c2file, d_c2place, d_m2res, s));
  if (trace) CIR_HIP(hipEventRecord(ev.ev[3], s));
  // (the need run table is where the emit pass left it: idxscan::Run is the
  // packed form but for its last word, which the kernel does not read)
  CIR_HIP(dev::launch_plan_want(ts.d_runs + plan::kRunWords * ts.item[0].runs_off, need_runs, n, bs,
                                need_files, d_c1src, d_c2src, d_have, d_want, d_wres, s));
  if (trace) CIR_HIP(hipEventRecord(ev.ev[4], s));
  c1src.resize(need_files);
  c2src.resize(need_files);
  c2file.resize(need_files);
  c2place.resize(copies::kPlaceWords * need_files);
  nrec.resize(need_files);
  if ((rc = stage.queue_verdicts(c))) return rc;
  CIR_HIP(hipMemcpyAsync(m1_res, d_m1res, sizeof m1_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(m2_res, d_m2res, sizeof m2_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(l_res, d_lres, sizeof l_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(w_res, d_wres, sizeof w_res, hipMemcpyDeviceToHost, s));
  if (need_files) {
    CIR_HIP(hipMemcpyAsync(c1src.data(), d_c1src, 4 * need_files, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipMemcpyAsync(c2src.data(), d_c2src, 4 * need_files, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipMemcpyAsync(c2file.data(), d_c2file, 8 * need_files, hipMemcpyDeviceToHost, s));
    CIR_HIP(hipMemcpyAsync(c2place.data(), d_c2place, 16 * need_files, hipMemcpyDeviceToHost, s));
    // (the need records: where each entry's own path stands, for the copies' stats[9])
    CIR_HIP(hipMemcpyAsync(nrec.data(), stage.d_nrec, 32 * need_files, hipMemcpyDeviceToHost, s));
  }
  // (with the run tables: the extent maps need them)
  if ((rc = stage.ts.finish(c, true))) return rc;
  const auto t5 = Clock::now();
  if ((rc = stage.verdicts_ok(m1_res[0] == files::kOk && m2_res[0] == files::kOk, why))) return rc;
  // steps 4 and 5.  The run tables: the need's twice (its first copy is the need
  // table of both maps, both copies the pool of the repeats), then the pool's.
  sources::BlockList nl, pl;
  for (size_t k = 0; k < nt; ++k) {
    sources::BlockList* list = k ? &pl : &nl;
    for (const idxscan::Run& run : ts.item[k].runs)
      list->runs.push_back(
          sources::FileRun{list->n + run.first, run.size, run.file, k ? tx[k].ordinal : 0});
    list->n += tx[k].nblk;
  }
  const size_t nr = nl.runs.size(), pr = pl.runs.size();
  tabs.resize(plan::kRunWords * (2 * nr + pr));
  sources::pack_runs(repeats::doubled(nl), tabs.data());
  sources::pack_runs(pl, tabs.data() + plan::kRunWords * 2 * nr);
  const uint64_t slots1 = dev::join_table_slots(pool_blocks), slots2 = dev::join_table_slots(n);
  uint64_t* d_tabs = nullptr;
  uint32_t* d_table = nullptr;  // (both joins initialise it, one after the other)
  uint32_t* d_match1 = nullptr;
  uint32_t* d_match2 = nullptr;
  uint64_t* d_xwork1 = nullptr;
  uint64_t* d_xwork2 = nullptr;
  uint64_t* d_fetch1 = nullptr;
  uint64_t* d_fetch2 = nullptr;
  uint64_t* d_present = nullptr;
  if ((rc = c.alloc(&d_tabs, 8 * tabs.size())) ||
      (rc = c.alloc(&d_table, sizeof(uint32_t) * (slots1 > slots2 ? slots1 : slots2))) ||
      (rc = c.alloc(&d_match1, (n + 4) * sizeof(uint32_t))) ||
      (rc = c.alloc(&d_match2, (n + 4) * sizeof(uint32_t))) ||
      (rc = c.alloc(&d_xwork1, dev::ext_work_bytes(n))) ||
      (rc = c.alloc(&d_xwork2, dev::ext_work_bytes(n))) || (rc = c.alloc(&d_fetch1, 8 * nwords)) ||
      (rc = c.alloc(&d_fetch2, 8 * nwords)) || (rc = c.alloc(&d_present, 8 * nwords)))
    return rc;
  CIR_HIP(hipMemcpyAsync(d_tabs, tabs.data(), 8 * tabs.size(), hipMemcpyHostToDevice, s));
  // `present` of step 5 is every block not in fetch1.  A block in fetch1 is
  // wanted there, and a bit set in both bitmaps means wanted
  // (repeats::key_of), so beside want = fetch1 an all-ones bitmap gives every
  // block the key its complement would: no kernel has to invert fetch1.
  CIR_HIP(hipMemsetAsync(d_present, 0xFF, 8 * nwords, s));
  const uint64_t* d_nruns = d_tabs;
  const uint64_t* d_pruns = d_tabs + plan::kRunWords * 2 * nr;
  const dev::ExtentArgs a1{d_match1, n, d_nruns, nr, d_pruns, pr, pool_blocks, bs, d_want};
  const dev::ExtentArgs a2{d_match2, n, d_nruns, nr, d_nruns, 2 * nr, 2 * n, bs, d_fetch1};
  if (trace) CIR_HIP(hipEventRecord(xev.ev[0], s));
  CIR_HIP(dev::launch_join(stage.d_ndig, n, stage.d_pdig, pool_blocks, d_table, slots1, draw_seed(),
                           d_match1, d_match1 + n, s));
  if (trace) CIR_HIP(hipEventRecord(xev.ev[1], s));
  // (no cap: the count decides the allocation, not the other way round)
  CIR_HIP(dev::launch_extent_map(a1, nullptr, nullptr, nullptr, d_fetch1, ~0ull, d_xwork1, d_x1res,
                                 s));
  if (trace) CIR_HIP(hipEventRecord(xev.ev[2], s));
  CIR_HIP(dev::launch_repeat_join(stage.d_ndig, n, d_fetch1, d_present, d_table, slots2,
                                  draw_seed(), d_match2, d_match2 + n, s));
  if (trace) CIR_HIP(hipEventRecord(xev.ev[3], s));
  CIR_HIP(dev::launch_extent_map(a2, nullptr, nullptr, nullptr, d_fetch2, ~0ull, d_xwork2, d_x2res,
                                 s));
  if (trace) CIR_HIP(hipEventRecord(xev.ev[4], s));
  CIR_HIP(hipMemcpyAsync(x1_res, d_x1res, sizeof x1_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipMemcpyAsync(x2_res, d_x2res, sizeof x2_res, hipMemcpyDeviceToHost, s));
  CIR_HIP(hipStreamSynchronize(s));
  const auto t6 = Clock::now();
  // the two extent tails; from here on *r owns what has come down
  auto drop = [&](int code) {
    r->drop();
    return code;
  };
  uint64_t* fetch1 = nullptr;
  auto t_emit = t6;
  if ((rc = device_extent_tail(c, a1, x1_res[5], d_xwork1, d_x1res, d_fetch1, false, &r->extents,
                               &fetch1, &t_emit)))
    return drop(rc);
  free(fetch1);  // (fetch2 is the plan's; fetch1 stays the device's business)
  r->nextents = x1_res[5];
  const auto t7 = Clock::now();
  if ((rc = device_extent_tail(c, a2, x2_res[5], d_xwork2, d_x2res, d_fetch2, false, &r->repeats,
                               &r->fetch, &t_emit)))
    return drop(rc);
  r->nrepeats = x2_res[5];
  r->nblk = n;
  const auto t8 = Clock::now();
  // compact the candidates, and decode each content candidate's path from the
  // source text held here
  std::vector<uint64_t> l1file;
  std::vector<uint32_t> l1src;
  uint64_t left_out = 0;  // (the skip bitmap is the device's: deny | candidate kept)
  for (uint64_t i = 0; i < need_files; ++i) {
    left_out += plan::skip_bit(in.deny, i, c1src[i]);
    if (c1src[i] == files::kNoSrc) continue;
    if (c1src[i] >= used) return drop(fail(CIR_EHIP, "candidate source out of range"));
    l1file.push_back(i);
    l1src.push_back(tx[1 + c1src[i]].ordinal);
  }
  copies::Found l2;
  switch (copies::compact(c2src.data(), c2file.data(), c2place.data(), nrec.data(), need_files,
                          stage.placed().data(), used, nullptr, &l2)) {
    case copies::kBadSource: return drop(fail(CIR_EHIP, "candidate source out of range"));
    case copies::kBadPlace: return drop(fail(CIR_EHIP, "candidate place out of range"));
    case copies::kCompacted: break;
  }
  const size_t n1 = l1file.size(), n2 = l2.file.size();
  if (n1 != l_res[0] || l_res[0] + l_res[1] != m1_res[1] || n2 != m2_res[1])
    return drop(fail(CIR_EHIP, "candidate count mismatch"));
  if (!dup(l1file.data(), n1, &r->link_file) || !dup(l1src.data(), n1, &r->link_src) ||
      !l2.give(&r->copy_file, &r->copy_src, &r->copy_src_file, &r->copy_path_off, &r->copy_paths))
    return drop(fail(CIR_ENOMEM, "malloc"));
  r->nlinks = n1;
  r->ncopies = n2;
  r->nskipped = in.nsrc - used;
  uint64_t* st = r->stats + plan::kStatSources;
  st[0] = need_files;
  st[1] = m1_res[1];
  st[2] = m1_res[2];
  st[3] = pool_files;
  st[4] = used;
  st[5] = dev::join_table_slots(pool_files);
  st[6] = 1;
  st = r->stats + plan::kStatCopies;
  st[0] = need_files;
  st[1] = n2;
  st[2] = m2_res[2];
  st[3] = pool_files;
  st[4] = used;
  st[5] = dev::join_table_slots(pool_files);
  st[6] = 1;
  st[8] = left_out;
  st[9] = l2.same;
  st = r->stats + plan::kStatExtents;
  st[0] = x1_res[1];
  st[1] = x1_res[2];
  st[2] = x1_res[3];
  st[3] = pool_blocks;
  st[4] = used;
  st[5] = x1_res[4];
  st[6] = slots1;
  st[7] = 1;
  st[8] = x1_res[5];
  st[9] = x1_res[1] - x1_res[2];
  st = r->stats + plan::kStatRepeats;
  st[0] = x2_res[1];
  st[1] = x2_res[2];
  st[2] = x2_res[3];
  st[3] = n;  // (with fetch1 and its complement every block takes part)
  st[4] = n - (x1_res[1] - x1_res[2]);
  st[5] = x2_res[4];
  st[6] = slots2;
  st[7] = 1;
  st[8] = x2_res[5];
  st[9] = x2_res[1] - x2_res[2];
  r->stats[plan::kStatWithdrawn] = l_res[1];
  r->stats[plan::kStatLinked] = n1 + n2;
  r->stats[plan::kStatLinkedBlocks] = w_res[1];
  r->stats[plan::kStatHave] = w_res[2];
  r->stats[plan::kStatDevice] = 1;
  uint64_t uploaded = 0;  // the texts' own bytes (the arena pads each to 16)
  for (const TextSet::Item& it : ts.item) uploaded += it.len;
  if (trace)
    fprintf(stderr,
            "cir fetch_plan: %llu files (%llu blocks) against %llu pool files (%llu blocks) of %zu "
            "source(s), device; frame and buffers %.2f ms, text upload %.2f ms (%llu bytes), count "
            "kernels %.2f ms, emit kernels %.2f ms, path join %.3f ms, links glue %.3f ms, content "
            "join %.3f ms, want glue %.3f ms, joins and download %.2f ms, block join %.3f ms, "
            "extent map %.3f ms, repeat join %.3f ms, repeat map %.3f ms, tables to counts %.2f "
            "ms, extent tail %.2f ms, repeat tail %.2f ms, compact and decode %.2f ms; %zu links, "
            "%zu copies, %llu extents, %llu repeats, %llu blocks to fetch\n",
            (unsigned long long)need_files, (unsigned long long)n, (unsigned long long)pool_files,
            (unsigned long long)pool_blocks, used, ms_between(t0, t1), ms_between(t1, t2),
            (unsigned long long)uploaded, ms_between(t2, t3), ms_between(t3, t4), ev.lap(0),
            ev.lap(1), ev.lap(2), ev.lap(3), ms_between(t4, t5), xev.lap(0), xev.lap(1),
            xev.lap(2), xev.lap(3), ms_between(t5, t6), ms_between(t6, t7), ms_between(t7, t8),
            ms_between(t8, Clock::now()), n1, n2, (unsigned long long)x1_res[5],
            (unsigned long long)x2_res[5], (unsigned long long)st[9]);
  return CIR_OK;
}

struct Outs {
  uint64_t** link_file_out;
  uint32_t** link_src_out;
  size_t* nlinks_out;
  uint64_t** copy_file_out;
  uint32_t** copy_src_out;
  uint64_t** copy_src_file_out;
  uint64_t** copy_path_off_out;
  uint8_t** copy_paths_out;
  size_t* ncopies_out;
  uint64_t** extents_out;
  size_t* nextents_out;
  uint64_t** repeat_extents_out;
  size_t* nrepeats_out;
  uint64_t** fetch_out;
  uint64_t* nblk_out;
  size_t* nskipped_out;
  uint64_t* stats;
  bool complete() const {
    return link_file_out && link_src_out && nlinks_out && copy_file_out && copy_src_out &&
           copy_src_file_out && copy_path_off_out && copy_paths_out && ncopies_out && extents_out &&
           nextents_out && repeat_extents_out && nrepeats_out && fetch_out && nblk_out && stats;
  }
  void give(const plan::Result& r) const {
    *link_file_out = r.link_file;
    *link_src_out = r.link_src;
    *nlinks_out = r.nlinks;
    *copy_file_out = r.copy_file;
    *copy_src_out = r.copy_src;
    *copy_src_file_out = r.copy_src_file;
    *copy_path_off_out = r.copy_path_off;
    *copy_paths_out = r.copy_paths;
    *ncopies_out = r.ncopies;
    *extents_out = r.extents;
    *nextents_out = r.nextents;
    *repeat_extents_out = r.repeats;
    *nrepeats_out = r.nrepeats;
    *fetch_out = r.fetch;
    *nblk_out = r.nblk;
    if (nskipped_out) *nskipped_out = r.nskipped;
    for (int i = 0; i < plan::kStatsFields; ++i) stats[i] = r.stats[i];
  }
};

int fetch_plan_impl(cir_ctx* ctx, const Inputs& in, const Outs& o) {
  if (!in.index || !o.complete() || (in.nsrc && (!in.src_index || !in.src_len)))
    return fail(CIR_EINVAL, "null pointer");
  plan::Result r;
  o.give(r);  // (every output null / 0 and the stats zero until the plan is whole)
  const bool trace = trace_enabled();
  uint64_t why = 0;
  if (ctx) {
    if (plan_on_host()) {
      why = CIR_FILE_WHY_ENV;
    } else {
      const int rc = fetch_plan_dev(ctx, in, &r, trace, &why);
      if (rc == CIR_OK) o.give(r);
      if (rc != kHostFlow) return rc;  // (nothing was reported yet)
      r.drop();
    }
  }
  const auto t0 = Clock::now();
  HostSiblings sib{in};
  const int rc = plan::plan_host(sib, in.deny, in.have, &r);
  if (rc) return rc;
  r.stats[plan::kStatWhy] = why;
  o.give(r);
  if (trace)
    fprintf(stderr,
            "cir fetch_plan: %llu files (%llu blocks) against %llu pool files of %llu source(s), "
            "host (why %llu); %.2f ms; %zu links, %zu copies, %zu extents, %zu repeats, %llu "
            "blocks to fetch\n",
            (unsigned long long)r.stats[0], (unsigned long long)r.nblk,
            (unsigned long long)r.stats[3], (unsigned long long)r.stats[4],
            (unsigned long long)why, ms_between(t0, Clock::now()), r.nlinks, r.ncopies, r.nextents,
            r.nrepeats, (unsigned long long)r.stats[plan::kStatRepeats + 9]);
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" int cir_plan_links_dev(cir_ctx* ctx, const uint64_t* d_deny, uint64_t n_files,
                                  uint32_t* d_cand_src, uint64_t* d_cand_file, uint64_t* d_skip,
                                  uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch, no side streams
  return cir::plan_links_dev_impl(d_deny, n_files, d_cand_src, d_cand_file, d_skip, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_plan_want_dev(cir_ctx* ctx, const uint64_t* d_need_runs, uint64_t n_need_runs,
                                 uint64_t n_blocks, uint64_t block_size, uint64_t n_files,
                                 const uint32_t* d_cand_a, const uint32_t* d_cand_b,
                                 const uint64_t* d_have, uint64_t* d_want, uint64_t* d_res,
                                 void* stream) try {
  (void)ctx;  // no scratch, no side streams
  return cir::plan_want_dev_impl(d_need_runs, n_need_runs, n_blocks, block_size, n_files, d_cand_a,
                                 d_cand_b, d_have, d_want, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_fetch_plan(cir_ctx* ctx, const uint8_t* index, size_t len,
                              const uint8_t* const* src_index, const size_t* src_len, size_t nsrc,
                              const uint64_t* deny, const uint64_t* have, uint64_t** link_file_out,
                              uint32_t** link_src_out, size_t* nlinks_out,
                              uint64_t** copy_file_out, uint32_t** copy_src_out,
                              uint64_t** copy_src_file_out, uint64_t** copy_path_off_out,
                              uint8_t** copy_paths_out, size_t* ncopies_out,
                              uint64_t** extents_out, size_t* nextents_out,
                              uint64_t** repeat_extents_out, size_t* nrepeats_out,
                              uint64_t** fetch_out, uint64_t* nblk_out, size_t* nskipped_out,
                              uint64_t stats[CIR_PLAN_STATS_FIELDS]) try {
  const cir::Inputs in{index, len, src_index, src_len, nsrc, deny, have};
  const cir::Outs o{link_file_out,     link_src_out,   nlinks_out,         copy_file_out,
                    copy_src_out,      copy_src_file_out, copy_path_off_out, copy_paths_out,
                    ncopies_out,       extents_out,    nextents_out,       repeat_extents_out,
                    nrepeats_out,      fetch_out,      nblk_out,           nskipped_out,
                    stats};
  return cir::fetch_plan_impl(ctx, in, o);
} CIR_CATCH_BOUNDARY
