// Seeded fuzz of the download plan's rule (ciruela_amd/csrc/plan.hpp: bit,
// withdrawn, skip_bit, blocks_of, run_at, class_of, links_host, want_host,
// present_host -- the text the kernels k_plan_links and k_plan_want of plan.hip
// compile -- and plan_host, the composition) against a double loop that goes
// one block and one file at a time.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/plan_fuzz.cpp -o build/plan_fuzz
// and run it; tests/test_fetch_plan_cpu.py does.  Every case holds the run
// table, the candidate arrays and the bitmaps in heap buffers of exactly their
// size, so a read or a write one element outside is an AddressSanitizer
// report.
//
// Per case: a layout of 0-40 files of 0-70 blocks (empty files take an ordinal
// and no run; short last blocks), random candidates, deny and have bitmaps.
//   1. links_host equals the loop over files: what is withdrawn, the skip
//      bits, every word written, bits at and past n_files 0, the counts;
//   2. want_host equals the loop over files and their blocks, through either
//      candidate array and through both;
//   3. a lying but sorted table (ordinals >= n_files, `first` >= n_blocks,
//      sizes of 2^64 - 1, bs = 1) equals a loop that goes block by block over
//      the table with 128-bit arithmetic; nothing outside the arrays is read;
//   4. plan_host over four stand-in calls, which answer by the siblings'
//      contracts from small tables and record what they were given, hands each
//      the bitmap the composition names -- skip = deny | L1, want = want1,
//      want = fetch1 with present = its complement below n -- withdraws what
//      deny forbids, fills the plan's own stats, and on a failure of any of the
//      four leaves every output null and the stats zero.
//
// usage: plan_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "plan.hpp"

using namespace cir;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

static uint64_t g_case, g_files, g_blocks, g_wanted, g_linked, g_held, g_lies, g_plans, g_failed;
#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "plan_fuzz: %s:%d: %s (case %llu)\n", __FILE__, __LINE__, #c, \
              (unsigned long long)g_case);                                     \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

// A heap array of exactly n elements (none at all for n == 0).
template <typename T>
struct Exact {
  T* p;
  uint64_t n;
  explicit Exact(uint64_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

static bool get(const uint64_t* m, uint64_t i) { return (m[i >> 6] >> (i & 63)) & 1; }

struct Shape {
  std::vector<uint64_t> nblk;  // blocks per file, in file order
  std::vector<uint64_t> size;
  uint64_t bs = 1, n_blocks = 0;
  std::vector<uint64_t> runs;  // packed
};

static Shape make_shape() {
  Shape s;
  s.bs = 1 + rnd() % 64;
  const uint64_t nf = rnd() % 41;
  for (uint64_t f = 0; f < nf; ++f) {
    const uint64_t k = rnd() % 4 == 0 ? 0 : rnd() % 3 == 0 ? 1 + rnd() % 70 : 1 + rnd() % 3;
    const uint64_t size = k == 0 ? 0 : (k - 1) * s.bs + (rnd() % 2 ? s.bs : 1 + rnd() % s.bs);
    s.nblk.push_back(k);
    s.size.push_back(size);
    if (k) {
      s.runs.insert(s.runs.end(), {s.n_blocks, size, f, rnd()});
      s.n_blocks += k;
    }
  }
  return s;
}

static void fill_bits(Exact<uint64_t>& m, uint64_t n, unsigned one_in) {
  for (uint64_t w = 0; w < m.n; ++w) m.p[w] = 0;
  for (uint64_t i = 0; i < 64 * m.n; ++i)  // (bits at and past n too: they are ignored)
    if (rnd() % one_in == 0 && (i < n || rnd() % 2)) m.p[i >> 6] |= 1ull << (i & 63);
}

static void one_case() {
  const Shape s = make_shape();
  const uint64_t nf = s.nblk.size(), nb = s.n_blocks, fw = (nf + 63) / 64, bw = (nb + 63) / 64;
  g_files += nf;
  g_blocks += nb;
  // 1. the links glue
  const bool with_deny = rnd() % 3 != 0, with_have = rnd() % 3 != 0;
  Exact<uint64_t> deny(with_deny ? fw : 0), have(with_have ? bw : 0), skip(fw);
  fill_bits(deny, nf, 3);
  fill_bits(have, nb, 3);
  Exact<uint32_t> ca(nf), cb(nf), ca0(nf);
  Exact<uint64_t> cf(nf);
  for (uint64_t f = 0; f < nf; ++f) {
    ca0.p[f] = ca.p[f] = rnd() % 2 ? (uint32_t)(rnd() % 5) : plan::kNoSrc;
    cf.p[f] = ca.p[f] == plan::kNoSrc ? plan::kNoFile : rnd() % 1000;
  }
  for (uint64_t w = 0; w < fw; ++w) skip.p[w] = rnd();  // (every word must be written)
  uint64_t lres[plan::kLinksResFields];
  plan::links_host(with_deny ? deny.p : nullptr, nf, ca.p, cf.p, skip.p, lres);
  uint64_t kept = 0, gone = 0;
  for (uint64_t f = 0; f < nf; ++f) {
    const bool d = with_deny && get(deny.p, f), had = ca0.p[f] != plan::kNoSrc;
    CHECK(ca.p[f] == (d ? plan::kNoSrc : ca0.p[f]));
    CHECK((ca.p[f] == plan::kNoSrc) == (cf.p[f] == plan::kNoFile));
    CHECK(get(skip.p, f) == (d || had));
    kept += had && !d;
    gone += had && d;
  }
  for (uint64_t i = nf; i < 64 * fw; ++i) CHECK(!get(skip.p, i));
  CHECK(lres[0] == kept && lres[1] == gone);
  // 2. the want glue, file by file and block by block
  for (uint64_t f = 0; f < nf; ++f) cb.p[f] = get(skip.p, f) || rnd() % 3 ? plan::kNoSrc : 1;
  for (int arrays = 0; arrays < 3; ++arrays) {
    const uint32_t* a = arrays == 1 ? nullptr : ca.p;
    const uint32_t* b = arrays == 0 ? nullptr : cb.p;
    Exact<uint64_t> want(bw);
    for (uint64_t w = 0; w < bw; ++w) want.p[w] = rnd();
    uint64_t wres[plan::kWantResFields];
    plan::want_host(s.runs.data(), s.runs.size() / 4, nb, s.bs, nf, nf ? a : nullptr,
                    nf ? b : nullptr, with_have ? have.p : nullptr, want.p, wres);
    uint64_t g = 0, wanted = 0, linked = 0, held = 0;
    for (uint64_t f = 0; f < nf; ++f)
      for (uint64_t k = 0; k < s.nblk[f]; ++k, ++g) {
        const bool l = (a && a[f] != plan::kNoSrc) || (b && b[f] != plan::kNoSrc);
        const bool h = !l && with_have && get(have.p, g);
        CHECK(get(want.p, g) == (!l && !h));
        wanted += !l && !h;
        linked += l;
        held += h;
      }
    CHECK(g == nb);
    for (uint64_t i = nb; i < 64 * bw; ++i) CHECK(!get(want.p, i));
    CHECK(wres[0] == wanted && wres[1] == linked && wres[2] == held);
    g_wanted += wanted;
    g_linked += linked;
    g_held += held;
  }
  // 3. a sorted table that lies
  {
    const uint64_t n = 1 + rnd() % 300, nruns = rnd() % 9, n_files = rnd() % 6;
    const uint64_t bs = rnd() % 3 == 0 ? 1 : 1 + rnd() % 64;
    Exact<uint64_t> runs(4 * nruns), want((n + 63) / 64), hv((n + 63) / 64);
    Exact<uint32_t> cand(n_files);
    for (uint64_t f = 0; f < n_files; ++f) cand.p[f] = rnd() % 2 ? 3 : plan::kNoSrc;
    fill_bits(hv, n, 4);
    uint64_t first = rnd() % 8;
    for (uint64_t r = 0; r < nruns; ++r) {
      runs.p[4 * r] = first;
      const unsigned kind = rnd() % 4;
      runs.p[4 * r + 1] = kind == 0 ? ~0ull : kind == 1 ? ~0ull - rnd() % 3 : rnd() % (70 * bs);
      runs.p[4 * r + 2] = rnd() % 3 == 0 ? ~0ull - rnd() % 2 : rnd() % (n_files + 2);
      runs.p[4 * r + 3] = rnd();
      first += 1 + (rnd() % 4 == 0 ? rnd() % 400 : rnd() % 40);  // (some at and past n)
      if (rnd() % 16 == 0) first = (1ull << 33) + first;
    }
    uint64_t wres[plan::kWantResFields];
    plan::want_host(runs.p, nruns, n, bs, n_files, cand.p, nullptr, hv.p, want.p, wres);
    uint64_t cnt[3] = {0, 0, 0};
    for (uint64_t g = 0; g < n; ++g) {
      int cls = -1;  // the last run with first <= g, found by walking the table
      for (uint64_t r = nruns; r-- > 0;) {
        if (runs.p[4 * r] > g) continue;
        const unsigned __int128 size = runs.p[4 * r + 1];
        const unsigned __int128 blocks = (size + bs - 1) / bs;  // (no wrap in 128 bits)
        if ((unsigned __int128)(g - runs.p[4 * r]) < blocks) {
          const uint64_t f = runs.p[4 * r + 2];
          cls = f < n_files && cand.p[f] != plan::kNoSrc ? 1 : get(hv.p, g) ? 2 : 0;
        }
        break;
      }
      CHECK(get(want.p, g) == (cls == 0));
      if (cls >= 0) ++cnt[cls];
    }
    CHECK(wres[0] == cnt[0] && wres[1] == cnt[1] && wres[2] == cnt[2]);
    ++g_lies;
  }
}

// ---- 4. the composition over stand-in calls ----------------------------------------

template <class T>
static T* give(const std::vector<T>& v) {
  if (v.empty()) return nullptr;
  T* p = (T*)malloc(v.size() * sizeof(T));
  memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

struct StandIns {
  Shape s;
  std::vector<uint32_t> same_path, by_content;  // per file: a source, or kNoSrc
  std::vector<uint8_t> local;                   // per block: an older image holds it
  std::vector<uint8_t> twin;                    // per block: an earlier block equals it
  int fail_at = 0;                              // 1..5: that call fails
  // what the calls were given
  std::vector<uint64_t> skip_seen, want_seen, want2_seen, present_seen;
  uint64_t nf() const { return s.nblk.size(); }

  int layout(plan::Layout* lay) const {
    if (fail_at == 1) return -3;
    lay->runs = s.runs;
    lay->n_files = nf();
    lay->n_blocks = s.n_blocks;
    lay->bs = s.bs;
    return 0;
  }
  int file_sources(uint64_t** file, uint32_t** src, size_t* n, size_t* nskipped, uint64_t* st) {
    if (fail_at == 2) return -4;
    std::vector<uint64_t> f;
    std::vector<uint32_t> sv;
    for (uint64_t i = 0; i < nf(); ++i)
      if (same_path[i] != plan::kNoSrc) {
        f.push_back(i);
        sv.push_back(same_path[i]);
      }
    *file = give(f);
    *src = give(sv);
    *n = f.size();
    *nskipped = 2;
    st[0] = nf();
    st[1] = f.size();
    return 0;
  }
  int file_copies(const uint64_t* skip, uint64_t** file, uint32_t** src, uint64_t** src_file,
                  uint64_t** path_off, uint8_t** paths, size_t* n, size_t* nskipped, uint64_t* st) {
    skip_seen.assign(skip, skip + (nf() + 63) / 64);
    if (fail_at == 3) return -5;
    std::vector<uint64_t> f, sf, off{0};
    std::vector<uint32_t> sv;
    std::vector<uint8_t> p;
    for (uint64_t i = 0; i < nf(); ++i)
      if (by_content[i] != plan::kNoSrc && !get(skip, i) && s.nblk[i]) {
        f.push_back(i);
        sv.push_back(by_content[i]);
        sf.push_back(i + 1);
        p.push_back('/');
        p.push_back((uint8_t)('a' + i % 26));
        off.push_back(p.size());
      }
    *file = give(f);
    *src = give(sv);
    *src_file = give(sf);
    *path_off = f.empty() ? nullptr : give(off);
    *paths = give(p);
    *n = f.size();
    *nskipped = 2;
    st[1] = f.size();
    return 0;
  }
  int block_extents(const uint64_t* want, uint64_t** ext, size_t* next, uint64_t** fetch,
                    uint64_t* nblk, size_t* nskipped, uint64_t* st) {
    const uint64_t n = s.n_blocks, nw = (n + 63) / 64;
    want_seen.assign(want, want + nw);
    if (fail_at == 4) return -6;
    *ext = nullptr;
    *next = 0;
    *fetch = nullptr;
    *nblk = n;
    *nskipped = 2;
    if (n == 0) return 0;
    std::vector<uint64_t> rec, fw(nw, 0);
    for (uint64_t g = 0; g < n; ++g) {
      if (!get(want, g)) continue;
      if (local[g])
        rec.insert(rec.end(), {g, 1, 0, 0, 0, 0, 0, 1});  // (one record per block: a stand-in)
      else
        fw[g >> 6] |= 1ull << (g & 63);
    }
    *ext = give(rec);
    *next = rec.size() / 8;
    *fetch = give(fw);
    st[1] = *next;
    return 0;
  }
  int block_repeats(const uint64_t* want, const uint64_t* present, uint64_t** ext, size_t* next,
                    uint64_t** fetch, uint64_t* nblk, uint64_t* st) {
    const uint64_t n = s.n_blocks, nw = (n + 63) / 64;
    want2_seen.assign(want, want + nw);
    present_seen.assign(present, present + nw);
    if (fail_at == 5) return -7;
    *ext = nullptr;
    *next = 0;
    *fetch = nullptr;
    *nblk = n;
    if (n == 0) return 0;
    std::vector<uint64_t> rec, fw(nw, 0);
    for (uint64_t g = 0; g < n; ++g) {
      if (!get(want, g)) continue;
      if (twin[g])
        rec.insert(rec.end(), {g, 1, 0, 0, 1, 0, 0, 1});
      else
        fw[g >> 6] |= 1ull << (g & 63);
    }
    *ext = give(rec);
    *next = rec.size() / 8;
    *fetch = give(fw);
    st[1] = *next;
    return 0;
  }
};

static void one_plan() {
  StandIns sib;
  sib.s = make_shape();
  const uint64_t nf = sib.nf(), nb = sib.s.n_blocks, fw = (nf + 63) / 64, bw = (nb + 63) / 64;
  for (uint64_t f = 0; f < nf; ++f) {
    sib.same_path.push_back(rnd() % 3 == 0 ? (uint32_t)(rnd() % 4) : plan::kNoSrc);
    sib.by_content.push_back(rnd() % 2 == 0 ? (uint32_t)(rnd() % 4) : plan::kNoSrc);
  }
  for (uint64_t g = 0; g < nb; ++g) {
    sib.local.push_back(rnd() % 2);
    sib.twin.push_back(rnd() % 4 == 0);
  }
  sib.fail_at = rnd() % 4 == 0 ? 1 + (int)(rnd() % 5) : 0;
  const bool with_deny = rnd() % 2, with_have = rnd() % 2;
  Exact<uint64_t> deny(with_deny ? fw : 0), have(with_have ? bw : 0);
  fill_bits(deny, nf, 3);
  fill_bits(have, nb, 3);
  const uint64_t* dn = with_deny ? deny.p : nullptr;
  const uint64_t* hv = with_have ? have.p : nullptr;
  plan::Result r;
  r.nlinks = 77;  // (whatever was there before is overwritten)
  const int rc = plan::plan_host(sib, dn, hv, &r);
  ++g_plans;
  if (sib.fail_at) {
    CHECK(rc == -2 - sib.fail_at);
    CHECK(!r.link_file && !r.link_src && !r.copy_file && !r.copy_src && !r.copy_src_file &&
          !r.copy_path_off && !r.copy_paths && !r.extents && !r.repeats && !r.fetch);
    CHECK(r.nlinks == 0 && r.ncopies == 0 && r.nextents == 0 && r.nrepeats == 0 && r.nblk == 0 &&
          r.nskipped == 0);
    for (int i = 0; i < plan::kStatsFields; ++i) CHECK(r.stats[i] == 0);
    ++g_failed;
    return;
  }
  CHECK(rc == 0);
  // file by file: the links, and what each later call must have been given
  std::vector<uint8_t> linked(nf, 0);
  uint64_t k1 = 0, k2 = 0, gone = 0;
  for (uint64_t f = 0; f < nf; ++f) {
    const bool d = dn && get(dn, f), l1 = sib.same_path[f] != plan::kNoSrc && !d;
    gone += sib.same_path[f] != plan::kNoSrc && d;
    CHECK(get(sib.skip_seen.data(), f) == (d || l1));
    if (l1) {
      CHECK(k1 < r.nlinks && r.link_file[k1] == f && r.link_src[k1] == sib.same_path[f]);
      ++k1;
    }
    const bool l2 = !d && !l1 && sib.by_content[f] != plan::kNoSrc && sib.s.nblk[f];
    if (l2) {
      CHECK(k2 < r.ncopies && r.copy_file[k2] == f && r.copy_src[k2] == sib.by_content[f] &&
            r.copy_src_file[k2] == f + 1 && r.copy_path_off[k2 + 1] - r.copy_path_off[k2] == 2);
      ++k2;
    }
    linked[f] = l1 || l2;
  }
  CHECK(k1 == r.nlinks && k2 == r.ncopies);
  CHECK((r.nlinks == 0) == (r.link_file == nullptr) && (r.ncopies == 0) == (r.copy_file == nullptr));
  // block by block
  uint64_t g = 0, e1 = 0, e2 = 0, lb = 0, hb = 0;
  for (uint64_t f = 0; f < nf; ++f)
    for (uint64_t k = 0; k < sib.s.nblk[f]; ++k, ++g) {
      const bool h = !linked[f] && hv && get(hv, g), w1 = !linked[f] && !h;
      lb += linked[f];
      hb += h;
      CHECK(get(sib.want_seen.data(), g) == w1);
      const bool f1 = w1 && !sib.local[g];
      CHECK(get(sib.want2_seen.data(), g) == f1 && get(sib.present_seen.data(), g) == !f1);
      if (w1 && sib.local[g]) {
        CHECK(e1 < r.nextents && r.extents[8 * e1] == g);
        ++e1;
      }
      if (f1 && sib.twin[g]) {
        CHECK(e2 < r.nrepeats && r.repeats[8 * e2] == g);
        ++e2;
      }
      CHECK(get(r.fetch, g) == (f1 && !sib.twin[g]));
    }
  CHECK(g == nb && e1 == r.nextents && e2 == r.nrepeats && r.nblk == nb);
  for (uint64_t i = nb; i < 64 * bw; ++i) CHECK(!get(sib.present_seen.data(), i));
  CHECK(r.nskipped == 2);
  CHECK(r.stats[plan::kStatWithdrawn] == gone && r.stats[plan::kStatLinked] == k1 + k2 &&
        r.stats[plan::kStatLinkedBlocks] == lb && r.stats[plan::kStatHave] == hb);
  CHECK(r.stats[plan::kStatSources] == nf && r.stats[plan::kStatCopies + 1] == k2 &&
        r.stats[plan::kStatExtents + 1] == e1 && r.stats[plan::kStatRepeats + 1] == e2);
  r.drop();
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (g_case = 0; g_case < cases; ++g_case) {
    one_case();
    one_plan();
  }
  fprintf(stderr,
          "plan_fuzz: %llu files, %llu blocks; %llu wanted, %llu linked, %llu held; %llu lying "
          "tables; %llu plans, %llu failed\n",
          (unsigned long long)g_files, (unsigned long long)g_blocks, (unsigned long long)g_wanted,
          (unsigned long long)g_linked, (unsigned long long)g_held, (unsigned long long)g_lies,
          (unsigned long long)g_plans, (unsigned long long)g_failed);
  printf("plan_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
