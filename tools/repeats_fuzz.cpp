// Seeded fuzz of the repeat rule (ciruela_amd/csrc/repeats.hpp: key_of,
// match_of -- the text the kernels of repeats.hip compile -- and host_match,
// doubled) and of the host path over it (sources::map_matches +
// sources::extents_of over the doubled run table, what cir_block_repeats runs
// with ctx = NULL) against a double loop that hashes nothing and bisects
// nothing.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/repeats_fuzz.cpp ciruela_amd/csrc/dirsig.cpp -o build/repeats_fuzz
// and run it; tests/test_block_repeats_cpu.py does.  Every case holds the
// digests, the bitmaps, the match array and the results in heap buffers of
// exactly their size, so a read or a write one element outside is an
// AddressSanitizer report.
//
// usage: repeats_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "repeats.hpp"
#include "sources.hpp"

using namespace cir;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

static uint64_t g_case;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      fprintf(stderr, "repeats_fuzz: %s:%d: %s (case %llu)\n", __FILE__, __LINE__, #c, \
              (unsigned long long)g_case);                                        \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)

// A heap array of exactly n elements (none at all for n == 0).
template <typename T>
struct Exact {
  T* p;
  explicit Exact(uint64_t n) : p(n ? new T[n]() : nullptr) {}
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

struct Plain {  // the double loop's answer for one block
  bool wanted = false, part = false, repeat = false, found = false, dropped = false;
  uint64_t leader = 0, run = 0, block = 0, len = 0;
  uint32_t cls = 0;  // of the leader: 0 present, 1 wanted
};

static bool bit_of(const uint64_t* map, uint64_t g) { return map[g / 64] >> (g % 64) & 1; }

static void one_case() {
  const uint64_t bs = 1 + rnd() % 9;
  // files of 1..7 blocks, some with a short tail; empty files in between
  sources::BlockList need;
  const int nfiles = (int)(rnd() % 9);
  uint64_t file = 0;
  for (int f = 0; f < nfiles; ++f) {
    file += rnd() % 3;
    uint64_t nfull = rnd() % 7;
    const uint64_t tail = (bs > 1 && rnd() % 3 == 0) ? 1 + rnd() % (bs - 1) : 0;
    if (nfull == 0 && tail == 0) nfull = 1;
    const uint64_t size = nfull * bs + tail;
    need.runs.push_back(sources::FileRun{need.n, size, file, 0});
    need.n += (size + bs - 1) / bs;
    ++file;
  }
  const uint64_t n = need.n, nwords = (n + 63) / 64;
  // digests from a small universe, so that repeats abound; stretches copied
  // from earlier blocks, so that extents longer than one block occur
  const uint64_t universe = 1 + rnd() % 12;
  Exact<uint8_t> digests(32 * n);
  for (uint64_t g = 0; g < n; ++g) {
    if (g > 0 && rnd() % 3 == 0) {
      const uint64_t from = rnd() % g, len = 1 + rnd() % 5;
      for (uint64_t k = 0; k < len && g + k < n && from + k < g; ++k)
        memcpy(digests.p + 32 * (g + k), digests.p + 32 * (from + k), 32);
      continue;
    }
    memset(digests.p + 32 * g, (int)(rnd() % universe), 32);
    digests.p[32 * g + 31] = (uint8_t)(rnd() % 2);  // (they differ in the last byte too)
  }
  const int mode = (int)(rnd() % 4);  // 0: no bitmaps, 1: want, 2: both, 3: present alone
  Exact<uint64_t> want_b(nwords), present_b(nwords);
  for (uint64_t w = 0; w < nwords; ++w) {
    want_b.p[w] = rnd() | rnd();
    present_b.p[w] = rnd();
  }
  const uint64_t* want = (mode == 1 || mode == 2) ? want_b.p : nullptr;
  const uint64_t* present = (mode == 2 || mode == 3) ? present_b.p : nullptr;
  if (nwords == 0) want = present = nullptr;

  // the rule, through the header
  Exact<uint32_t> match(n), src(n);
  Exact<uint64_t> sfile(n), sblock(n), fetch(nwords);
  const repeats::Counts c = repeats::host_match(digests.p, n, want, present, match.p, rnd());
  const sources::BlockList pool = repeats::doubled(need);
  const sources::MapStats ms =
      sources::map_matches(need, pool, bs, want, match.p, src.p, sfile.p, sblock.p);
  std::vector<sources::Extent> ex;
  const uint64_t left = sources::extents_of(need, bs, want, src.p, sfile.p, sblock.p, &ex, fetch.p);

  // the double loop
  std::vector<Plain> pl(n);
  std::vector<uint64_t> run_of(n), blk_of(n), len_of(n);
  for (size_t r = 0; r < need.runs.size(); ++r) {
    const sources::FileRun& run = need.runs[r];
    const uint64_t nb = (run.size + bs - 1) / bs;
    for (uint64_t b = 0; b < nb; ++b) {
      run_of[run.first + b] = r;
      blk_of[run.first + b] = b;
      len_of[run.first + b] = run.size - b * bs < bs ? run.size - b * bs : bs;
    }
  }
  uint64_t wanted = 0, npresent = 0, nrepeat = 0, found = 0, bytes = 0, dropped = 0;
  for (uint64_t g = 0; g < n; ++g) {
    Plain& p = pl[g];
    p.wanted = !want || bit_of(want, g);
    const bool pres = !p.wanted && present && bit_of(present, g);
    p.part = p.wanted || pres;
    wanted += p.wanted;
    npresent += pres;
  }
  for (uint64_t g = 0; g < n; ++g) {
    Plain& p = pl[g];
    if (!p.wanted) {
      CHECK(match.p[g] == repeats::kNone);
      continue;
    }
    // the leader: a present holder, the first; else the first wanted holder
    bool have = false;
    for (int cls = 0; cls < 2 && !have; ++cls)
      for (uint64_t j = 0; j < n && !have; ++j) {
        if (!pl[j].part || pl[j].wanted != (cls == 1)) continue;
        if (memcmp(digests.p + 32 * j, digests.p + 32 * g, 32) != 0) continue;
        have = true;
        p.leader = j;
        p.cls = (uint32_t)cls;
      }
    CHECK(have);
    p.repeat = p.leader != g;
    if (!p.repeat) {
      CHECK(match.p[g] == repeats::kNone);
      continue;
    }
    ++nrepeat;
    CHECK(match.p[g] == (p.cls ? n + p.leader : p.leader));
    if (len_of[p.leader] != len_of[g]) {
      p.dropped = true;
      ++dropped;
    } else {
      p.found = true;
      ++found;
      bytes += len_of[g];
    }
  }
  CHECK(c.wanted == wanted && c.present == npresent && c.repeats == nrepeat);
  const repeats::Counts cc = repeats::count_classes(want, present, n);
  CHECK(cc.wanted == wanted && cc.present == npresent);
  CHECK(ms.wanted == wanted && ms.found == found && ms.bytes == bytes && ms.dropped == dropped);
  CHECK(left == wanted - found);
  // the extents, block by block
  size_t at = 0;
  for (uint64_t g = 0; g < n; ++g) {
    const Plain& p = pl[g];
    CHECK(bit_of(fetch.p, g) == (p.wanted && !p.found));
    if (!p.found) {
      CHECK(src.p[g] == sources::kNone);
      continue;
    }
    CHECK(src.p[g] == p.cls && sfile.p[g] == need.runs[run_of[p.leader]].file &&
          sblock.p[g] == blk_of[p.leader]);
    const Plain* q = g ? &pl[g - 1] : nullptr;
    const bool joins = q && q->found && run_of[g - 1] == run_of[g] && q->cls == p.cls &&
                       run_of[q->leader] == run_of[p.leader] && p.leader == q->leader + 1;
    if (joins) continue;
    uint64_t h = g;  // the stretch's last block
    while (h + 1 < n && pl[h + 1].found && run_of[h + 1] == run_of[g] &&
           pl[h + 1].cls == p.cls && run_of[pl[h + 1].leader] == run_of[p.leader] &&
           pl[h + 1].leader == pl[h].leader + 1)
      ++h;
    CHECK(at < ex.size());
    const sources::Extent& e = ex[at++];
    uint64_t nbytes = 0;
    for (uint64_t k = g; k <= h; ++k) nbytes += len_of[k];
    CHECK(e.first == g && e.count == h - g + 1 && e.need_file == need.runs[run_of[g]].file &&
          e.need_block == blk_of[g] && e.src == p.cls &&
          e.src_file == need.runs[run_of[p.leader]].file && e.src_block == blk_of[p.leader] &&
          e.bytes == nbytes);
  }
  CHECK(at == ex.size());
  for (uint64_t g = n; g < 64 * nwords; ++g) CHECK(!bit_of(fetch.p, g));  // no bit at or past n
  // the tail cir_block_repeats runs with ctx = NULL hands the same over, malloc'd
  uint64_t* o_rec = nullptr;
  uint64_t* o_fetch = nullptr;
  size_t o_count = 0;
  uint64_t o_left = 0;
  CHECK(sources::extents_owned(need, bs, want, src.p, sfile.p, sblock.p, &o_rec, &o_count, &o_fetch,
                               &o_left));
  CHECK(o_count == ex.size() && o_left == left && (o_rec == nullptr) == ex.empty());
  CHECK(ex.empty() || memcmp(o_rec, ex.data(), ex.size() * sizeof(sources::Extent)) == 0);
  CHECK(nwords == 0 || memcmp(o_fetch, fetch.p, 8 * nwords) == 0);
  free(o_rec);
  free(o_fetch);
  // no block is both a source and a destination
  for (uint64_t g = 0; g < n; ++g)
    if (pl[g].repeat) CHECK(!pl[pl[g].leader].repeat && pl[pl[g].leader].part);
  // with nothing dropped, the blocks left to fetch have pairwise distinct
  // digests, none of them a present block's
  if (dropped == 0)
    for (uint64_t g = 0; g < n; ++g) {
      if (!bit_of(fetch.p, g)) continue;
      for (uint64_t j = 0; j < n; ++j) {
        if (j == g || memcmp(digests.p + 32 * j, digests.p + 32 * g, 32) != 0) continue;
        CHECK(!bit_of(fetch.p, j));
        CHECK(!(pl[j].part && !pl[j].wanted));
      }
    }
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (g_case = 0; g_case < cases; ++g_case) one_case();
  printf("repeats_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
