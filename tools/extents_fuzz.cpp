// Seeded fuzz of the extent rule (ciruela_amd/csrc/extents.hpp: map_block,
// cont, extent_bytes -- the text the kernels of extents.hip compile) and of the
// host path over it (sources::map_matches + sources::extents_of in
// ciruela_amd/csrc/sources.hpp) against a block-by-block double loop that
// bisects nothing.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/extents_fuzz.cpp ciruela_amd/csrc/dirsig.cpp -o build/extents_fuzz
// and run it; tests/test_block_extents_cpu.py does.  Every case holds the run
// tables, the match array, the want bitmap and the results in heap buffers of
// exactly their size, so a read or a write one element outside is an
// AddressSanitizer report.  Every eighth case scrambles the tables (unsorted
// runs, `first` past n_need, sizes of 2^64 - 1, ordinals >= n_pool): the rule
// promises no answer there, only that nothing outside the buffers is touched.
//
// usage: extents_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "extents.hpp"
#include "sources.hpp"

using namespace cir;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      fprintf(stderr, "extents_fuzz: %s:%d: %s (case %llu)\n", __FILE__, __LINE__, #c, \
              (unsigned long long)g_case);                                        \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)
static uint64_t g_case;

// A random block list: files of 1..9 blocks, some with a short tail.
static sources::BlockList random_list(uint64_t bs, int max_files, uint32_t nsrc) {
  sources::BlockList l;
  const int nfiles = (int)(rnd() % (max_files + 1));
  uint64_t file = 0;
  uint32_t src = 0;
  for (int f = 0; f < nfiles; ++f) {
    file += rnd() % 3;  // (empty files in between take an ordinal and no run)
    if (nsrc > 1 && rnd() % 4 == 0 && src + 1 < nsrc) {
      ++src;
      file = 0;
    }
    const uint64_t nfull = rnd() % 9;
    const uint64_t tail = (nfull == 0 || rnd() % 3 == 0) ? 1 + rnd() % (bs - 1) : 0;
    l.runs.push_back(sources::FileRun{l.n, nfull * bs + tail, file, src});
    l.n += nfull + (tail != 0);
    ++file;
  }
  return l;
}

struct Plain {  // the double loop's answer for one block
  bool in_file = false, wanted = false, found = false, dropped = false;
  size_t run = 0;
  uint64_t need_file = 0, need_block = 0, size = 0, len = 0, file = 0, block = 0;
  uint32_t src = 0;
};

static Plain plain_block(const sources::BlockList& need, const sources::BlockList& pool,
                         uint64_t bs, const uint64_t* want, const uint32_t* match, uint64_t g) {
  Plain p;
  for (size_t r = 0; r < need.runs.size(); ++r) {
    const sources::FileRun& run = need.runs[r];
    const uint64_t nb = (run.size + bs - 1) / bs;
    if (g < run.first || g >= run.first + nb) continue;
    p.in_file = true;
    p.run = r;
    p.need_file = run.file;
    p.need_block = g - run.first;
    p.size = run.size;
    p.len = run.size - p.need_block * bs < bs ? run.size - p.need_block * bs : bs;
  }
  if (!p.in_file) return p;
  p.wanted = !want || (want[g / 64] >> (g % 64) & 1);
  if (!p.wanted || match[g] >= pool.n) return p;
  for (const sources::FileRun& run : pool.runs) {
    const uint64_t nb = (run.size + bs - 1) / bs;
    const uint64_t j = match[g];
    if (j < run.first || j >= run.first + nb) continue;
    const uint64_t pb = j - run.first;
    const uint64_t plen = run.size - pb * bs < bs ? run.size - pb * bs : bs;
    if (plen != p.len) {
      p.dropped = true;
    } else {
      p.found = true;
      p.src = run.src;
      p.file = run.file;
      p.block = pb;
    }
  }
  return p;
}

static void tables_of(const sources::BlockList& l, std::vector<uint64_t>* t) {
  t->clear();
  for (const sources::FileRun& r : l.runs) {
    t->push_back(r.first);
    t->push_back(r.size);
    t->push_back(r.file);
    t->push_back(r.src | (rnd() << 32));  // (only the low half is the source)
  }
  t->shrink_to_fit();
}

// One honest case: well-formed tables, any match and want.
static void honest_case() {
  const uint64_t B = 2 + rnd() % 70;  // the block size
  const uint32_t nsrc = 1 + (uint32_t)(rnd() % 3);
  const sources::BlockList need = random_list(B, 6, 1);
  const sources::BlockList pool = random_list(B, 6, nsrc);
  const uint64_t n = need.n, nwords = (n + 63) / 64;
  uint32_t* match = (uint32_t*)malloc(n ? n * 4 : 1);
  uint64_t* want = rnd() % 3 ? (uint64_t*)malloc(nwords ? nwords * 8 : 1) : nullptr;
  // matches: mostly stretches of consecutive pool ordinals, some repeats, some none
  uint64_t j = pool.n ? rnd() % pool.n : 0;
  for (uint64_t g = 0; g < n; ++g) {
    const uint64_t k = rnd() % 16;
    if (k == 0 || pool.n == 0)
      match[g] = sources::kNone;
    else if (k == 1)
      match[g] = (uint32_t)(pool.n + rnd() % 3);  // past the pool: none
    else if (k == 2)
      match[g] = (uint32_t)(j = rnd() % pool.n);
    else if (k == 3)
      match[g] = (uint32_t)j;  // the same pool block again
    else
      match[g] = (uint32_t)(j = (j + 1) % pool.n);
  }
  for (uint64_t w = 0; want && w < nwords; ++w) want[w] = rnd() | rnd() | (rnd() % 4 ? 0 : ~0ull);

  // the double loop
  std::vector<Plain> plain(n);
  for (uint64_t g = 0; g < n; ++g) plain[g] = plain_block(need, pool, B, want, match, g);
  std::vector<sources::Extent> ref;
  auto joined = [&](uint64_t g) {  // does g continue g - 1?
    const Plain &a = plain[g - 1], &b = plain[g];
    return a.found && b.found && a.run == b.run && a.src == b.src && a.file == b.file &&
           b.block == a.block + 1;
  };
  for (uint64_t g = 0; g < n; ++g) {
    if (!plain[g].found || (g && joined(g))) continue;
    uint64_t e = g;
    while (e + 1 < n && joined(e + 1)) ++e;
    const Plain& h = plain[g];
    const uint64_t count = e - g + 1;
    const uint64_t end = (h.need_block + count) * B < h.size ? (h.need_block + count) * B : h.size;
    ref.push_back(sources::Extent{g, count, h.need_file, h.need_block, h.src, h.file, h.block,
                                  end - h.need_block * B});
  }

  // the rule's text, as the kernels use it
  std::vector<uint64_t> nt, pt;
  tables_of(need, &nt);
  tables_of(pool, &pt);
  const extents::Tables t{match, n, nt.data(), need.runs.size(), pt.data(), pool.runs.size(),
                          pool.n, B, want};
  std::vector<extents::Map> maps(n + 1);
  for (uint64_t g = 0; g <= n; ++g) maps[g] = extents::map_block(t, g);  // (g == n: in no file)
  CHECK(maps[n].flags == 0 && maps[n].src == extents::kNoSrc);
  std::vector<sources::Extent> byrule;
  for (uint64_t g = 0; g < n; ++g) {
    const extents::Map& m = maps[g];
    const Plain& p = plain[g];
    CHECK(p.in_file);  // (honest tables: every block lies in a file)
    CHECK(!!(m.flags & extents::kWanted) == p.wanted);
    CHECK(!!(m.flags & extents::kFound) == p.found);
    CHECK(!!(m.flags & extents::kDropped) == p.dropped);
    CHECK(m.run == p.run && m.need_file == p.need_file && m.need_block == p.need_block);
    if (p.found) {
      CHECK(m.src == p.src && m.file == p.file && m.block == p.block && m.len == p.len);
    } else {
      CHECK(m.src == extents::kNoSrc && m.file == extents::kNone64 && m.block == extents::kNone64 &&
            m.len == 0);
    }
    const bool head = p.found && !(g && extents::cont(maps[g - 1], m));
    const bool tail = p.found && !extents::cont(m, maps[g + 1]);
    if (head)
      byrule.push_back(sources::Extent{g, 0, m.need_file, m.need_block, m.src, m.file, m.block, 0});
    if (tail) {
      CHECK(!byrule.empty());
      sources::Extent& e = byrule.back();
      e.count = g - e.first + 1;
      e.bytes = extents::extent_bytes(e.need_block, m.need_end, B);
    }
  }
  CHECK(byrule.size() == ref.size());
  CHECK(ref.empty() || memcmp(byrule.data(), ref.data(), ref.size() * sizeof(sources::Extent)) == 0);

  // the host path: map_matches, then extents_of
  uint32_t* so = (uint32_t*)malloc(n ? n * 4 : 1);
  uint64_t* fo = (uint64_t*)malloc(n ? n * 8 : 1);
  uint64_t* bo = (uint64_t*)malloc(n ? n * 8 : 1);
  uint64_t* fetch = (uint64_t*)malloc(nwords ? nwords * 8 : 1);
  const sources::MapStats ms = sources::map_matches(need, pool, B, want, match, so, fo, bo);
  std::vector<sources::Extent> host;
  const uint64_t left = sources::extents_of(need, B, want, so, fo, bo, &host, fetch);
  CHECK(host.size() == ref.size());
  CHECK(ref.empty() || memcmp(host.data(), ref.data(), ref.size() * sizeof(sources::Extent)) == 0);
  uint64_t wanted = 0, found = 0, bytes = 0;
  for (uint64_t g = 0; g < n; ++g) {
    const Plain& p = plain[g];
    wanted += p.wanted;
    found += p.found;
    bytes += p.found ? p.len : 0;
    CHECK((fetch[g / 64] >> (g % 64) & 1) == (uint64_t)(p.wanted && !p.found));
  }
  for (uint64_t g = n; g < 64 * nwords; ++g) CHECK(!(fetch[g / 64] >> (g % 64) & 1));
  CHECK(ms.wanted == wanted && ms.found == found && ms.bytes == bytes && left == wanted - found);
  uint64_t sum = 0;
  for (const sources::Extent& e : ref) sum += e.bytes;
  CHECK(sum == bytes);
  // the same through the tail the whole calls share: the records and the
  // bitmap come back malloc'd and are this case's to free (the leak check
  // watches the ownership)
  uint64_t* o_rec = nullptr;
  uint64_t* o_fetch = nullptr;
  size_t o_count = ~(size_t)0;
  uint64_t o_left = ~0ull;
  CHECK(sources::extents_owned(need, B, want, so, fo, bo, &o_rec, &o_count, &o_fetch, &o_left));
  CHECK(o_count == ref.size() && (o_rec == nullptr) == ref.empty());
  CHECK(ref.empty() || memcmp(o_rec, ref.data(), ref.size() * sizeof(sources::Extent)) == 0);
  CHECK(o_fetch != nullptr && o_left == wanted - found);
  for (uint64_t g = 0; g < 64 * nwords; ++g)
    CHECK((o_fetch[g / 64] >> (g % 64) & 1) == (uint64_t)(g < n && plain[g].wanted && !plain[g].found));
  free(o_rec);
  free(o_fetch);
  free(so);
  free(fo);
  free(bo);
  free(fetch);
  free(match);
  free(want);
}

// One hostile case: the tables hold anything.  No answer is checked; the
// sanitizers watch the reads.
static void hostile_case() {
  const uint64_t n = rnd() % 200, nr = rnd() % 9, pr = rnd() % 9, nwords = (n + 63) / 64;
  uint32_t* match = (uint32_t*)malloc(n ? n * 4 : 1);
  uint64_t* nt = (uint64_t*)malloc(nr ? nr * 32 : 1);
  uint64_t* pt = (uint64_t*)malloc(pr ? pr * 32 : 1);
  uint64_t* want = rnd() % 2 ? (uint64_t*)malloc(nwords ? nwords * 8 : 1) : nullptr;
  auto any = [&]() -> uint64_t {
    switch (rnd() % 5) {
      case 0: return ~0ull;
      case 1: return rnd();
      case 2: return rnd() % 4;
      default: return rnd() % 300;
    }
  };
  for (uint64_t i = 0; i < 4 * nr; ++i) nt[i] = any();
  for (uint64_t i = 0; i < 4 * pr; ++i) pt[i] = any();
  for (uint64_t g = 0; g < n; ++g) match[g] = (uint32_t)any();
  for (uint64_t w = 0; want && w < nwords; ++w) want[w] = rnd();
  const uint64_t n_pool = rnd() % 3 ? rnd() % 400 : 0x7FFFFFFFull;
  const uint64_t bs = rnd() % 4 ? 1 + rnd() % 100 : (rnd() % 2 ? 1 : ~0ull);
  const extents::Tables t{match, n, nt, nr, pt, pr, n_pool, bs, want};
  uint64_t heads = 0, tails = 0;
  extents::Map prev = extents::map_block(t, 0);
  for (uint64_t g = 0; g < n; ++g) {
    const extents::Map m = g ? extents::map_block(t, g) : prev;
    const extents::Map next = extents::map_block(t, g + 1);
    const bool found = m.flags & extents::kFound;
    heads += found && !(g && extents::cont(prev, m));
    tails += found && !extents::cont(m, next);
    prev = m;
  }
  CHECK(heads == tails);  // (they alternate whatever the tables hold: the emit pass relies on it)
  free(match);
  free(nt);
  free(pt);
  free(want);
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (g_case = 0; g_case < cases; ++g_case) {
    if (g_case % 8 == 7)
      hostile_case();
    else
      honest_case();
  }
  printf("extents_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
