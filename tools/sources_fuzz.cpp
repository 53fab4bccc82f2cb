// Seeded fuzz of ciruela_amd/csrc/sources.hpp (the host side of
// cir_block_sources: the block lists, the pool, the host join and the mapping
// of a pool ordinal back to source, file and block) against an O(n m) double
// loop.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/sources_fuzz.cpp ciruela_amd/csrc/dirsig.cpp -o build/sources_fuzz
// and run it; tests/test_block_sources_cpu.py does.  Every case emits random
// small indexes (dirsig::Emitter), parses them back (dirsig::parse) and holds
// the digest lists, the match array and the three result arrays in heap
// buffers of exactly their size, so a read or a write one element outside is
// an AddressSanitizer report.
//
// usage: sources_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dirsig.hpp"
#include "sources.hpp"

using namespace cir;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

struct Digest {
  uint8_t b[32];
};

// A random index of the given block size, its digests drawn from `universe`
// (so that equal digests occur, at blocks of any length), parsed back.
static bool random_index(uint64_t bs, const std::vector<Digest>& universe, dirsig::Index* out) {
  dirsig::Header h;
  h.block_size = bs;
  dirsig::Emitter em(h);
  const int ndirs = 1 + (int)(rnd() % 3);
  for (int d = 0; d < ndirs; ++d) {
    em.start_dir(d == 0 ? "/" : "/d" + std::to_string(d));
    const int nfiles = (int)(rnd() % 5);
    for (int f = 0; f < nfiles; ++f) {
      const std::string name = "f" + std::to_string(f);
      if (rnd() % 6 == 0) {
        em.add_symlink(name, "target");
        continue;
      }
      static const uint64_t kFull[] = {0, 0, 1, 2, 3, 9};
      const uint64_t nfull = kFull[rnd() % 6];
      const uint64_t tail = rnd() % 3 == 0 ? 1 + rnd() % (bs - 1) : 0;
      const uint64_t nb = nfull + (tail != 0);
      std::vector<uint8_t> hs(32 * nb);
      for (uint64_t k = 0; k < nb; ++k)
        memcpy(hs.data() + 32 * k, universe[rnd() % universe.size()].b, 32);
      em.add_file(name, rnd() % 4 == 0, nfull * bs + tail, hs.data(), nb);
    }
  }
  static const uint8_t footer[32] = {1};
  size_t len = 0;
  uint8_t* raw = em.finish_malloc(footer, 32, &len);
  if (!raw) return false;
  std::string err;
  const bool ok = dirsig::parse(raw, len, out, &err);
  free(raw);
  if (!ok) fprintf(stderr, "parse: %s\n", err.c_str());
  return ok;
}

struct Place {
  uint32_t src;
  uint64_t file, block, size;
  const uint8_t* digest;
};

static void places(const dirsig::Index& idx, uint32_t src, std::vector<Place>* out) {
  uint64_t file = 0;
  for (const dirsig::Entry& en : idx.entries) {
    if (en.kind != dirsig::EntryKind::kFile) continue;
    for (uint64_t b = 0; b < en.hashes.size() / 32; ++b)
      out->push_back(Place{src, file, b, en.size, en.hashes.data() + 32 * b});
    ++file;
  }
}

static int one(uint64_t id) {
  const uint64_t bs = 2 + rnd() % 40;
  std::vector<Digest> universe(1 + rnd() % 24);
  for (Digest& d : universe)
    for (uint8_t& c : d.b) c = (uint8_t)rnd();
  dirsig::Index idx;
  if (!random_index(bs, universe, &idx)) return 1;
  const size_t nsrc = rnd() % 5;
  std::vector<dirsig::Index> srcs(nsrc);
  std::vector<bool> usable(nsrc);
  for (size_t s = 0; s < nsrc; ++s) {
    if (!random_index(bs, universe, &srcs[s])) return 1;
    usable[s] = rnd() % 5 != 0;  // (a skipped source keeps its ordinal out of the result)
  }
  // the library's way
  sources::BlockList need, pool;
  sources::append_runs(idx, 0, &need);
  uint64_t n_pool = 0;
  for (size_t s = 0; s < nsrc; ++s)
    if (usable[s]) n_pool += sources::count_blocks(srcs[s]);
  uint8_t* need_d = (uint8_t*)malloc(32 * need.n + 1);  // (+1: malloc(0) may be null)
  uint8_t* pool_d = (uint8_t*)malloc(32 * n_pool + 1);
  sources::copy_digests(idx, need_d);
  for (size_t s = 0; s < nsrc; ++s)
    if (usable[s]) {
      sources::copy_digests(srcs[s], pool_d + 32 * pool.n);
      sources::append_runs(srcs[s], (uint32_t)s, &pool);
    }
  if (pool.n != n_pool || need.n != sources::count_blocks(idx)) {
    fprintf(stderr, "case %llu: block counts disagree\n", (unsigned long long)id);
    return 1;
  }
  const uint64_t nwords = (need.n + 63) / 64;
  uint64_t* want = nullptr;
  if (rnd() % 2) {
    want = (uint64_t*)malloc(8 * nwords + 1);
    for (uint64_t w = 0; w < nwords; ++w) want[w] = rnd() | (rnd() % 2 ? ~0ull << (need.n & 63) : 0);
  }
  uint32_t* match = (uint32_t*)malloc(4 * need.n + 1);
  uint32_t* so = (uint32_t*)malloc(4 * need.n + 1);
  uint64_t* fo = (uint64_t*)malloc(8 * need.n + 1);
  uint64_t* bo = (uint64_t*)malloc(8 * need.n + 1);
  sources::host_join(need_d, need.n, pool_d, n_pool, want, match, rnd());
  const sources::MapStats st = sources::map_matches(need, pool, bs, want, match, so, fo, bo);
  // the double loop
  std::vector<Place> np, pp;
  places(idx, 0, &np);
  for (size_t s = 0; s < nsrc; ++s)
    if (usable[s]) places(srcs[s], (uint32_t)s, &pp);
  int bad = np.size() != need.n || pp.size() != n_pool;
  uint64_t wanted = 0, found = 0, bytes = 0, dropped = 0;
  for (uint64_t g = 0; g < np.size() && !bad; ++g) {
    uint32_t ws = sources::kNone;
    uint64_t wf = sources::kNone64, wb = sources::kNone64;
    if (!want || (want[g >> 6] >> (g & 63) & 1)) {
      ++wanted;
      for (const Place& p : pp)
        if (memcmp(p.digest, np[g].digest, 32) == 0) {
          const uint64_t a = sources::block_len(np[g].size, bs, np[g].block);
          if (sources::block_len(p.size, bs, p.block) == a) {
            ws = p.src;
            wf = p.file;
            wb = p.block;
            ++found;
            bytes += a;
          } else {
            ++dropped;
          }
          break;  // the first place, whatever its length
        }
    }
    if (so[g] != ws || fo[g] != wf || bo[g] != wb) {
      fprintf(stderr, "case %llu: block %llu is (%u, %llu, %llu), want (%u, %llu, %llu)\n",
              (unsigned long long)id, (unsigned long long)g, so[g], (unsigned long long)fo[g],
              (unsigned long long)bo[g], ws, (unsigned long long)wf, (unsigned long long)wb);
      bad = 1;
    }
  }
  if (!bad && (st.wanted != wanted || st.found != found || st.bytes != bytes ||
               st.dropped != dropped)) {
    fprintf(stderr, "case %llu: stats disagree\n", (unsigned long long)id);
    bad = 1;
  }
  // every pool ordinal maps back to its place
  for (uint64_t j = 0; j < pp.size() && !bad; ++j) {
    const sources::FileRun& r = sources::run_of(pool, j);
    if (r.src != pp[j].src || r.file != pp[j].file || j - r.first != pp[j].block ||
        r.size != pp[j].size) {
      fprintf(stderr, "case %llu: pool ordinal %llu maps wrong\n", (unsigned long long)id,
              (unsigned long long)j);
      bad = 1;
    }
  }
  free(need_d);
  free(pool_d);
  free(want);
  free(match);
  free(so);
  free(fo);
  free(bo);
  return bad;
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 3000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20240611;
  // the limit of a pool, which no index a test may hold can reach
  if (!sources::pool_count_ok(0) || !sources::pool_count_ok((1ull << 31) - 1) ||
      sources::pool_count_ok(1ull << 31) || sources::pool_count_ok(~0ull)) {
    fprintf(stderr, "pool_count_ok: the limit is not 2^31-1\n");
    return 1;
  }
  if (sources::block_len(130, 64, 2) != 2 || sources::block_len(128, 64, 1) != 64 ||
      sources::block_len(~0ull, 1ull << 32, (1ull << 32) - 1) != (1ull << 32) - 1) {
    fprintf(stderr, "block_len is wrong\n");
    return 1;
  }
  uint64_t ran = 0;
  for (uint64_t i = 0; i < cases; ++i) {
    if (one(i)) return 1;
    ++ran;
  }
  printf("sources_fuzz: %llu cases ok\n", (unsigned long long)ran);
  return 0;
}
