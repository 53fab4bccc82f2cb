// The in-place update rule (ciruela_amd/csrc/update.hpp, over copyblk.hpp)
// under ASan + UBSan: a stand-alone host program, no device code.
//
//   update_fuzz [cases] [seed]
//
// Per case a seeded random layout in one heap arena of exactly its size:
//   * one to four resident buffers, disjoint, at any alignment, of whole blocks
//     or with a tail; block sizes 16, 48, 1000 and 4096;
//   * one to six files of the new image whose destinations are a resident
//     buffer itself, a resident buffer shifted by k blocks, shifted by 1 to 15
//     bytes, begun inside one and ending outside it, fresh memory, or absent --
//     pairwise disjoint, as the call requires;
//   * content drawn from a few block contents, so equal blocks abound (one case
//     in eight is a single content: the file of zeros); the digests are made
//     from the content's number and the length, the arena holds its bytes;
//   * a match array as the join would give it (the smallest ordinal with the
//     digest), then damaged: no match, an ordinal past the pool, an ordinal of
//     another length, any ordinal;
//   * a cap: 0, "all", exactly what the candidates need, or something between.
// update::plan_host runs (once to learn the scratch, which is then allocated at
// exactly its size), then copyblk::apply_host on table A and on table B.  A
// block-by-block model that finds files and buffers by walking them, and works
// from a snapshot of the arena taken beforehand, gives the classes, the bitmap,
// every count and both tables; every taken block's destination must hold the
// snapshot's source bytes and every other byte of the arena must be unchanged;
// that no destination of table A meets a source of table A, and none of table
// B a source of table B, is checked on the tables themselves.
// update::spans_overlap is checked against all pairs.
// Exit status 0 and "update_fuzz: N cases ok" on stdout; the totals go to
// stderr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
#include <vector>

#include "update.hpp"

using namespace cir;

namespace {

struct Totals {
  uint64_t blocks = 0, kept = 0, direct = 0, staged = 0, demoted = 0, dropped = 0, none = 0;
} tot;

[[noreturn]] void die(const char* what, uint64_t c) {
  fprintf(stderr, "update_fuzz: case %llu: %s\n", (unsigned long long)c, what);
  exit(1);
}

uint64_t units_of(uint64_t bytes) { return (bytes + 15) / 16; }

uint8_t content_byte(uint32_t id, uint64_t i) { return (uint8_t)((id * 131u + 7u) * (i + 1) >> 3); }

void digest_of(uint32_t id, uint64_t len, uint8_t* out) {
  uint64_t x = 0x9E3779B97F4A7C15ull * (id + 1) ^ (len << 20);
  for (int i = 0; i < 32; ++i) {
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    out[i] = (uint8_t)(x >> 56);
  }
}

struct Buf {
  uint64_t off, size;  // in the arena
};

template <class T>
std::unique_ptr<T[]> dup(const std::vector<T>& v) {  // (exactly sized: a read past it is an ASan report)
  std::unique_ptr<T[]> q(new T[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(q.get(), v.data(), sizeof(T) * v.size());
  return q;
}

// Do a table's destinations meet its sources?
bool table_self_overlap(const uint64_t* runs, uint64_t n) {
  struct S {
    uint64_t lo, hi;
    int dst;
  };
  std::vector<S> v;
  for (uint64_t r = 0; r < n; ++r) {
    v.push_back({runs[4 * r + 1], runs[4 * r + 1] + runs[4 * r + 3], 0});
    v.push_back({runs[4 * r + 2], runs[4 * r + 2] + runs[4 * r + 3], 1});
  }
  std::sort(v.begin(), v.end(), [](const S& a, const S& b) { return a.lo < b.lo; });
  uint64_t end[2] = {0, 0};
  for (const S& s : v) {
    if (s.lo < end[!s.dst]) return true;
    if (s.dst && s.lo < end[1]) return true;  // (two destinations)
    end[s.dst] = std::max(end[s.dst], s.hi);
  }
  return false;
}

void spans_case(uint64_t c, std::mt19937_64& rng) {
  const size_t n = (size_t)(rng() % 7);
  std::vector<std::pair<uint64_t, uint64_t>> v;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t lo = rng() % 200, len = rng() % 5 ? 1 + rng() % 30 : 0;
    v.push_back({lo, lo + len});
  }
  bool want = false;
  for (size_t i = 0; i < n; ++i)
    for (size_t j = i + 1; j < n; ++j)
      if (v[i].first < v[i].second && v[j].first < v[j].second && v[i].first < v[j].second &&
          v[j].first < v[i].second)
        want = true;
  if (update::spans_overlap(v) != want) die("spans_overlap differs from all pairs", c);
}

void plan_case(uint64_t c, std::mt19937_64& rng) {
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const uint64_t bs_choices[] = {16, 48, 1000, 4096};
  const uint64_t bs = bs_choices[rng() % 4];
  auto nblk_of = [&](uint64_t size) { return (size + bs - 1) / bs; };
  auto size_of = [&]() {
    const uint64_t kinds[] = {1, bs - 1, bs, bs + 1, 3 * bs + 5, bs * pick(1, 12),
                              bs * pick(1, 12) + pick(1, bs - 1), 70 * bs};
    return kinds[rng() % 8];
  };
  // the resident buffers, in address order with gaps
  const size_t nhave = (size_t)pick(1, 4);
  std::vector<Buf> held(nhave);
  uint64_t pos = pick(0, 40);
  for (Buf& b : held) {
    b.off = pos;
    b.size = size_of();
    pos += b.size + (rng() % 3 ? pick(0, 2 * bs + 20) : 0);
  }
  const uint64_t fresh0 = pos + pick(0, 31);
  // the files and their destinations
  const size_t nfiles = (size_t)pick(1, 6);
  std::vector<uint64_t> sizes(nfiles), doff(nfiles, ~0ull);  // (~0: no destination)
  uint64_t fresh = fresh0;
  for (size_t i = 0; i < nfiles; ++i) {
    const Buf& b = held[rng() % nhave];
    uint64_t at = ~0ull;
    sizes[i] = rng() % 8 == 0 ? 0 : rng() % 3 ? b.size : size_of();
    switch (rng() % 8) {
      case 0: case 1: case 2: at = b.off; break;                    // the buffer itself
      case 3: at = b.off + bs * pick(1, 3); break;                  // shifted by whole blocks
      case 4: at = b.off + pick(1, 15); break;                      // shifted by odd bytes
      case 5: at = b.off + b.size - std::min<uint64_t>(b.size, pick(1, 2 * bs)); break;  // partly in
      case 6: break;                                                // none
      default: at = fresh; break;                                   // fresh memory
    }
    if (at != ~0ull && sizes[i]) {
      for (size_t k = 0; k < i; ++k)
        if (doff[k] != ~0ull && sizes[k] && at < doff[k] + sizes[k] && doff[k] < at + sizes[i])
          at = fresh;  // (pairwise disjoint: the fresh zone lies behind everything so far)
      fresh = std::max(fresh, at + sizes[i] + pick(0, 40));
    }
    doff[i] = at;
  }
  const uint64_t arena_bytes = fresh + 16;
  std::unique_ptr<uint8_t[]> arena(new uint8_t[arena_bytes]);
  for (uint64_t i = 0; i < arena_bytes; ++i) arena[i] = (uint8_t)rng();
  const uint64_t base = (uint64_t)(uintptr_t)arena.get();
  // the resident content
  const uint32_t nids = rng() % 8 == 0 ? 1 : (uint32_t)pick(2, 9);
  std::vector<uint64_t> have;
  std::vector<uint32_t> pool_id;
  std::vector<uint64_t> pool_len;
  uint64_t n_pool = 0;
  for (const Buf& b : held) {
    const uint64_t rec[3] = {n_pool, base + b.off, b.size};
    have.insert(have.end(), rec, rec + 3);
    for (uint64_t j = 0; j < nblk_of(b.size); ++j) {
      const uint64_t len = std::min(bs, b.size - j * bs);
      const uint32_t id = (uint32_t)(rng() % nids);
      pool_id.push_back(id);
      pool_len.push_back(len);
      for (uint64_t i = 0; i < len; ++i) arena[b.off + j * bs + i] = content_byte(id, i);
    }
    n_pool += nblk_of(b.size);
  }
  std::vector<uint8_t> pool_dig((size_t)(32 * n_pool));
  for (uint64_t m = 0; m < n_pool; ++m) digest_of(pool_id[m], pool_len[m], &pool_dig[32 * m]);
  // which resident block stands at an arena offset, block-aligned?  ~0: none
  auto block_under = [&](uint64_t off) -> uint64_t {
    uint64_t first = 0;
    for (const Buf& b : held) {
      if (off >= b.off && off < b.off + b.size && (off - b.off) % bs == 0)
        return first + (off - b.off) / bs;
      first += nblk_of(b.size);
    }
    return ~0ull;
  };
  // the new image: its content, digests, runs, dests and the match array
  std::vector<uint64_t> runs, dests(nfiles, 0);
  std::vector<uint8_t> need_dig;
  std::vector<uint32_t> match;
  uint64_t n_need = 0;
  for (size_t i = 0; i < nfiles; ++i) {
    if (doff[i] != ~0ull) dests[i] = base + doff[i];
    if (!sizes[i]) continue;
    const uint64_t run[4] = {n_need, sizes[i], (uint64_t)i, rng()};
    runs.insert(runs.end(), run, run + 4);
    for (uint64_t j = 0; j < nblk_of(sizes[i]); ++j, ++n_need) {
      const uint64_t len = std::min(bs, sizes[i] - j * bs);
      const uint64_t under = doff[i] != ~0ull ? block_under(doff[i] + j * bs) : ~0ull;
      // what stands there already, some other resident content, or new content
      uint32_t id = (uint32_t)(rng() % nids);
      if (under != ~0ull && rng() % 3) id = pool_id[under];
      if (rng() % 6 == 0) id = 1000 + (uint32_t)(rng() % 50);
      uint8_t dig[32];
      digest_of(id, len, dig);
      need_dig.insert(need_dig.end(), dig, dig + 32);
      // the join's answer: the smallest ordinal with this digest ...
      uint32_t m = copyblk::kNoMatch;
      for (uint64_t q = 0; q < n_pool && m == copyblk::kNoMatch; ++q)
        if (pool_id[q] == id && pool_len[q] == len) m = (uint32_t)q;
      // ... then damaged
      switch (rng() % 12) {
        case 0: m = copyblk::kNoMatch; break;
        case 1: m = (uint32_t)(n_pool + rng() % 3); break;
        case 2: m = (uint32_t)(rng() % n_pool); break;
        case 3:  // an ordinal of another length, where there is one
          for (uint64_t q = 0; q < n_pool; ++q)
            if (pool_len[q] != len) m = (uint32_t)q;
          break;
        default: break;
      }
      match.push_back(m);
    }
  }
  // the cap: candidates are counted by the model below, so draw it lazily
  const uint64_t cap_kind = rng() % 5, cap_draw = rng();

  // ---- the model, from a snapshot
  std::vector<uint8_t> snap(arena.get(), arena.get() + arena_bytes), want = snap;
  struct Blk {
    uint32_t cls;
    bool dropped;
    uint64_t src, dst, len;  // arena offsets
  };
  std::vector<Blk> model;
  uint64_t cand_units = 0;
  for (size_t i = 0; i < nfiles; ++i)
    for (uint64_t j = 0; j < nblk_of(sizes[i]); ++j) {
      const uint64_t g = model.size();
      Blk k{update::kNone, false, 0, 0, std::min(bs, sizes[i] - j * bs)};
      model.push_back(k);
      if (doff[i] == ~0ull) continue;
      Blk& o = model.back();
      o.dst = doff[i] + j * bs;
      const uint64_t under = block_under(o.dst);
      if (under != ~0ull && pool_len[under] == o.len &&
          !memcmp(&pool_dig[32 * under], &need_dig[32 * g], 32)) {
        o.cls = update::kKept;
        continue;
      }
      const uint32_t m = match[g];
      if (m == copyblk::kNoMatch || m >= n_pool) continue;
      if (pool_len[m] != o.len) {
        o.dropped = true;
        continue;
      }
      uint64_t first = 0;
      for (const Buf& b : held) {
        if (m < first + nblk_of(b.size)) {
          o.src = b.off + (m - first) * bs;
          break;
        }
        first += nblk_of(b.size);
      }
      bool over = false;
      for (const Buf& b : held) over |= o.dst < b.off + b.size && b.off < o.dst + o.len;
      o.cls = over ? update::kStaged : update::kDirect;
      if (over) cand_units += units_of(o.len);
    }
  const uint64_t cap = cap_kind == 0   ? 0
                       : cap_kind == 1 ? update::kNoCap
                       : cap_kind == 2 ? cand_units
                                       : cap_draw % (cand_units + 2);

  // ---- the rule
  const auto m_ = dup(match);
  const auto runs_ = dup(runs), have_ = dup(have), dests_ = dup(dests);
  const auto pool_ = dup(pool_dig), need_ = dup(need_dig);
  update::Plan p{{m_.get(), n_need, runs_.get(), runs.size() / 4, dests_.get(), nfiles, have_.get(),
                  nhave, n_pool, bs},
                 pool_.get(),
                 need_.get(),
                 cap,
                 0};
  const uint64_t nwords = (n_need + 63) / 64;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[nwords ? nwords : 1]);
  std::unique_ptr<uint64_t[]> ta(new uint64_t[4 * (n_need ? n_need : 1)]);
  std::unique_ptr<uint64_t[]> tb(new uint64_t[4 * (n_need ? n_need : 1)]);
  uint64_t res[update::kResFields], res2[update::kResFields];
  update::plan_host(p, bits.get(), ta.get(), tb.get(), res);
  const uint64_t scratch_bytes = 16 * res[update::kBUnits];
  if (cap != update::kNoCap && res[update::kBUnits] > cap) die("the scratch exceeds the cap", c);
  std::unique_ptr<uint8_t[]> scratch(new uint8_t[scratch_bytes ? scratch_bytes : 1]);
  p.scratch = (uint64_t)(uintptr_t)scratch.get();
  for (uint64_t w = 0; w < nwords; ++w) bits[w] = ~0ull;  // (every word must be written)
  update::plan_host(p, bits.get(), ta.get(), tb.get(), res2);
  if (memcmp(res, res2, sizeof res)) die("the counts depend on the scratch's address", c);

  // the model's cut, tables, bitmap and counts
  uint64_t e[update::kResFields] = {};
  uint64_t prefix = 0;
  for (uint64_t g = 0; g < n_need; ++g) {
    const Blk& o = model[g];
    if (o.dropped) ++e[update::kDroppedMatches];
    bool have_bit = o.cls != update::kNone;
    uint64_t to = base + o.dst;
    if (o.cls == update::kKept) {
      ++e[update::kKeptBlocks];
      e[update::kKeptBytes] += o.len;
    } else if (o.cls == update::kDirect) {
      ++e[update::kDirectBlocks];
      e[update::kDirectBytes] += o.len;
      ++e[update::kCandARecs];
      e[update::kCandAUnits] += units_of(o.len);
    } else if (o.cls == update::kStaged) {
      ++e[update::kCandARecs];
      e[update::kCandAUnits] += units_of(o.len);
      ++e[update::kCandSRecs];
      e[update::kCandSUnits] += units_of(o.len);
      const uint64_t at = prefix;
      prefix += units_of(o.len);
      if (cap == update::kNoCap || prefix <= cap) {
        to = p.scratch + 16 * at;
        const uint64_t* q = tb.get() + 4 * e[update::kBRecs];
        if (e[update::kBRecs] >= res[update::kBRecs] || q[0] != e[update::kBUnits] || q[1] != to ||
            q[2] != base + o.dst || q[3] != o.len)
          die("a record of table B differs", c);
        ++e[update::kBRecs];
        e[update::kBUnits] += units_of(o.len);
        e[update::kStagedBytes] += o.len;
      } else {
        have_bit = false;
        ++e[update::kDemotedBlocks];
        e[update::kDemotedBytes] += o.len;
      }
    }
    if (((bits[g >> 6] >> (g & 63)) & 1) != (have_bit ? 1u : 0u)) die("a bit differs", c);
    if (!have_bit || o.cls == update::kKept) continue;
    const uint64_t* q = ta.get() + 4 * e[update::kARecs];
    if (e[update::kARecs] >= res[update::kARecs] || q[0] != e[update::kAUnits] ||
        q[1] != base + o.src || q[2] != to || q[3] != o.len)
      die("a record of table A differs", c);
    ++e[update::kARecs];
    e[update::kAUnits] += units_of(o.len);
    memcpy(&want[o.dst], &snap[o.src], o.len);
  }
  for (uint64_t b = n_need; b < 64 * nwords; ++b)
    if ((bits[b >> 6] >> (b & 63)) & 1) die("a bit past the last block is set", c);
  for (int i = 0; i < update::kResFields; ++i)
    if (res[i] != e[i]) die("a count differs", (uint64_t)i * 1000000 + c);
  if (update::classify(p, n_need).cls || update::classify(p, ~0ull).cls)
    die("a block past the image has a class", c);
  if (table_self_overlap(ta.get(), res[update::kARecs])) die("table A writes what it reads", c);
  if (table_self_overlap(tb.get(), res[update::kBRecs])) die("table B writes what it reads", c);

  // ---- the copies
  const std::unique_ptr<uint64_t[]> xa(new uint64_t[4 * res[update::kARecs] + 1]);
  const std::unique_ptr<uint64_t[]> xb(new uint64_t[4 * res[update::kBRecs] + 1]);
  memcpy(xa.get(), ta.get(), 32 * res[update::kARecs]);
  memcpy(xb.get(), tb.get(), 32 * res[update::kBRecs]);
  if (copyblk::apply_host(xa.get(), res[update::kARecs], res[update::kAUnits]))
    die("table A has a bad record", c);
  if (copyblk::apply_host(xb.get(), res[update::kBRecs], res[update::kBUnits]))
    die("table B has a bad record", c);
  if (memcmp(arena.get(), want.data(), arena_bytes)) {
    for (uint64_t i = 0; i < arena_bytes; ++i)
      if (arena[i] != want[i]) {
        fprintf(stderr, "update_fuzz: byte %llu of %llu\n", (unsigned long long)i,
                (unsigned long long)arena_bytes);
        break;
      }
    die("the arena is not the model's", c);
  }
  tot.blocks += n_need;
  tot.kept += e[update::kKeptBlocks];
  tot.direct += e[update::kDirectBlocks];
  tot.staged += e[update::kBRecs];
  tot.demoted += e[update::kDemotedBlocks];
  tot.dropped += e[update::kDroppedMatches];
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 3000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (uint64_t c = 0; c < cases; ++c) {
    std::mt19937_64 rng(seed * 1000003 + c);
    spans_case(c, rng);
    plan_case(c, rng);
  }
  fprintf(stderr,
          "update_fuzz: %llu blocks; %llu kept, %llu direct, %llu staged, %llu demoted, %llu "
          "dropped\n",
          (unsigned long long)tot.blocks, (unsigned long long)tot.kept,
          (unsigned long long)tot.direct, (unsigned long long)tot.staged,
          (unsigned long long)tot.demoted, (unsigned long long)tot.dropped);
  printf("update_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
