// The copy and plan rules (ciruela_amd/csrc/copyblk.hpp) under ASan + UBSan: a
// stand-alone host program, no device code.
//
//   copyblk_fuzz [cases] [seed]
//
// Per case:
//   * a seeded random copy table over heap buffers of exactly their size: every
//     source sits at an alignment of its own (0 .. 15) in a buffer of exactly
//     skew + bytes bytes, so a read past a source is an ASan report; every
//     destination at an alignment of its own between two poisoned redzones;
//     runs of 1 to 4101 bytes; over the cases every one of the 16 x 16
//     alignment pairs occurs.  copyblk::apply_host runs the table; the
//     destinations are compared with a byte-by-byte restatement, redzones
//     included, and the sources with what they held;
//   * the same table damaged -- zero bytes, a wrong unit_first, a wrong unit
//     total -- against a sequential restatement of the bad set: exactly those
//     records are counted, nothing of them is written, and every other record
//     holds its own bytes or nothing (a unit_first that steps back can hide
//     the record in front of it from the bisection);
//   * the plan's rule (copyblk::take_of, plan_host) over random files, resident
//     buffers, match arrays (matches, none, ordinals past the pool), missing
//     destinations and tails of other lengths, against a block-by-block loop
//     that finds files and buffers by walking them.
// Exit status 0 and "copyblk_fuzz: N cases ok" on stdout; the totals go to
// stderr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "copyblk.hpp"

using namespace cir;

namespace {

constexpr size_t kRedzone = 48;
constexpr uint8_t kPoison = 0xA5;

struct Totals {
  uint64_t records = 0, units = 0, bytes = 0, damaged = 0, bad = 0, blocks = 0, taken = 0,
           dropped = 0;
  bool pair[16][16] = {};
} tot;

[[noreturn]] void die(const char* what, uint64_t c) {
  fprintf(stderr, "copyblk_fuzz: case %llu: %s\n", (unsigned long long)c, what);
  exit(1);
}

uint64_t units_of(uint64_t bytes) { return bytes / 16 + (bytes % 16 != 0); }

struct Rec {
  std::vector<uint8_t> data;
  std::unique_ptr<uint8_t[]> src, dst;  // skew + bytes; skew + redzone + bytes + redzone
  size_t sa = 0, da = 0;
  uint8_t* s() const { return src.get() + sa; }
  uint8_t* d() const { return dst.get() + da + kRedzone; }
  size_t dst_size() const { return da + kRedzone + data.size() + kRedzone; }
};

// the sequential restatement: is record r bad?
std::vector<char> restate_bad(const std::vector<uint64_t>& t, uint64_t nunits) {
  const size_t n = t.size() / 4;
  std::vector<char> bad(n, 0);
  for (size_t r = 0; r < n; ++r) {
    const uint64_t first = t[4 * r], bytes = t[4 * r + 3];
    if (bytes == 0) bad[r] = 1;
    const uint64_t want = r ? t[4 * (r - 1)] + units_of(t[4 * (r - 1) + 3]) : 0;
    if (first != want) bad[r] = 1;
    if (r + 1 == n && first + units_of(bytes) != nunits) bad[r] = 1;
  }
  return bad;
}

void copy_case(uint64_t c, std::mt19937_64& rng, bool damage) {
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const size_t nrec = (size_t)pick(1, 10);
  std::vector<Rec> recs(nrec);
  std::vector<uint64_t> table;
  uint64_t nunits = 0;
  for (size_t r = 0; r < nrec; ++r) {
    Rec& x = recs[r];
    const uint64_t kinds[] = {1, 15, 16, 17, 4101, pick(1, 4101), pick(1, 64), 16 * pick(1, 40)};
    x.data.resize((size_t)kinds[rng() % 8]);
    for (uint8_t& b : x.data) b = (uint8_t)rng();
    // (the pairs are walked, not drawn: 256 records see all of them)
    const uint64_t p = (c * 11 + r) % 256;
    x.sa = (size_t)(p / 16);
    x.da = (size_t)(p % 16);
    x.src.reset(new uint8_t[x.sa + x.data.size()]);
    memset(x.src.get(), kPoison, x.sa);
    memcpy(x.s(), x.data.data(), x.data.size());
    x.dst.reset(new uint8_t[x.dst_size()]);
    memset(x.dst.get(), kPoison, x.dst_size());
    if ((uintptr_t)x.src.get() % 16 || (uintptr_t)x.dst.get() % 16) die("buffer not 16-byte aligned", c);
    if ((uintptr_t)x.s() % 16 != x.sa || (uintptr_t)x.d() % 16 != x.da) die("alignment", c);
    tot.pair[x.sa][x.da] = true;
    const uint64_t rec[4] = {nunits, (uint64_t)(uintptr_t)x.s(), (uint64_t)(uintptr_t)x.d(),
                             (uint64_t)x.data.size()};
    table.insert(table.end(), rec, rec + 4);
    nunits += units_of(x.data.size());
  }
  std::vector<uint64_t> t = table;
  uint64_t nu = nunits;
  if (damage) {
    ++tot.damaged;
    const uint64_t v = rng() % nrec;
    switch (rng() % 4) {
      case 0: t[4 * v + 3] = 0; break;  // zero bytes
      // a wrong unit_first (still ascending: at most the next record's)
      case 1: t[4 * v] += 1 + rng() % units_of(t[4 * v + 3]); break;
      case 2: t[4 * v] -= v ? 1 : 0; if (!v) t[0] = 1; break;  // ... or one that steps back
      default: nu += rng() % 2 ? 1 : (uint64_t)-1; break;      // a wrong unit total
    }
  }
  const std::vector<char> bad = restate_bad(t, nu);
  uint64_t nbad = 0;
  for (char x : bad) nbad += x;
  if (damage && !nbad) die("the damage made no record bad", c);
  if (!damage && nbad) die("the restatement calls a sound table bad", c);
  std::unique_ptr<uint64_t[]> tt(new uint64_t[t.size()]);  // (exactly the table: no slack)
  memcpy(tt.get(), t.data(), 8 * t.size());
  const uint64_t got = copyblk::apply_host(tt.get(), nrec, nu);
  if (got != nbad) die("the bad count is not the restatement's", c);
  tot.bad += nbad;
  tot.records += nrec;
  tot.units += nu;
  for (size_t r = 0; r < nrec; ++r) {
    const Rec& x = recs[r];
    // a sound record of a damaged table is written whole only where the
    // bisection still finds it: the unit_first values the damage leaves ascend
    // except for case 2, whose step back may hide the record in front
    std::vector<uint8_t> want(x.dst_size(), kPoison);
    if (!bad[r])
      for (size_t i = 0; i < x.data.size(); ++i) want[x.da + kRedzone + i] = x.data[i];
    if (damage && !bad[r]) {
      // outside the record nothing, inside it the bytes or the poison
      for (size_t i = 0; i < x.dst_size(); ++i) {
        const bool inside = i >= x.da + kRedzone && i < x.da + kRedzone + x.data.size();
        if (x.dst[i] != want[i] && !(inside && x.dst[i] == kPoison))
          die("a sound record of a damaged table holds other bytes", c);
      }
    } else if (memcmp(x.dst.get(), want.data(), want.size())) {
      die(bad[r] ? "a bad record was written" : "a destination is not the restatement's", c);
    }
    if (memcmp(x.s(), x.data.data(), x.data.size())) die("a source was written", c);
    for (size_t i = 0; i < x.sa; ++i)
      if (x.src[i] != kPoison) die("a byte in front of a source was written", c);
    if (!bad[r]) tot.bytes += x.data.size();
  }
}

void plan_case(uint64_t c, std::mt19937_64& rng) {
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const uint64_t bs_choices[] = {1, 7, 16, 100, 512, 1000};
  const uint64_t bs = bs_choices[rng() % 6];
  auto nblk_of = [&](uint64_t size) { return (size + bs - 1) / bs; };
  // the new image's files: some empty (no run), some without a destination
  const size_t nfiles = (size_t)pick(1, 9);
  std::vector<uint64_t> sizes(nfiles), dests(nfiles), runs;
  uint64_t n_need = 0;
  for (size_t i = 0; i < nfiles; ++i) {
    const uint64_t kinds[] = {0, 1, bs, bs + 1, 3 * bs + 5, pick(1, 70 * bs), 64 * bs, 65 * bs};
    sizes[i] = kinds[rng() % 8];
    dests[i] = rng() % 5 ? 0x100000 * (i + 1) + rng() % 16 : 0;
    if (!sizes[i]) continue;
    const uint64_t run[4] = {n_need, sizes[i], (uint64_t)i, rng()};
    runs.insert(runs.end(), run, run + 4);
    n_need += nblk_of(sizes[i]);
  }
  const size_t nhave = (size_t)pick(0, 6);
  std::vector<uint64_t> have;
  uint64_t n_pool = 0;
  for (size_t k = 0; k < nhave; ++k) {
    const uint64_t size = rng() % 3 ? pick(1, 40 * bs) : bs * pick(1, 8) + (rng() % 2 ? 0 : pick(1, bs));
    const uint64_t rec[3] = {n_pool, 0x80000000ull + 0x1000000 * k + rng() % 16, size};
    have.insert(have.end(), rec, rec + 3);
    n_pool += nblk_of(size);
  }
  std::vector<uint32_t> match((size_t)n_need + 1);
  for (uint32_t& m : match) {
    const uint64_t kind = rng() % 8;
    m = kind == 0 || !n_pool ? copyblk::kNoMatch
                              : kind == 1 ? (uint32_t)(n_pool + rng() % 3) : (uint32_t)(rng() % n_pool);
  }
  // (exactly sized copies: a read past a table is an ASan report)
  auto dup64 = [](const std::vector<uint64_t>& v) {
    std::unique_ptr<uint64_t[]> q(new uint64_t[v.size() ? v.size() : 1]);
    if (!v.empty()) memcpy(q.get(), v.data(), 8 * v.size());
    return q;
  };
  std::unique_ptr<uint32_t[]> m_(new uint32_t[n_need ? n_need : 1]);
  memcpy(m_.get(), match.data(), 4 * n_need);
  const std::unique_ptr<uint64_t[]> runs_ = dup64(runs), have_ = dup64(have), dests_ = dup64(dests);
  const copyblk::Plan p{m_.get(), n_need, runs_.get(), runs.size() / 4, dests_.get(), nfiles,
                        have_.get(), nhave, n_pool, bs};
  const uint64_t nwords = (n_need + 63) / 64;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[nwords ? nwords : 1]);
  std::unique_ptr<uint64_t[]> out(new uint64_t[4 * (n_need ? n_need : 1)]);
  uint64_t res[copyblk::kPlanResFields];
  for (uint64_t w = 0; w < nwords; ++w) bits[w] = ~0ull;  // (every word must be written)
  copyblk::plan_host(p, bits.get(), out.get(), res);
  // the restatement: block by block, files and buffers found by walking them
  uint64_t g = 0, nrec = 0, nunits = 0, bytes = 0, dropped = 0;
  for (size_t i = 0; i < nfiles; ++i)
    for (uint64_t j = 0; j < nblk_of(sizes[i]); ++j, ++g) {
      const uint64_t need_len = std::min(bs, sizes[i] - j * bs);
      const uint32_t m = match[g];
      bool taken = false;
      uint64_t src = 0;
      if (m != copyblk::kNoMatch && m < n_pool && dests[i]) {
        uint64_t at = 0;
        for (size_t k = 0; k < nhave; ++k) {
          const uint64_t nb = nblk_of(have[3 * k + 2]);
          if (m < at + nb) {
            const uint64_t pj = m - at, have_len = std::min(bs, have[3 * k + 2] - pj * bs);
            if (have_len == need_len) {
              taken = true;
              src = have[3 * k + 1] + pj * bs;
            } else {
              ++dropped;
            }
            break;
          }
          at += nb;
        }
      }
      if (((bits[g >> 6] >> (g & 63)) & 1) != (taken ? 1u : 0u)) die("a plan bit differs", c);
      if (!taken) continue;
      const uint64_t* q = out.get() + 4 * nrec;
      if (q[0] != nunits || q[1] != src || q[2] != dests[i] + j * bs || q[3] != need_len)
        die("a plan record differs", c);
      ++nrec;
      nunits += units_of(need_len);
      bytes += need_len;
    }
  for (uint64_t b = n_need; b < 64 * nwords; ++b)
    if ((bits[b >> 6] >> (b & 63)) & 1) die("a bit past the last block is set", c);
  if (res[0] != nrec || res[1] != nunits || res[2] != bytes || res[3] != dropped)
    die("the plan's counts differ", c);
  if (copyblk::take_of(p, n_need).flags || copyblk::take_of(p, ~0ull).flags)
    die("a block past the image is taken", c);
  tot.blocks += n_need;
  tot.taken += nrec;
  tot.dropped += dropped;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 3000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (uint64_t c = 0; c < cases; ++c) {
    std::mt19937_64 rng(seed * 1000003 + c);
    copy_case(c, rng, false);
    copy_case(c, rng, true);
    plan_case(c, rng);
  }
  if (cases >= 256)
    for (int a = 0; a < 16; ++a)
      for (int b = 0; b < 16; ++b)
        if (!tot.pair[a][b]) die("an alignment pair never occurred", (uint64_t)(16 * a + b));
  fprintf(stderr,
          "copyblk_fuzz: %llu records, %llu units, %llu bytes; %llu damaged tables, %llu bad "
          "records; %llu plan blocks, %llu taken, %llu dropped\n",
          (unsigned long long)tot.records, (unsigned long long)tot.units,
          (unsigned long long)tot.bytes, (unsigned long long)tot.damaged,
          (unsigned long long)tot.bad, (unsigned long long)tot.blocks,
          (unsigned long long)tot.taken, (unsigned long long)tot.dropped);
  printf("copyblk_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
