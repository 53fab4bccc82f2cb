// The gather rule (ciruela_amd/csrc/gather.hpp) under ASan + UBSan: a
// stand-alone host program, no device code.
//
//   gather_fuzz [cases] [seed]
//
// Per case seeded random files and a random block size go through the packing
// cir_store_blocks uses (pack.hpp: pack_run into batches of a random fill);
// each run becomes a gather record (gather::record_of) and gather::apply_host
// fills the batch's slot from the files' sources:
//   * every source has an alignment of its own (0 .. 15) and sits in a heap
//     buffer of exactly redzone + size + redzone bytes, so a read past a source
//     is an ASan report; the sources are compared with the files afterwards (the
//     gather writes none of them);
//   * the slot is a heap buffer of exactly the batch's bytes rounded up to 16
//     between two poisoned redzones of its own; it is compared with a
//     byte-by-byte restatement -- the runs' bytes, zeros up to each run's next
//     multiple of 16, the poison elsewhere --, so a store outside a record's
//     rounded range shows;
//   * then one batch's table is damaged -- a misaligned dst_pos, a range past
//     the slot, a zero bytes, a length whose rounding wraps, a wrong
//     unit_first, a wrong nunits -- and the expected bad set is restated by a
//     plain sequential walk: exactly those records must be counted, nothing of
//     them written (their ranges keep the poison) and every other record
//     written whole.
// Exit status 0 and "gather_fuzz: N cases ok" on stdout; the totals go to
// stderr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "gather.hpp"
#include "pack.hpp"

using namespace cir;

namespace {

constexpr size_t kRedzone = 48;
constexpr uint8_t kPoison = 0xA5;

struct Totals {
  uint64_t files = 0, batches = 0, records = 0, units = 0, bytes = 0, damaged = 0, bad = 0;
} tot;

[[noreturn]] void die(const char* what, uint64_t c) {
  fprintf(stderr, "gather_fuzz: case %llu: %s\n", (unsigned long long)c, what);
  exit(1);
}

struct File {
  std::vector<uint8_t> data;
  std::unique_ptr<uint8_t[]> buf;  // skew, the source, nothing behind it
  size_t skew = 0;
  const uint8_t* src() const { return buf.get() + skew; }
  uint64_t nblk(uint64_t bs) const { return (data.size() + bs - 1) / bs; }
};

uint64_t units_of(uint64_t bytes) { return bytes / 16 + (bytes % 16 != 0); }

// the sequential restatement: is record r bad?  (128-bit sums: no wrap)
std::vector<char> restate_bad(const std::vector<uint64_t>& t, uint64_t nunits, uint64_t dst_bytes) {
  const size_t n = t.size() / 4;
  std::vector<char> bad(n, 0);
  for (size_t r = 0; r < n; ++r) {
    const uint64_t first = t[4 * r], pos = t[4 * r + 1], bytes = t[4 * r + 3];
    if (pos % 16 || bytes == 0) bad[r] = 1;
    const unsigned __int128 end = (unsigned __int128)pos + (unsigned __int128)16 * units_of(bytes);
    if (end > dst_bytes) bad[r] = 1;
    const uint64_t want = r ? t[4 * (r - 1)] + units_of(t[4 * (r - 1) + 3]) : 0;
    if (first != want) bad[r] = 1;
    if (r + 1 == n && first + units_of(bytes) != nunits) bad[r] = 1;
  }
  return bad;
}

void one_case(uint64_t c, std::mt19937_64& rng) {
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const uint64_t bs_choices[] = {1, 7, 16, 17, 100, 512, 1000, 4096};
  const uint64_t bs = bs_choices[rng() % 8];
  const size_t nfiles = (size_t)pick(1, 12);
  std::vector<File> files(nfiles);
  uint64_t seg = 0;
  for (File& f : files) {
    const uint64_t kinds[] = {1, bs - 1 ? bs - 1 : 1, bs, bs + 1, 3 * bs, pick(1, 9 * bs), pick(1, 40)};
    f.data.resize((size_t)kinds[rng() % 7]);
    for (uint8_t& b : f.data) b = (uint8_t)rng();
    f.skew = (size_t)(rng() % 16);
    // exactly skew + size bytes: ASan's own redzones lie in front and behind,
    // and the skew bytes in front are poison no record names
    f.buf.reset(new uint8_t[f.skew + f.data.size()]);
    memset(f.buf.get(), kPoison, f.skew);
    memcpy(f.buf.get() + f.skew, f.data.data(), f.data.size());
    if ((uintptr_t)f.buf.get() % 16) die("buffer not 16-byte aligned", c);
    seg = std::max<uint64_t>(seg, std::min<uint64_t>(f.data.size(), bs));
    ++tot.files;
  }
  SlotSizes sz = slot_sizes(pick(64, 6000), seg, rng() % 2);
  sz.cap_blk = pick(1, 40);  // (small: batches end on the block count too)
  std::vector<uint64_t> h_off(sz.cap_blk);
  std::vector<uint32_t> h_len(sz.cap_blk);
  const uint64_t damage_batch = rng() % 3 ? ~0ull : rng() % 4;

  size_t fi = 0;
  uint64_t fblk = 0, batch_no = 0;
  while (fi < nfiles) {
    Batch b;
    std::vector<uint64_t> table;
    std::vector<size_t> rec_file;
    std::vector<uint64_t> rec_fblk;
    uint64_t nunits = 0;
    while (fi < nfiles && b.n < sz.cap_blk) {
      File& f = files[fi];
      const Run r = pack_run(b, sz.fill, sz.cap_blk, bs, f.data.size(), fblk, f.nblk(bs) - fblk,
                             h_off.data(), h_len.data());
      if (!r.take) break;
      uint64_t rec[4];
      nunits = gather::record_of(r, (uint64_t)(uintptr_t)f.src(), fblk, bs, nunits, rec);
      table.insert(table.end(), rec, rec + 4);
      rec_file.push_back(fi);
      rec_fblk.push_back(fblk);
      fblk += r.take;
      if (fblk == f.nblk(bs)) {
        ++fi;
        fblk = 0;
      }
    }
    sz.offered();
    if (!b.n) {
      if (sz.fill == sz.cap) die("a whole slot took nothing", c);
      continue;
    }
    // the slot's device twin as the gather is told it: the used bytes rounded up
    const uint64_t dst_bytes = align16(b.used);
    if (dst_bytes > sz.cap) die("the rounded batch does not fit the slot", c);
    std::unique_ptr<uint8_t[]> raw(new uint8_t[kRedzone + dst_bytes + kRedzone]);
    memset(raw.get(), kPoison, kRedzone + dst_bytes + kRedzone);
    uint8_t* slot = raw.get() + kRedzone;
    const uint64_t nruns = table.size() / 4;
    ++tot.batches;
    tot.records += nruns;
    tot.units += nunits;

    std::vector<uint64_t> t = table;
    uint64_t nu = nunits;
    const bool damaged = batch_no++ == damage_batch;
    if (damaged) {
      ++tot.damaged;
      const uint64_t v = rng() % nruns;
      switch (rng() % 7) {
        case 0: t[4 * v + 1] += 1 + rng() % 15; break;                  // a misaligned dst_pos
        case 1: t[4 * v + 1] = dst_bytes + 16 * (rng() % 3); break;     // the range starts at or past the end
        case 2: t[4 * v + 3] = dst_bytes - t[4 * v + 1] + 1; break;     // ... or ends past it
        case 3: t[4 * v + 3] = 0; break;                                // zero bytes
        case 4: t[4 * v + 3] = ~0ull - rng() % 15; break;               // the rounding wraps
        // a wrong unit_first (still ascending: at most the next record's)
        case 5: t[4 * v] += 1 + rng() % scatter::units(t[4 * v + 3]); break;
        default: nu += rng() % 2 ? 1 : (uint64_t)-1; break;             // a wrong unit total
      }
    }
    const std::vector<char> bad = restate_bad(t, nu, dst_bytes);
    uint64_t nbad = 0;
    for (char x : bad) nbad += x;
    if (damaged && !nbad) die("the damage made no record bad", c);
    if (!damaged && nbad) die("the restatement calls a sound table bad", c);
    std::unique_ptr<uint64_t[]> tt(new uint64_t[t.size()]);  // (exactly the table: no slack)
    memcpy(tt.get(), t.data(), 8 * t.size());
    const uint64_t got = gather::apply_host(slot, dst_bytes, tt.get(), nruns, nu);
    if (got != nbad) die("the bad count is not the restatement's", c);
    tot.bad += nbad;
    // the restatement, byte by byte, from the sound table's places and lengths
    std::vector<uint8_t> want(kRedzone + dst_bytes + kRedzone, kPoison);
    for (uint64_t r = 0; r < nruns; ++r) {
      if (bad[r]) continue;
      const File& f = files[rec_file[r]];
      const uint64_t pos = table[4 * r + 1], n = table[4 * r + 3];
      for (uint64_t i = 0; i < 16 * units_of(n); ++i)
        want[kRedzone + pos + i] = i < n ? f.data[rec_fblk[r] * bs + i] : 0;
      tot.bytes += n;
    }
    if (memcmp(raw.get(), want.data(), want.size())) die("the slot is not the restatement's", c);
    // what the packer's descriptors say of the slot is what the files hold
    if (!damaged)
      for (uint64_t k = 0; k < b.n; ++k)
        if (h_off[k] + h_len[k] > dst_bytes) die("a descriptor reaches past the slot", c);
  }
  for (const File& f : files) {
    if (memcmp(f.src(), f.data.data(), f.data.size())) die("a source was written", c);
    for (size_t i = 0; i < f.skew; ++i)
      if (f.buf[i] != kPoison) die("a byte in front of a source was written", c);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 3000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (uint64_t c = 0; c < cases; ++c) {
    std::mt19937_64 rng(seed * 1000003 + c);
    one_case(c, rng);
  }
  fprintf(stderr,
          "gather_fuzz: %llu files, %llu batches, %llu records, %llu units, %llu bytes; %llu "
          "damaged tables, %llu bad records\n",
          (unsigned long long)tot.files, (unsigned long long)tot.batches,
          (unsigned long long)tot.records, (unsigned long long)tot.units,
          (unsigned long long)tot.bytes, (unsigned long long)tot.damaged,
          (unsigned long long)tot.bad);
  printf("gather_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
