// The scatter rule (ciruela_amd/csrc/scatter.hpp) under ASan + UBSan: a
// stand-alone host program, no device code.
//
//   scatter_fuzz [cases] [seed]
//
// Per case seeded random files and a random block size go through the packing
// cir_load_blocks uses (pack.hpp: pack_run into batches of a random fill,
// cut_pieces for the reads that fill the slot); each run becomes a scatter
// record (scatter::record_of) and scatter::apply_host moves the batch into the
// files' destinations:
//   * every destination has an alignment of its own (0 .. 15) and sits in a heap
//     buffer of exactly redzone + size + redzone bytes, the redzones and the
//     destination poisoned; after the last batch the destination is compared
//     byte by byte with the file and the redzones with the poison, so a byte
//     stored outside a run shows, and ASan reports one outside the buffer;
//   * the slot is a heap buffer of exactly the bytes the batch uses, so a read
//     past what was uploaded is a report;
//   * then one batch's table is damaged -- a misaligned src_pos, a source range
//     past the slot, a zero bytes, a wrong unit_first, a wrong nunits -- and the
//     expected bad set is restated by a plain sequential walk: exactly those
//     records must be counted, nothing of them written (their destinations keep
//     the poison) and every other record written whole.
// Exit status 0 and "scatter_fuzz: N cases ok" on stdout; the totals go to
// stderr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "pack.hpp"
#include "scatter.hpp"

using namespace cir;

namespace {

constexpr size_t kRedzone = 48;
constexpr uint8_t kPoison = 0xA5;

struct Totals {
  uint64_t files = 0, batches = 0, records = 0, units = 0, bytes = 0, damaged = 0, bad = 0;
} tot;

[[noreturn]] void die(const char* what, uint64_t c) {
  fprintf(stderr, "scatter_fuzz: case %llu: %s\n", (unsigned long long)c, what);
  exit(1);
}

struct File {
  std::vector<uint8_t> data;
  std::unique_ptr<uint8_t[]> buf;  // redzone, skew, the destination, redzone
  size_t skew = 0;
  uint8_t* dst() const { return buf.get() + kRedzone + skew; }
  size_t buf_len() const { return kRedzone + skew + data.size() + kRedzone; }
  uint64_t nblk(uint64_t bs) const { return (data.size() + bs - 1) / bs; }
};

struct Job {  // cut_pieces' job
  uint64_t file_off, len;
  uint8_t* dst;
  size_t file;
};

// the sequential restatement: is record r bad?
std::vector<char> restate_bad(const std::vector<uint64_t>& t, uint64_t nunits, uint64_t src_bytes) {
  const size_t n = t.size() / 4;
  std::vector<char> bad(n, 0);
  for (size_t r = 0; r < n; ++r) {
    const uint64_t first = t[4 * r], pos = t[4 * r + 1], bytes = t[4 * r + 3];
    if (pos % 16 || bytes == 0) bad[r] = 1;
    if (bytes > src_bytes || pos > src_bytes - bytes) bad[r] = 1;
    const uint64_t want = r ? t[4 * (r - 1)] + (t[4 * (r - 1) + 3] + 15) / 16 : 0;
    if (first != want) bad[r] = 1;
    if (r + 1 == n && first + (bytes + 15) / 16 != nunits) bad[r] = 1;
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
    f.buf.reset(new uint8_t[f.buf_len()]);
    memset(f.buf.get(), kPoison, f.buf_len());
    // (new[] is 16-byte aligned: skew is the destination's alignment)
    if (((uintptr_t)f.buf.get() + kRedzone) % 16) die("buffer not 16-byte aligned", c);
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
    std::vector<uint8_t> stage((size_t)sz.cap);  // the pinned slot
    std::vector<Job> jobs;
    std::vector<uint64_t> table;
    std::vector<size_t> rec_file;
    std::vector<uint64_t> rec_fblk;
    uint64_t nunits = 0;
    while (fi < nfiles && b.n < sz.cap_blk) {
      File& f = files[fi];
      const Run r = pack_run(b, sz.fill, sz.cap_blk, bs, f.data.size(), fblk, f.nblk(bs) - fblk,
                             h_off.data(), h_len.data());
      if (!r.take) break;
      cut_pieces(jobs, Job{fblk * bs, r.bytes, stage.data() + r.pos, fi});
      uint64_t rec[4];
      nunits = scatter::record_of(r, (uint64_t)(uintptr_t)f.dst(), fblk, bs, nunits, rec);
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
    for (const Job& j : jobs) memcpy(j.dst, files[j.file].data.data() + j.file_off, j.len);
    // the device twin: exactly the bytes uploaded
    const uint64_t used = b.used;
    std::unique_ptr<uint8_t[]> slot(new uint8_t[used]);
    memcpy(slot.get(), stage.data(), used);
    const uint64_t nruns = table.size() / 4;
    ++tot.batches;
    tot.records += nruns;
    tot.units += nunits;

    if (batch_no++ != damage_batch) {
      std::unique_ptr<uint64_t[]> t(new uint64_t[table.size()]);
      memcpy(t.get(), table.data(), 8 * table.size());
      if (scatter::apply_host(slot.get(), used, t.get(), nruns, nunits))
        die("a sound table has a bad record", c);
      for (uint64_t r = 0; r < nruns; ++r) tot.bytes += table[4 * r + 3];
      continue;
    }
    // one damaged table: its runs' destinations still hold the poison
    ++tot.damaged;
    std::vector<uint64_t> t = table;
    uint64_t nu = nunits;
    const uint64_t v = rng() % nruns;
    switch (rng() % 6) {
      case 0: t[4 * v + 1] += 1 + rng() % 15; break;              // a misaligned src_pos
      case 1: t[4 * v + 1] = (used + 16) & ~15ull; break;         // the source starts past the slot
      case 2: t[4 * v + 3] = used - t[4 * v + 1] + 1; break;      // ... or ends one byte past it
      case 3: t[4 * v + 3] = 0; break;                            // zero bytes
      // a wrong unit_first (still ascending: at most the next record's)
      case 4: t[4 * v] += 1 + rng() % scatter::units(t[4 * v + 3]); break;
      default: nu += rng() % 2 ? 1 : (uint64_t)-1; break;          // a wrong unit total
    }
    const std::vector<char> bad = restate_bad(t, nu, used);
    uint64_t nbad = 0;
    for (char x : bad) nbad += x;
    if (!nbad) die("the damage made no record bad", c);
    std::unique_ptr<uint64_t[]> tt(new uint64_t[t.size()]);
    memcpy(tt.get(), t.data(), 8 * t.size());
    const uint64_t got = scatter::apply_host(slot.get(), used, tt.get(), nruns, nu);
    if (got != nbad) die("the bad count is not the restatement's", c);
    tot.bad += nbad;
    for (uint64_t r = 0; r < nruns; ++r) {
      // judged by the sound table's place and length: a bad record wrote nothing there
      const File& f = files[rec_file[r]];
      const uint8_t* d = f.dst() + rec_fblk[r] * bs;
      const uint64_t n = table[4 * r + 3];
      if (bad[r]) {
        for (uint64_t i = 0; i < n; ++i)
          if (d[i] != kPoison) die("a bad record was written", c);
        // leave the file whole for the final compare
        memcpy(const_cast<uint8_t*>(d), f.data.data() + rec_fblk[r] * bs, n);
      } else if (memcmp(d, f.data.data() + rec_fblk[r] * bs, n)) {
        die("a sound record beside a bad one was not written whole", c);
      }
    }
  }
  for (const File& f : files) {
    if (memcmp(f.dst(), f.data.data(), f.data.size())) die("a destination is not its file", c);
    const uint8_t* p = f.buf.get();
    for (size_t i = 0; i < kRedzone + f.skew; ++i)
      if (p[i] != kPoison) die("a byte in front of a destination was written", c);
    for (size_t i = kRedzone + f.skew + f.data.size(); i < f.buf_len(); ++i)
      if (p[i] != kPoison) die("a byte behind a destination was written", c);
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
          "scatter_fuzz: %llu files, %llu batches, %llu records, %llu units, %llu bytes; %llu "
          "damaged tables, %llu bad records\n",
          (unsigned long long)tot.files, (unsigned long long)tot.batches,
          (unsigned long long)tot.records, (unsigned long long)tot.units,
          (unsigned long long)tot.bytes, (unsigned long long)tot.damaged,
          (unsigned long long)tot.bad);
  printf("scatter_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
