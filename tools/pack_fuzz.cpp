// Seeded fuzz of ciruela_amd/csrc/pack.hpp (the slot layout of the scan and of
// cir_check_index / cir_check_links / cir_check_blocks) against a restatement
// of the packing rule that goes one block at a time.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/pack_fuzz.cpp -o build/pack_fuzz
// and run it; tests/test_pack_cpu.py does.  The descriptor arrays are heap
// buffers of exactly cap_blk entries, so a descriptor written past a slot's
// block count is an AddressSanitizer report.
//
// The rule, restated here per block.  A range's events are, in unit order,
// every block of a unit that lies in [b0, b1) and every zero-block unit whose
// place f has b0 <= f < b1, or f == b1 when b1 is the end of all blocks.  A
// batch takes events while it holds fewer than cap_blk blocks.  A block goes
// on with the run before it when that is the block before it of the same file
// and the run, every block counted at a full bs, still ends at or below
// `fill`; else it starts a run at the next multiple of 16, if its own length
// fits below `fill` there, and ends the batch if not.  A batch never goes
// past its range; `fill` doubles up to `cap` after every batch.
//
// usage: pack_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "pack.hpp"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      fprintf(stderr, "case %llu, line %d: %s\n", (unsigned long long)case_no, __LINE__, #cond); \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static uint64_t case_no;

struct File {
  uint64_t size, nblk, first_blk;
};
struct Block {
  uint64_t global, off, len;
  bool operator==(const Block& o) const {
    return global == o.global && off == o.off && len == o.len;
  }
};
struct OutBatch {
  size_t range = 0;
  uint64_t fill = 0, used = 0;
  std::vector<Block> blocks;
  std::vector<size_t> zeros;  // the zero-block units passed
};
struct Job {  // (dst as a number: the cut is checked, nothing is read)
  uint64_t file_off, len, dst;
  int tag;
};
struct Event {
  size_t unit;
  uint64_t k;  // its block (zero-block units: none)
};

// the pieces tile [off0, off0 + bytes) of the file and [dst, dst + bytes)
static bool tiles(const std::vector<Job>& jobs, size_t from, uint64_t off0, uint64_t bytes,
                  uint64_t dst, int tag) {
  uint64_t done = 0;
  for (size_t i = from; i < jobs.size(); ++i) {
    const Job& j = jobs[i];
    if (j.file_off != off0 + done || j.dst != dst + done || j.len == 0 ||
        j.len > cir::kReadPiece || j.tag != tag)
      return false;
    // (every piece but the last is a whole one)
    if (i + 1 < jobs.size() && j.len != cir::kReadPiece) return false;
    done += j.len;
  }
  return done == bytes;
}

static int one() {
  static const uint64_t kBs[] = {1, 2, 15, 16, 17, 48, 100, 512, 1000, 4095, 4096};
  const uint64_t bs = rnd() % 3 == 0 ? kBs[rnd() % 11] : rnd() % 4096 + 1;
  std::vector<File> files(rnd() % 12 + 1);
  uint64_t total = 0, seg = 0;
  for (size_t i = 0; i < files.size(); ++i) {
    File& f = files[i];
    // (some empty; never all of them: the callers do not come here then)
    const bool empty = rnd() % 4 == 0 && !(i + 1 == files.size() && total == 0);
    f.nblk = empty ? 0 : rnd() % 8 == 0 ? rnd() % 40 + 1 : rnd() % 6 + 1;
    f.size = empty ? 0 : (f.nblk - 1) * bs + (rnd() % 4 == 0 ? bs : rnd() % bs + 1);
    f.first_blk = total;
    total += f.nblk;
    seg = std::max(seg, std::min(f.size, bs));
  }
  uint64_t staging;
  switch (rnd() % 4) {
    case 0: staging = rnd() % bs; break;               // below a block
    case 1: staging = bs; break;                       // one block
    case 2: staging = bs + rnd() % (3 * bs) + 1; break;  // a few
    default: staging = bs * (rnd() % 30 + 1) + rnd() % bs;
  }
  cir::SlotSizes sz = cir::slot_sizes(staging, seg, rnd() & 1);
  CHECK(sz.cap % 16 == 0 && sz.cap >= seg + 16 && sz.cap >= staging && sz.cap < staging + 16 + seg + 16);
  CHECK(sz.fill >= seg + 16 && sz.fill <= sz.cap);
  if (rnd() % 3 == 0) sz.cap_blk = rnd() % 6 + 1;  // so that it binds
  // one to five ranges that start and end anywhere; often from the first
  // block and to the last one
  size_t nr = rnd() % 5 + 1;
  while (2 * nr > total + 1) --nr;
  std::vector<uint64_t> cuts;
  if (rnd() & 1) cuts.push_back(0);
  if (rnd() & 1) cuts.push_back(total);
  while (cuts.size() < 2 * nr) {
    const uint64_t c = rnd() % (total + 1);
    if (std::find(cuts.begin(), cuts.end(), c) == cuts.end()) cuts.push_back(c);
  }
  std::sort(cuts.begin(), cuts.end());
  cir::BlockRanges ranges;
  for (size_t r = 0; r < nr; ++r) ranges.push_back({cuts[2 * r], cuts[2 * r + 1]});

  // ---- the header: cursor and packing step, driven as the callers drive them
  std::vector<OutBatch> got;
  {
    cir::SlotSizes z = sz;
    std::unique_ptr<uint64_t[]> h_off(new uint64_t[z.cap_blk]);
    std::unique_ptr<uint32_t[]> h_len(new uint32_t[z.cap_blk]);
    cir::RangeCursor cur(
        files.size(),
        [&](size_t i) { return std::make_pair(files[i].first_blk, files[i].nblk); }, ranges,
        total);
    while (cur.more()) {
      OutBatch o;
      o.range = cur.range();
      o.fill = z.fill;
      cir::Batch b;
      std::vector<Job> jobs;
      while (cur.here() && b.n < z.cap_blk) {
        const File& f = files[cur.ui];
        if (f.nblk == 0) {
          o.zeros.push_back(cur.ui);
          cur.advance(0);
          continue;
        }
        const uint64_t fblk = cur.fblk, at = cur.at(), left = cur.left();
        CHECK(left >= 1 && at >= ranges[o.range].first && at + left <= ranges[o.range].second);
        const cir::Batch before = b;
        const cir::Run r =
            cir::pack_run(b, z.fill, z.cap_blk, bs, f.size, fblk, left, h_off.get(), h_len.get());
        if (!r.take) {
          CHECK(b.n == before.n && b.used == before.used);
          break;
        }
        CHECK(r.take <= left && r.at == before.n && b.n == r.at + r.take);
        CHECK(r.pos % 16 == 0 && r.pos >= before.pos && r.pos < before.pos + 16);
        CHECK(b.used == r.pos + r.bytes && b.pos == b.used && b.used <= z.fill);
        uint64_t bytes = 0;
        for (uint64_t j = 0; j < r.take; ++j) {
          CHECK(h_off[r.at + j] == r.pos + j * bs);
          CHECK(h_len[r.at + j] == std::min(bs, f.size - (fblk + j) * bs));
          bytes += h_len[r.at + j];
          o.blocks.push_back({at + j, h_off[r.at + j], h_len[r.at + j]});
        }
        CHECK(bytes == r.bytes);
        const size_t from = jobs.size();
        cir::cut_pieces(jobs, Job{fblk * bs, r.bytes, r.pos, (int)cur.ui});
        CHECK(tiles(jobs, from, fblk * bs, r.bytes, r.pos, (int)cur.ui));
        cur.advance(r.take);
      }
      CHECK(b.n <= z.cap_blk && b.used <= z.fill && z.fill <= z.cap);
      CHECK(b.n == o.blocks.size());
      o.used = b.used;
      got.push_back(o);
      z.offered();
    }
  }

  // ---- the restatement
  std::vector<OutBatch> want;
  {
    uint64_t fill = sz.fill;
    for (size_t ri = 0; ri < ranges.size(); ++ri) {
      const uint64_t b0 = ranges[ri].first, b1 = ranges[ri].second;
      std::vector<Event> ev;
      for (size_t u = 0; u < files.size(); ++u) {
        const File& f = files[u];
        if (f.nblk == 0) {
          if ((b0 <= f.first_blk && f.first_blk < b1) || (f.first_blk == b1 && b1 == total))
            ev.push_back({u, 0});
        } else {
          for (uint64_t k = 0; k < f.nblk; ++k)
            if (f.first_blk + k >= b0 && f.first_blk + k < b1) ev.push_back({u, k});
        }
      }
      size_t i = 0;
      while (i < ev.size()) {
        OutBatch o;
        o.range = ri;
        o.fill = fill;
        uint64_t pos = 0;
        bool in_run = false;  // the event before this one was a block of this batch
        uint64_t run_pos = 0, run_cnt = 0;
        while (i < ev.size() && o.blocks.size() < sz.cap_blk) {
          const File& f = files[ev[i].unit];
          if (f.nblk == 0) {
            o.zeros.push_back(ev[i].unit);
            in_run = false;
            ++i;
            continue;
          }
          const uint64_t k = ev[i].k, len = std::min(bs, f.size - k * bs);
          const bool same_file = in_run && ev[i - 1].unit == ev[i].unit;
          if (same_file && run_pos + (run_cnt + 1) * bs <= fill) {
            o.blocks.push_back({f.first_blk + k, run_pos + run_cnt * bs, len});
            ++run_cnt;
          } else {
            const uint64_t p = (pos + 15) / 16 * 16;
            if (p + len > fill) break;
            o.blocks.push_back({f.first_blk + k, p, len});
            run_pos = p;
            run_cnt = 1;
          }
          pos = o.blocks.back().off + len;
          o.used = pos;
          in_run = true;
          ++i;
        }
        want.push_back(o);
        fill = std::min(sz.cap, fill * 2);
      }
    }
  }

  CHECK(got.size() == want.size());
  for (size_t i = 0; i < got.size(); ++i) {
    CHECK(got[i].range == want[i].range);
    CHECK(got[i].fill == want[i].fill);
    CHECK(got[i].blocks == want[i].blocks);
    CHECK(got[i].zeros == want[i].zeros);
    CHECK(got[i].used == want[i].used);
  }
  // every block of every range exactly once, in order; every zero-block unit
  // at most once (by construction of the restatement: once in the range that
  // owns it)
  size_t bi = 0;
  std::vector<Block> all;
  std::vector<int> zero_seen(files.size(), 0);
  for (const OutBatch& o : got) {
    all.insert(all.end(), o.blocks.begin(), o.blocks.end());
    for (size_t u : o.zeros) CHECK(++zero_seen[u] == 1);
  }
  for (const auto& r : ranges)
    for (uint64_t g = r.first; g < r.second; ++g, ++bi) CHECK(bi < all.size() && all[bi].global == g);
  CHECK(bi == all.size());
  return 0;
}

// a run long enough to be cut: whole pieces and a rest
static int cuts() {
  for (int i = 0; i < 8; ++i) {
    const uint64_t bytes = i < 4 ? (uint64_t)i * cir::kReadPiece + (i == 0)
                                 : rnd() % (5 * cir::kReadPiece) + 1;
    const uint64_t off0 = rnd() % (1ull << 40), dst = rnd() % (1ull << 30) * 16;
    std::vector<Job> jobs;
    cir::cut_pieces(jobs, Job{off0, bytes, dst, 7});
    CHECK(tiles(jobs, 0, off0, bytes, dst, 7));
    CHECK(jobs.size() == (bytes + cir::kReadPiece - 1) / cir::kReadPiece);
  }
  return 0;
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20240611;
  for (case_no = 0; case_no < cases; ++case_no)
    if (one() || (case_no % 64 == 0 && cuts())) return 1;
  printf("pack_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
