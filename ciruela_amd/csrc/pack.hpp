// How the staged loops (scan.cpp hash_range, check.cpp's three pipelines) lay
// file blocks out in a staging slot: the slot's sizes, the step that packs one
// run of a file's blocks into a batch, the cut of a run into read pieces, and
// the cursor that walks units of blocks through a list of block ranges.
// Host only, no dependencies: tools/pack_fuzz.cpp checks it against a
// restatement that goes one block at a time.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace cir {

// Read jobs are cut into pieces of at most this size so that `threads`
// readers stay busy on trees of large files.
constexpr uint64_t kReadPiece = 4ull << 20;

inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

// A slot's sizes.  A slot holds at least one block; a block is never longer
// than the largest file, so a huge block size over small files does not grow
// the slots to the block size.  (cap is a multiple of 16: runs start 16-byte
// aligned.)  The first batches ramp up (1/8, 1/4, 1/2 of a slot, then whole
// slots): the first upload starts after a short read instead of a whole
// slot's, and each read still finishes within the previous upload.
struct SlotSizes {
  uint64_t cap = 0;      // bytes of a slot
  uint64_t cap_blk = 0;  // blocks of a slot
  uint64_t fill = 0;     // bytes the next batch may use
  // a slot was offered for packing, whether or not anything went into it
  void offered() { fill = std::min(cap, fill * 2); }
};

// `seg`: the largest min(size, bs) of the files.
inline SlotSizes slot_sizes(uint64_t staging, uint64_t seg, bool ramp) {
  SlotSizes z;
  z.cap = align16(std::max<uint64_t>(staging, seg + 16));
  z.cap_blk = std::max<uint64_t>(z.cap / 512, 4096);
  z.fill = ramp ? std::max<uint64_t>(seg + 16, z.cap >> 3) : z.cap;
  return z;
}

// A batch while it is packed: `n` blocks so far, the next run starts at or
// after `pos`, the last run ended at `used` (pos may be aligned past it: only
// `used` bytes are uploaded).
struct Batch {
  uint64_t pos = 0, n = 0, used = 0;
};

// One run: `take` blocks of one file (0: the batch is full), `bytes` long, at
// byte `pos` of the slot, from block `at` of the batch on.
struct Run {
  uint64_t take = 0, at = 0, pos = 0, bytes = 0;
};

// Pack blocks fblk.. of a file of `size` bytes into the batch: at most
// left_blk (>= 1) of them, and only while b.n < cap_blk.  The run starts
// 16-byte aligned; it is refused when its first block does not fit below
// `fill`, and then takes as many blocks as fit, every one after the first
// counted at a full bs (so a short last block that does not fit by that count
// starts a run of its own in the same batch if its real length fits).  Block
// b.n + j of the batch gets h_off and h_len.
inline Run pack_run(Batch& b, uint64_t fill, uint64_t cap_blk, uint64_t bs, uint64_t size,
                    uint64_t fblk, uint64_t left_blk, uint64_t* h_off, uint32_t* h_len) {
  Run r;
  const uint64_t off0 = fblk * bs;
  b.pos = align16(b.pos);
  if (b.pos + std::min<uint64_t>(bs, size - off0) > fill) return r;
  r.take = std::min({left_blk, cap_blk - b.n, std::max<uint64_t>((fill - b.pos) / bs, 1)});
  r.bytes = std::min<uint64_t>(r.take * bs, size - off0);
  r.at = b.n;
  r.pos = b.pos;
  for (uint64_t j = 0; j < r.take; ++j) {
    h_off[r.at + j] = r.pos + j * bs;
    h_len[r.at + j] = (uint32_t)std::min<uint64_t>(bs, size - off0 - j * bs);
  }
  b.pos += r.bytes;
  b.used = b.pos;
  b.n += r.take;
  return r;
}

// The read jobs of one run: `whole` (file_off, len and dst of the whole run,
// the rest as every piece shall have it) cut into pieces of kReadPiece.
template <class Job>
void cut_pieces(std::vector<Job>& jobs, Job whole) {
  const uint64_t off0 = whole.file_off, bytes = whole.len;
  const auto dst = whole.dst;
  for (uint64_t piece = 0; piece < bytes; piece += kReadPiece) {
    whole.file_off = off0 + piece;
    whole.len = std::min<uint64_t>(kReadPiece, bytes - piece);
    whole.dst = dst + piece;
    jobs.push_back(whole);
  }
}

using BlockRanges = std::vector<std::pair<uint64_t, uint64_t>>;

// A walk over `count` units of blocks -- unit(i) = (first_blk, nblk), sorted
// by first_blk, a zero-block unit before the unit that shares its first_blk
// -- through the block ranges `ranges` (increasing; a range may start or end
// inside a unit).  A zero-block unit is a range's when it lies inside it, or
// at its end when that is the end of all blocks (nblk_total).
template <class Unit>
class RangeCursor {
 public:
  size_t ui = 0;               // the unit being packed
  uint64_t fblk = 0;           // its next block
  size_t looked = SIZE_MAX;    // the caller's: the unit it has examined in this range
  uint64_t b0 = 0, b1 = 0;     // the range being packed

  RangeCursor(size_t count, Unit unit, const BlockRanges& ranges, uint64_t nblk_total)
      : count_(count), unit_(unit), ranges_(ranges), total_(nblk_total) {
    start_range(0);
  }

  void start_range(size_t r) {
    ri_ = r;
    b0 = ranges_[r].first;
    b1 = ranges_[r].second;
    // the first unit at or past b0, or the unit b0 falls inside
    size_t lo = 0, hi = count_;
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (unit_(mid).first < b0)
        lo = mid + 1;
      else
        hi = mid;
    }
    ui = lo;
    fblk = 0;
    if (ui > 0 && unit_(ui - 1).first + unit_(ui - 1).second > b0) {
      --ui;
      fblk = b0 - unit_(ui).first;
    }
    looked = SIZE_MAX;
  }
  size_t range() const { return ri_; }
  uint64_t at() const { return unit_(ui).first + fblk; }  // the next block's global index
  // is unit ui (from block fblk on) this range's?
  bool here() const {
    if (ui >= count_) return false;
    const uint64_t a = at();
    return a < b1 || (b1 == total_ && a == b1 && unit_(ui).second == 0);
  }
  // something left in this or a later range (moves on to the next range)
  bool more() {
    while (!here()) {
      if (ri_ + 1 >= ranges_.size()) return false;
      start_range(ri_ + 1);
    }
    return true;
  }
  // the unit's blocks from fblk on that lie in this range
  uint64_t left() const { return std::min<uint64_t>(unit_(ui).second - fblk, b1 - at()); }
  // n blocks further (0 passes a zero-block unit)
  void advance(uint64_t n) {
    fblk += n;
    if (fblk == unit_(ui).second) {
      ++ui;
      fblk = 0;
    }
  }

 private:
  size_t count_;
  Unit unit_;
  const BlockRanges& ranges_;
  uint64_t total_;
  size_t ri_ = 0;
};

}  // namespace cir
