// cir_check_index: the re-hash loop of commit_image over a whole image
// (and, below it, cir_check_links: the same pipeline with a verdict per file
// for the hardlink candidates of check_and_hardlink, cir_check_blocks: the
// same pipeline with a verdict per block, for the resume of a partial image,
// and cir_load_blocks: cir_check_blocks that keeps the bytes it read, in
// device buffers of the caller's).
//
// Reference: commit_image (src/daemon/disk/commit.rs:51-117) walks the
// index's entries in order, re-hashes every non-empty file
// (Hashes::check_file, :104) and fails with Error::Checksum(path) at the
// first file that does not match (:108-111), at an "empty" file that is not
// empty (:79-81), or with Error::ReadFile at one it cannot open or read
// (:98-106).  Here the whole image goes through the scan's staging pipeline
// (scan.cpp hash_range: file segments packed into pinned slots by reader
// threads, three slots in flight) in a check mode: a batch's expected digests
// travel up with its descriptors, the batch is hashed and compared on the
// device (kernels.hip k_first_bad) and 16 bytes come back per batch.
//
// Order.  Every file entry has a place in the index's order and every block
// of a non-empty file a global index g (blocks counted in index order, from
// the index alone).  A failure's key is (entry, g): for a bad block its file
// and its g, for a failure met on the host (a file that cannot be opened, a
// length that differs, a non-empty "empty" file) the entry and the g at
// which the packer met it.  The verdict is the smallest key.  One device
// packs in index order and retires batches in submission order, so when it
// meets a host-side failure every earlier block is packed: it stops packing,
// drains what is in flight, and the smallest key reported wins.  With several
// devices (stripes of the global block order dealt round-robin, as
// hash_files deals them) each device does the same over its stripes and may
// stop early only when a failure already known lies below everything it has
// yet to pack -- so whatever the timing, nothing below the final minimum is
// ever skipped and the verdict does not depend on it.
//
// Descriptors.  A batch may hold thousands of one-block files, so no fd is
// kept per packed file: the packer opens each file (openat in its directory,
// O_NOFOLLOW), fstats it, remembers (st_dev, st_ino, st_size) and closes it;
// a reader thread opens it again the same way -- every directory component
// with openat(O_DIRECTORY | O_NOFOLLOW) below the root fd, never by a path
// -- and reads only if fstat shows the same file.  Each packer holds one
// directory fd and each reader one directory and one file fd.
//
// The three entry points share everything that is not their policy: the
// slot's layout and the walk through the block ranges (pack.hpp), and below
// the index's layout (load_index), the readers (run_reads), the deal of
// stripes to devices (run_striped) and, from stage.hpp (cir_store_blocks uses
// them too), the directory cache and the rotation over a device's slots
// (rotate_slots).
#include <errno.h>
#include <fcntl.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "bits.hpp"
#include "dirsig.hpp"
#include "linkpath.hpp"
#include "pack.hpp"
#include "reload.hpp"
#include "runtime.hpp"
#include "scatter.hpp"
#include "stage.hpp"
#include "stripes.hpp"

namespace cir {
namespace {

using namespace stage;

constexpr uint64_t kNone = ~0ull;

// Parse and validate the index; the entries' places: directory lines as
// components, files with the global index of their first block.
int load_index(const uint8_t* index, size_t len, Layout* t) {
  dirsig::Index& idx = t->idx;
  std::string err;
  if (!dirsig::parse(index, len, &idx, &err)) return parse_fail(idx.bad_hash_size, err);
  if (dirsig::digest_len(idx.header.hash) != 32)
    return fail(CIR_EHASHSIZE, "hash size is unsupported");
  if (idx.header.block_size > 0xffffffffull)
    return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  t->bs = idx.header.block_size;
  t->ht = idx.header.hash == dirsig::HashType::kSha512_256 ? CIR_HASH_SHA512_256
                                                            : CIR_HASH_BLAKE2B_256;
  for (size_t e = 0; e < idx.entries.size(); ++e) {
    const dirsig::Entry& en = idx.entries[e];
    if (en.kind == dirsig::EntryKind::kDir) {
      std::vector<std::string> comps;
      size_t i = 0;
      while (i < en.path.size()) {
        size_t j = en.path.find('/', i);
        if (j == std::string::npos) j = en.path.size();
        if (j > i) comps.push_back(en.path.substr(i, j - i));
        i = j + 1;
      }
      t->dirs.push_back(std::move(comps));
    } else if (en.kind == dirsig::EntryKind::kFile) {
      if (t->dirs.empty()) return fail(CIR_EPARSE, "error parsing index: entry before a directory");
      Item it;
      it.entry = e;
      it.dir = t->dirs.size() - 1;
      it.name = en.path.substr(en.path.find_last_of('/') + 1);
      it.size = en.size;
      it.nblk = en.hashes.size() / 32;
      it.first_blk = t->nblk_total;
      t->nblk_total += it.nblk;
      t->items.push_back(std::move(it));
    }
    // symlink entries are the caller's to create (commit.rs:118-126)
  }
  return CIR_OK;
}

// openat + fstat of a listed non-empty file: 0 with *fd_out open, or the
// failure's kind with *err.  (O_NONBLOCK: a fifo in the file's place fails
// the fstat test below instead of blocking the open.)
int open_listed(FdCount& fds, const DirFd& d, const std::string& name, int* fd_out,
                struct stat* st, int* err) {
  *fd_out = -1;
  *err = 0;
  if (d.fd < 0) {
    *err = d.err;
    return CIR_CHECK_READ;
  }
  const int fd =
      fds.took(::openat(d.fd, name.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC | O_NONBLOCK));
  if (fd < 0) {
    *err = errno;
    return CIR_CHECK_READ;
  }
  if (::fstat(fd, st) != 0) {
    *err = errno;
    fds.close(fd);
    return CIR_CHECK_READ;
  }
  if (!S_ISREG(st->st_mode)) {
    *err = S_ISDIR(st->st_mode) ? EISDIR : EINVAL;
    fds.close(fd);
    return CIR_CHECK_READ;
  }
  *fd_out = fd;
  return CIR_CHECK_OK;
}

// One piece of a packed file for a reader: where to open the file again,
// what it must then be, and what to read of it.
struct ReadJob {
  int root;  // below this fd, in Layout::dirs[dir], by name
  size_t dir;
  const std::string* name;
  Seen seen;
  uint64_t min_len, max_len;  // the length the reopened file may have
  uint64_t file_off, len;
  uint8_t* dst;
  size_t tag;  // the caller's
};

// Read the batch's jobs on `threads` readers, each with a directory of its
// own kept across the jobs that share it.  A job that fails goes to
// on_fail(job index, errno) on the reader's thread: ESTALE when the file is
// not the one that was packed or has another length than allowed, ENODATA
// when it shrank under the read.  With `skip_after` the readers pass over
// the jobs after *skip_after (on_fail may lower it); without it every job
// is tried.
template <class Fail>
void run_reads(Layout& t, const std::vector<ReadJob>& jobs, unsigned threads, Fail on_fail,
               const std::atomic<size_t>* skip_after = nullptr) {
  std::atomic<size_t> next{0};
  const bool nt = stage_copy_nt();
  auto worker = [&] {
    DirCache dir(t);
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= jobs.size() || (skip_after && i > skip_after->load())) break;
      const ReadJob& j = jobs[i];
      int fd = -1, e = 0;
      struct stat st;
      bool ok =
          open_listed(t.fds, dir.of(j.root, j.dir), *j.name, &fd, &st, &e) == CIR_CHECK_OK;
      if (ok && (st.st_dev != j.seen.dev || st.st_ino != j.seen.ino ||
                 (uint64_t)st.st_size < j.min_len || (uint64_t)st.st_size > j.max_len)) {
        ok = false;
        e = ESTALE;
      }
      uint64_t got = 0;
      while (ok && got < j.len) {
        const ssize_t r =
            pread_staged(fd, j.dst + got, j.len - got, (off_t)(j.file_off + got), nt);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          ok = false;
          e = r == 0 ? ENODATA : errno;
          break;
        }
        got += (uint64_t)r;
      }
      t.fds.close(fd);
      if (!ok) on_fail(i, e);
    }
  };
  parallel_run(std::max(1u, std::min<unsigned>(threads, (unsigned)jobs.size())), worker);
}

// The global block order [0, nblk_total) over the context's devices:
// fn(device index, device, reader threads, its block ranges) on one device
// with the whole order, or on each of several with the stripes dealt to it
// round-robin (as hash_files deals them), each on a thread of its own with
// threads / devices readers.  The first failure in device order is returned.
template <class Fn>
int run_striped(cir_ctx* ctx, uint64_t nblk_total, uint64_t bs, unsigned threads, Fn fn) {
  if (nblk_total == 0) return CIR_OK;  // nothing for a device
  if (threads == 0) threads = host_copy_threads(ctx->devs.size());
  const size_t nd = (size_t)std::min<uint64_t>(ctx->devs.size(), nblk_total);
  if (nd <= 1) return fn((size_t)0, *ctx->devs[0], threads, BlockRanges{{0, nblk_total}});
  uint64_t stripe = std::max<uint64_t>(1, ctx->staging / bs);
  if (const char* e = getenv("CIR_DEBUG_STRIPE_BLOCKS"))  // tests: stripes of a few blocks
    if (atoll(e) > 0) stripe = (uint64_t)atoll(e);
  const StripePrefix order(nblk_total, stripe);
  std::vector<BlockRanges> dev_ranges(nd);
  for (size_t st = 0; st < order.stripes(); ++st)
    dev_ranges[st % nd].push_back({st * stripe, st * stripe + order.stripe_len(st)});
  const unsigned per = std::max(1u, threads / (unsigned)nd);
  std::vector<int> rcs(nd, 0);
  std::vector<std::string> errs(nd);
  fan_out(nd, [&](size_t i) {
    if (dev_ranges[i].empty()) return;
    rcs[i] = fn(i, *ctx->devs[i], per, dev_ranges[i]);
    if (rcs[i]) errs[i] = cir_last_error();
  });
  for (size_t i = 0; i < nd; ++i)
    if (rcs[i]) return fail(rcs[i], errs[i]);
  return CIR_OK;
}

// ---- cir_check_index ------------------------------------------------------

struct Failure {
  size_t item = SIZE_MAX;
  uint64_t blk = kNone;  // second half of the key
  int kind = CIR_CHECK_OK;
  int err = 0;
  uint64_t bad_blk = kNone;  // the first bad block, when that is what failed
  bool before(size_t it, uint64_t b) const { return item < it || (item == it && blk < b); }
};

struct Image : Layout {
  // the smallest failure reported so far
  std::mutex mu;
  Failure best;
  std::atomic<uint64_t> n_files{0}, n_blocks{0}, n_bytes{0}, n_batches{0}, n_empty{0};

  void report(size_t item, uint64_t blk, int kind, int err, uint64_t bad_blk = kNone) {
    std::lock_guard<std::mutex> lk(mu);
    const Failure f{item, blk, kind, err, bad_blk};
    if (f.before(best.item, best.blk)) best = f;
  }
  // a failure is known below (it, b): nothing from there on can be the verdict
  bool decided_before(size_t it, uint64_t b) {
    std::lock_guard<std::mutex> lk(mu);
    return best.before(it, b);
  }
  // the non-empty file that holds global block g
  size_t item_of(uint64_t g) const {
    size_t i = std::upper_bound(items.begin(), items.end(), g,
                                [](uint64_t b, const Item& x) { return b < x.first_blk; }) -
               items.begin();
    // (empty files share the next file's first_blk and sort before it: the
    // last item whose first_blk <= g is the file itself)
    return i - 1;
  }
};

// A size-0 entry (commit.rs:57-90): absent passes (the caller creates it),
// present it must be an empty regular file.
int examine_empty(const DirFd& d, const Item& it, int* err) {
  *err = 0;
  if (d.fd < 0) {
    if (d.err == ENOENT) return CIR_CHECK_OK;
    *err = d.err;
    return CIR_CHECK_READ;
  }
  struct stat st;
  if (::fstatat(d.fd, it.name.c_str(), &st, AT_SYMLINK_NOFOLLOW) != 0) {
    if (errno == ENOENT) return CIR_CHECK_OK;
    *err = errno;
    return CIR_CHECK_READ;
  }
  return S_ISREG(st.st_mode) && st.st_size == 0 ? CIR_CHECK_OK : CIR_CHECK_CHECKSUM;
}

// A non-empty entry before it is packed: READ, CHECKSUM on a length that is
// not the index's (the verdict cir_check_file gives: wrong block count, or a
// last block that cannot match), else what identifies the file to the readers.
int examine_file(Image& im, const DirFd& d, const Item& it, Seen* seen, int* err) {
  int fd = -1;
  struct stat st;
  const int kind = open_listed(im.fds, d, it.name, &fd, &st, err);
  if (kind) return kind;
  im.fds.close(fd);
  if ((uint64_t)st.st_size != it.size) return CIR_CHECK_CHECKSUM;
  seen->dev = st.st_dev;
  seen->ino = st.st_ino;
  return CIR_CHECK_OK;
}

// The block ranges `ranges` (increasing) on device d, with the entries each
// range owns -- those whose first block lies in it, the trailing empty files
// with the last range -- examined in order as the packer reaches them.  Every
// failure goes to im.report().
int check_range(cir_ctx* ctx, Device& d, Image& im, unsigned threads, const BlockRanges& ranges) {
  const std::vector<Item>& items = im.items;
  uint64_t seg = 0;
  for (const Item& it : items) seg = std::max(seg, std::min<uint64_t>(it.size, im.bs));
  SlotSizes sz = slot_sizes(ctx->staging, seg, scan_ramp());
  RangeCursor cur(
      items.size(), [&](size_t i) { return std::make_pair(items[i].first_blk, items[i].nblk); },
      ranges, im.nblk_total);
  Seen seen;             // of the item whose host-side look passed (cur.looked)
  bool stopped = false;  // nothing further is packed
  DirCache dir(im);      // the packer's directory
  // the batch being packed: its first global block, and where each of its
  // runs starts (ReadJob::tag names the run)
  struct Seg {
    size_t item;
    uint64_t blk, pos;
  };
  Batch b;
  uint64_t first = 0, new_files = 0, file_bytes = 0;
  std::vector<ReadJob> jobs;
  std::vector<Seg> segs;
  // (another device's failure below everything left here ends this one)
  auto more = [&] {
    if (stopped || !cur.more()) return false;
    if (im.decided_before(cur.ui, cur.at())) stopped = true;
    return !stopped;
  };
  auto retire = [&](int, Slot& s) {
    const uint64_t bad = s.h_cell[0];
    if (bad == kNone) return;
    im.report(im.item_of(bad), bad, CIR_CHECK_CHECKSUM, 0, bad);
    stopped = true;  // what is still in flight lies above it and is only drained
  };
  auto pack = [&](int, Slot& s) {
    b = Batch();
    first = cur.at();
    new_files = file_bytes = 0;
    jobs.clear();
    segs.clear();
    while (!stopped && cur.here() && b.n < sz.cap_blk) {
      const Item& it = items[cur.ui];
      const DirFd& dfd = dir.of(im.root, it.dir);
      int err = 0;
      int kind = CIR_CHECK_OK;
      if (it.nblk == 0)
        kind = examine_empty(dfd, it, &err);
      else if (cur.looked != cur.ui)
        kind = examine_file(im, dfd, it, &seen, &err);
      if (kind) {
        im.report(cur.ui, cur.at(), kind, err);
        stopped = true;
        break;
      }
      if (it.nblk == 0) {
        im.n_empty.fetch_add(1);
        cur.advance(0);
        continue;
      }
      cur.looked = cur.ui;
      const uint64_t fblk = cur.fblk;
      const Run r = pack_run(b, sz.fill, sz.cap_blk, im.bs, it.size, fblk, cur.left(), s.h_off,
                             s.h_len);
      if (!r.take) break;
      // the index's digests of these blocks, in block order (nothing comes
      // back through h_out in this mode: it carries them up)
      memcpy(s.h_out + 32 * r.at, im.digests(it, fblk), 32 * r.take);
      cut_pieces(jobs, ReadJob{im.root, it.dir, &it.name, seen, it.size, it.size, fblk * im.bs,
                               r.bytes, s.h_data + r.pos, segs.size()});
      segs.push_back({cur.ui, r.at, r.pos});
      if (fblk == 0) ++new_files;
      file_bytes += r.bytes;
      cur.advance(r.take);
    }
    return b.n > 0;
  };
  // The first job (in job order, whatever the timing: a reader skips only
  // jobs after a failed one) that fails makes READ at its file: the batch
  // keeps the blocks before that run (any of them may still be the verdict),
  // nothing further is packed.
  auto read = [&](int, Slot&) {
    std::atomic<size_t> bad{jobs.size()};
    std::mutex mu;
    int bad_err = 0;
    run_reads(
        im, jobs, threads,
        [&](size_t i, int e) {
          std::lock_guard<std::mutex> lk(mu);
          if (i < bad.load()) {
            bad.store(i);
            bad_err = e;
          }
        },
        &bad);
    if (bad.load() == jobs.size()) return;
    const Seg& g = segs[jobs[bad.load()].tag];
    im.report(g.item, first + g.blk, CIR_CHECK_READ, bad_err);
    stopped = true;
    b.n = g.blk;
    b.used = g.pos;
  };
  auto submit = [&](int, Slot& s) -> int {
    if (b.n == 0) return CIR_OK;
    const int rc = slot_submit_check(d, s, std::max<uint64_t>(b.used, 16), b.n, im.ht, first);
    if (rc) return rc;
    im.n_files.fetch_add(new_files);
    im.n_blocks.fetch_add(b.n);
    im.n_bytes.fetch_add(file_bytes);
    im.n_batches.fetch_add(1);
    return CIR_OK;
  };
  Laps laps(false);  // (this pipeline prints no trace line)
  return rotate_slots(d, sz, &Device::ensure_check, laps, more, retire, pack, read, submit);
}

int check_impl(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
               uint32_t threads, int* kind_out, uint8_t** path_out, size_t* path_len,
               uint64_t* stats) {
  if (!ctx || !index || !kind_out || !path_out || !path_len || !stats)
    return fail(CIR_EINVAL, "null pointer");
  *kind_out = CIR_CHECK_OK;
  *path_out = nullptr;
  *path_len = 0;
  for (int i = 0; i < CIR_CHECK_STATS_FIELDS; ++i) stats[i] = 0;
  stats[7] = kNone;
  Image im;
  int rc = load_index(index, len, &im);
  if (rc) return rc;
  rc = open_image(im, dirfd, dir);
  if (rc) return rc;
  if (im.nblk_total == 0) {
    // only size-0 entries (or none): nothing for a device
    DirCache cur(im);
    for (size_t i = 0; i < im.items.size(); ++i) {
      const Item& it = im.items[i];
      int e = 0;
      const int kind = examine_empty(cur.of(im.root, it.dir), it, &e);
      if (kind) {
        im.report(i, 0, kind, e);
        break;
      }
      im.n_empty.fetch_add(1);
    }
  } else {
    rc = run_striped(ctx, im.nblk_total, im.bs, threads,
                     [&](size_t, Device& d, unsigned per, const BlockRanges& ranges) {
                       return check_range(ctx, d, im, per, ranges);
                     });
  }
  stats[5] = im.fds.peak.load();
  if (rc) return rc;
  const Failure& f = im.best;
  if (f.kind != CIR_CHECK_OK) {
    const std::string& p = im.idx.entries[im.items[f.item].entry].path;
    uint8_t* out = (uint8_t*)malloc(p.size() + 1);
    if (!out) return fail(CIR_ENOMEM, "malloc");
    memcpy(out, p.data(), p.size());
    out[p.size()] = 0;
    *path_out = out;
    *path_len = p.size();
    *kind_out = f.kind;
    stats[6] = f.kind == CIR_CHECK_READ ? (uint64_t)f.err : 0;
    stats[7] = f.bad_blk;
    return CIR_OK;
  }
  stats[0] = im.n_files.load();
  stats[1] = im.n_blocks.load();
  stats[2] = im.n_bytes.load();
  stats[3] = im.n_batches.load();
  stats[4] = im.n_empty.load();
  return CIR_OK;
}

// ---- cir_check_links ------------------------------------------------------
//
// try_hardlink (src/daemon/disk/public.rs:308-346) over every candidate of
// check_and_hardlink (:285-305) in one call.  The pipeline is check_range's
// without its order and its stop: every candidate is on its own (:303), so a
// failure is written to the candidate's own verdict and packing goes on.  The
// candidates are worked through by source root and index order (a packer's
// and a reader's directory fd serves the neighbours too); their blocks,
// counted in that order, are what several devices take stripes of.  A batch's
// segment table (one segment = one candidate's run of blocks in the batch)
// travels up with the descriptors, k_seg_bad answers per segment, and 16 +
// nseg bytes come back.
//
// cir_check_links_at is the same call with a place per candidate: the
// candidate is looked for at a path the caller gives (cir_file_copies': the
// file's path in the source) instead of the entry's own.  A candidate carries
// its place, a directory and a name; the directories of the given paths are
// interned behind the index's own in Layout::dirs, so DirCache and ReadJob
// serve both.  What is expected of the file -- size, mode bits, digests -- is
// the entry's either way.  The paths come from another party's index and are
// validated before any I/O (linkpath.hpp).

struct Cand {
  size_t item = 0;         // index into Links::items: what the file must be
  uint32_t src = 0;        // source root
  size_t out = 0;          // the caller's candidate number
  uint64_t first_blk = 0;  // global index of block 0 in the work order
  size_t dir = 0;          // where it is looked for: index into Layout::dirs ...
  const std::string* name = nullptr;  // ... and the name there (the item's, or one of Links::names)
};

// (Layout::nblk_total and Item::first_blk count every file entry's blocks;
// the candidates' blocks are counted by Cand::first_blk and nblk_cand.)
struct Links : Layout {
  std::vector<int> roots;   // per source: its fd, or -1 with root_err
  std::vector<int> root_err;
  std::vector<Cand> cands;  // the non-empty candidates below a root that opened, in work order
  std::deque<std::string> names;  // the names of the caller's paths (addresses stay)
  uint64_t nblk_cand = 0;
  std::mutex mu;
  uint8_t* kind = nullptr;  // per candidate of the caller
  int32_t* err = nullptr;
  std::atomic<uint64_t> n_blocks{0}, n_bytes{0}, n_batches{0};

  // READ wins over CHECKSUM; the first READ's errno stays
  void report(size_t out, int k, int e) {
    std::lock_guard<std::mutex> lk(mu);
    if (k == CIR_CHECK_READ) {
      if (kind[out] != CIR_CHECK_READ) {
        kind[out] = CIR_CHECK_READ;
        err[out] = e;
      }
    } else if (kind[out] == CIR_CHECK_OK) {
      kind[out] = (uint8_t)k;
    }
  }
  bool exe(const Item& it) const { return idx.entries[it.entry].exe; }
};

// The packer's look at a candidate (try_hardlink without the read): READ,
// CHECKSUM on a length or mode bits (public.rs:331-338) that are not the
// entry's, else what identifies the file to the readers.
int examine_link(Links& L, const DirFd& d, const std::string& name, const Item& it, Seen* seen,
                 int* err) {
  int fd = -1;
  struct stat st;
  const int kind = open_listed(L.fds, d, name, &fd, &st, err);
  if (kind) return kind;
  L.fds.close(fd);
  if ((uint64_t)st.st_size != it.size) return CIR_CHECK_CHECKSUM;
  if ((st.st_mode & 0777) != (L.exe(it) ? 0755u : 0644u)) return CIR_CHECK_CHECKSUM;
  seen->dev = st.st_dev;
  seen->ino = st.st_ino;
  return CIR_CHECK_OK;
}

// check_range for the candidates: the block ranges `ranges` (increasing, of
// the work order's global blocks) on device d.  A candidate is examined by
// every range that holds some of its blocks; what fails the look is reported
// and its blocks in the range are passed over.
int links_range(cir_ctx* ctx, Device& d, Links& L, unsigned threads, const BlockRanges& ranges) {
  const std::vector<Cand>& cands = L.cands;
  uint64_t seg = 0;
  for (const Cand& c : cands) seg = std::max(seg, std::min<uint64_t>(L.items[c.item].size, L.bs));
  SlotSizes sz = slot_sizes(ctx->staging, seg, scan_ramp());
  RangeCursor cur(
      cands.size(),
      [&](size_t i) { return std::make_pair(cands[i].first_blk, L.items[cands[i].item].nblk); },
      ranges, L.nblk_cand);
  Seen seen;        // of the candidate whose look passed (cur.looked)
  DirCache dir(L);  // the packer's directory
  std::vector<size_t> seg_cand[Device::kSlots];  // per slot in flight: each segment's Cand::out
  Batch b;
  uint64_t file_bytes = 0;
  std::vector<ReadJob> jobs;
  auto retire = [&](int k, Slot& s) {
    uint32_t nbad = 0;
    memcpy(&nbad, s.h_seg_res, 4);
    if (!nbad) return;
    const uint8_t* flags = s.h_seg_res + kSegResHead;
    for (size_t g = 0; g < seg_cand[k].size(); ++g)
      if (flags[g]) L.report(seg_cand[k][g], CIR_CHECK_CHECKSUM, 0);
  };
  auto pack = [&](int k, Slot& s) {
    std::vector<size_t>& segs = seg_cand[k];
    segs.clear();
    jobs.clear();
    b = Batch();
    file_bytes = 0;
    while (cur.here() && b.n < sz.cap_blk) {
      const Cand& c = cands[cur.ui];
      const Item& it = L.items[c.item];
      if (cur.looked != cur.ui) {
        int err = 0;
        const int kind = examine_link(L, dir.of(L.roots[c.src], c.dir), *c.name, it, &seen, &err);
        if (kind) {
          L.report(c.out, kind, err);
          cur.advance(cur.left());  // its blocks in this range are passed over
          continue;
        }
        cur.looked = cur.ui;
      }
      const uint64_t fblk = cur.fblk;
      const Run r =
          pack_run(b, sz.fill, sz.cap_blk, L.bs, it.size, fblk, cur.left(), s.h_off, s.h_len);
      if (!r.take) break;
      // the entry's digests of these blocks travel up through h_out
      memcpy(s.h_out + 32 * r.at, L.digests(it, fblk), 32 * r.take);
      // a failed read makes READ of its own candidate and of nothing else (its
      // bytes in the slot are then whatever they are: READ wins over what the
      // compare finds)
      cut_pieces(jobs, ReadJob{L.roots[c.src], c.dir, c.name, seen, it.size, it.size,
                               fblk * L.bs, r.bytes, s.h_data + r.pos, c.out});
      s.h_seg_end[segs.size()] = (uint32_t)b.n;  // (at most one segment per block: <= cap_blk)
      segs.push_back(c.out);
      file_bytes += r.bytes;
      cur.advance(r.take);
    }
    return b.n > 0;
  };
  auto read = [&](int, Slot&) {
    run_reads(L, jobs, threads,
              [&](size_t i, int e) { L.report(jobs[i].tag, CIR_CHECK_READ, e); });
  };
  auto submit = [&](int k, Slot& s) -> int {
    const int rc = slot_submit_links(d, s, std::max<uint64_t>(b.used, 16), b.n, L.ht,
                                     seg_cand[k].size());
    if (rc) return rc;
    L.n_blocks.fetch_add(b.n);
    L.n_bytes.fetch_add(file_bytes);
    L.n_batches.fetch_add(1);
    return CIR_OK;
  };
  Laps laps(trace_enabled());
  const int rc = rotate_slots(
      d, sz, &Device::ensure_links, laps, [&] { return cur.more(); }, retire, pack, read, submit);
  if (rc) return rc;
  if (laps.on)
    fprintf(stderr,
            "cir check_links dev %d: %llu batches; packer's look and segment table %.2f ms, "
            "reads %.2f ms, submit %.2f ms, waiting for results and flags %.2f ms\n",
            d.id, (unsigned long long)laps.batches, laps.pack, laps.read, laps.submit, laps.wait);
  return CIR_OK;
}

// link_path_off == nullptr: cir_check_links, every candidate at its entry's own path.
int links_impl(cir_ctx* ctx, const uint8_t* index, size_t len, const int* src_dirfd,
               const char* const* src_dir, size_t nsrc, const uint64_t* link_file,
               const uint32_t* link_src, const uint64_t* link_path_off, const uint8_t* link_paths,
               size_t nlinks, uint32_t threads, uint8_t* kind_out, int32_t* errno_out,
               uint64_t* stats) {
  if (!ctx || !index || !stats || (nsrc && (!src_dirfd || !src_dir)) ||
      (nlinks && (!link_file || !link_src || !kind_out)))
    return fail(CIR_EINVAL, "null pointer");
  if (link_path_off && nlinks && link_path_off[nlinks] > link_path_off[0] && !link_paths)
    return fail(CIR_EINVAL, "null pointer");
  for (int i = 0; i < CIR_LINKS_STATS_FIELDS; ++i) stats[i] = 0;
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  for (size_t i = 0; i < nlinks; ++i)
    if (link_src[i] >= nsrc) return fail(CIR_EINVAL, "link_src names no source root");
  Links L;
  const int prc = load_index(index, len, &L);
  if (prc) return prc;
  for (size_t i = 0; i < nlinks; ++i)
    if (link_file[i] >= L.items.size())
      return fail(CIR_EINVAL, "link_file is past the last file entry");
  // the candidates' places: the entry's own, or the caller's path split and
  // validated, its directory interned behind the index's own
  std::vector<size_t> place_dir(nlinks);
  std::vector<const std::string*> place_name(nlinks);
  std::vector<char> nul_path(nlinks, 0);
  {
    std::map<std::vector<std::string>, size_t> interned;
    std::vector<std::string> comps;
    for (size_t i = 0; i < nlinks; ++i) {
      const Item& it = L.items[(size_t)link_file[i]];
      place_dir[i] = it.dir;
      place_name[i] = &it.name;
      if (!link_path_off) continue;
      if (link_path_off[i + 1] < link_path_off[i])
        return fail(CIR_EINVAL, "link_path_off must not decrease");
      const linkpath::Verdict v = linkpath::split(link_paths + link_path_off[i],
                                                  (size_t)(link_path_off[i + 1] - link_path_off[i]),
                                                  &comps);
      if (v == linkpath::kInvalid)
        return fail(CIR_EINVAL, "a candidate's path has a `.` or `..` component or no component");
      if (v == linkpath::kNul) nul_path[i] = 1;
      if (v != linkpath::kOk) continue;
      L.names.push_back(std::move(comps.back()));
      place_name[i] = &L.names.back();
      comps.pop_back();
      const auto at = interned.emplace(comps, L.dirs.size());
      if (at.second) L.dirs.push_back(comps);
      place_dir[i] = at.first->second;
    }
  }
  // ---- nothing above touched a file or a device
  const double ms_parse = ms_since(t_start);
  const auto t_roots = std::chrono::steady_clock::now();
  std::vector<int32_t> errs(nlinks, 0);
  L.kind = kind_out;
  L.err = errs.data();
  for (size_t i = 0; i < nlinks; ++i) kind_out[i] = CIR_CHECK_OK;
  // the roots some candidate names
  L.roots.assign(nsrc, -1);
  L.root_err.assign(nsrc, 0);
  std::vector<char> used(nsrc, 0);
  struct CloseRoots {
    Links& L;
    const char* const* src_dir;
    ~CloseRoots() {
      for (size_t j = 0; j < L.roots.size(); ++j)
        if (src_dir[j]) L.fds.close(L.roots[j]);
    }
  } close_roots{L, src_dir};
  for (size_t i = 0; i < nlinks; ++i) used[link_src[i]] = 1;
  for (size_t j = 0; j < nsrc; ++j)
    if (used[j]) L.roots[j] = open_root(L.fds, src_dirfd[j], src_dir[j], &L.root_err[j]);
  // the work order: by root, then by directory, then by index order (the index's own
  // directories ascend with the file ordinals: without paths this is root, then index order)
  std::vector<size_t> order(nlinks);
  for (size_t i = 0; i < nlinks; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    if (link_src[a] != link_src[b]) return link_src[a] < link_src[b];
    if (place_dir[a] != place_dir[b]) return place_dir[a] < place_dir[b];
    return link_file[a] < link_file[b];
  });
  {
    DirCache cur(L);
    for (size_t i : order) {
      Cand c;
      c.item = (size_t)link_file[i];
      c.src = link_src[i];
      c.out = i;
      c.dir = place_dir[i];
      c.name = place_name[i];
      const Item& it = L.items[c.item];
      if (L.roots[c.src] < 0) {
        L.report(i, CIR_CHECK_READ, L.root_err[c.src]);
      } else if (nul_path[i]) {
        L.report(i, CIR_CHECK_READ, EINVAL);  // (no such name can be opened)
      } else if (it.nblk == 0) {
        // a size-0 candidate: an empty regular file of the right mode, seen by the host alone
        Seen seen;
        int e = 0;
        const int kind = examine_link(L, cur.of(L.roots[c.src], c.dir), *c.name, it, &seen, &e);
        if (kind) L.report(i, kind, e);
        ++stats[7];
      } else {
        c.first_blk = L.nblk_cand;
        L.nblk_cand += it.nblk;
        L.cands.push_back(c);
      }
    }
  }
  const double ms_roots = ms_since(t_roots);
  const auto t_pipe = std::chrono::steady_clock::now();
  const int rc = run_striped(ctx, L.nblk_cand, L.bs, threads,
                             [&](size_t, Device& d, unsigned per, const BlockRanges& ranges) {
                               return links_range(ctx, d, L, per, ranges);
                             });
  stats[6] = L.fds.peak.load();
  if (trace_enabled())
    fprintf(stderr,
            "cir check_links%s: %zu candidates; index parse %.2f ms, roots, work order and size-0 "
            "candidates %.2f ms, pipeline %.2f ms\n",
            link_path_off ? "_at" : "", nlinks, ms_parse, ms_roots, ms_since(t_pipe));
  if (rc) return rc;
  for (size_t i = 0; i < nlinks; ++i) {
    ++stats[kind_out[i] == CIR_CHECK_OK ? 0 : kind_out[i] == CIR_CHECK_CHECKSUM ? 1 : 2];
    if (errno_out) errno_out[i] = kind_out[i] == CIR_CHECK_READ ? errs[i] : 0;
  }
  stats[3] = L.n_blocks.load();
  stats[4] = L.n_bytes.load();
  stats[5] = L.n_batches.load();
  return CIR_OK;
}

// ---- cir_check_blocks -----------------------------------------------------
//
// The resume the reference does not have: after a restart it finds the image
// unfinished ("Resuming download", src/daemon/tracking/mod.rs:561-585), removes
// the partial .tmp directory (start_image, src/daemon/disk/public.rs:91-93) and
// queues every block again (fill_blocks, src/daemon/tracking/progress.rs:
// 129-170).  Here the directory is kept and every block of the index gets one
// bit: present and correct, or not.  The pipeline is links_range's -- no stop,
// every file on its own -- over one root in index order; a file may be short
// (only the blocks wholly inside the length the packer saw are packed), long
// (its blocks up to the entry's size are judged) or missing.  A slot keeps a
// host-side run table in place of a segment table: each run of packed blocks
// with its place in the batch and in the global block order; launch_block_bits
// answers with one bit per block of the batch and slot_wait's side copies each
// run's bits into the device's bitmap (bits.hpp).  Several devices take
// stripes of the global block order, each into a bitmap of its own; every
// block has one owner, so the merge is an OR and does not depend on timing.
//
// cir_load_blocks is the same pipeline with a destination per file (Blocks::
// dests): pack appends one scatter record (scatter.hpp) per packed run to the
// slot's table, the table goes up with the descriptors and launch_scatter_runs
// copies the batch's runs from the slot's device twin to the files' buffers
// behind the compare, on the compute stream.  A non-empty file without a
// destination is left out of the work list: nothing of it is looked at.  One
// device takes the whole image, the one the caller's stream belongs to.
//
// cir_reload_blocks (reload.cpp) is cir_load_blocks with a bitmap of the blocks
// still wanted (Blocks::want): the others already stand in the destinations,
// copied there from buffers resident in device memory.  A run taken from a file
// ends at the first unwanted block, unwanted blocks are passed over without
// being read, and a file none of whose blocks in the range is wanted is not
// looked at.

// What the looks and the reads found of a file.
constexpr uint8_t kLookAbsent = 1, kLookBlocked = 2, kLookShort = 4, kLookLong = 8;

struct Blocks : Layout {
  std::vector<size_t> work;  // the non-empty entries (indices into items), in index order
  std::mutex mu;
  // what the looks and the reads found of each file (kLook* bits), and the
  // errno of the first thing that blocked it
  std::vector<uint8_t> look;
  std::vector<int32_t> err;
  std::atomic<uint64_t> n_bytes{0}, n_batches{0}, n_unread{0};
  // cir_load_blocks: each file entry's device buffer (null: cir_check_blocks),
  // the bytes and records scattered, and the records a scatter found bad
  void* const* dests = nullptr;
  std::atomic<uint64_t> n_scat_bytes{0}, n_scat_recs{0}, n_scat_bad{0};
  // cir_reload_blocks: the blocks still to be read, over the global blocks
  // (null: all of them)
  const uint64_t* want = nullptr;

  void report(size_t item, uint8_t bits, int e = 0) {
    std::lock_guard<std::mutex> lk(mu);
    if ((bits & kLookBlocked) && !(look[item] & kLookBlocked)) err[item] = e;
    look[item] |= bits;
  }
};

// What keeps a file from being judged: ENOENT (on it or on a directory
// component) is ABSENT, everything else BLOCKED.
uint8_t look_of_errno(int e) { return e == ENOENT ? kLookAbsent : kLookBlocked; }

// The packer's look at a non-empty entry: false with the file's state
// reported, else what identifies the file to the readers and its length.
bool examine_block_file(Blocks& B, const DirFd& d, size_t item, Seen* seen, uint64_t* cur_len) {
  const Item& it = B.items[item];
  int fd = -1, e = 0;
  struct stat st;
  if (open_listed(B.fds, d, it.name, &fd, &st, &e) != CIR_CHECK_OK) {
    B.report(item, look_of_errno(e), e);
    return false;
  }
  B.fds.close(fd);
  seen->dev = st.st_dev;
  seen->ino = st.st_ino;
  *cur_len = (uint64_t)st.st_size;
  if (*cur_len < it.size) B.report(item, kLookShort);
  if (*cur_len > it.size) B.report(item, kLookLong);
  return true;
}

// A size-0 entry, judged by the host alone.
void examine_block_empty(Blocks& B, const DirFd& d, size_t item) {
  const Item& it = B.items[item];
  if (d.fd < 0) {
    B.report(item, look_of_errno(d.err), d.err);
    return;
  }
  struct stat st;
  if (::fstatat(d.fd, it.name.c_str(), &st, AT_SYMLINK_NOFOLLOW) != 0) {
    B.report(item, look_of_errno(errno), errno);
    return;
  }
  if (!S_ISREG(st.st_mode))  // (the errno an openat(O_NOFOLLOW) and the fstat test would give)
    B.report(item, kLookBlocked,
             S_ISDIR(st.st_mode) ? EISDIR : S_ISLNK(st.st_mode) ? ELOOP : EINVAL);
  else if (st.st_size != 0)
    B.report(item, kLookLong);
}

// One run of packed blocks: `count` blocks from block `at` of the batch are
// the global blocks from `global` on.
struct BitRun {
  uint64_t at, global, count;
};

// links_range for the blocks of one image: the block ranges `ranges`
// (increasing, of the global block order) on device d, their verdicts into
// `have` (this device's bitmap of the whole image, zeroed by the caller).  A
// file is looked at by every range that holds some of its blocks.
int blocks_range(cir_ctx* ctx, Device& d, Blocks& B, unsigned threads, const BlockRanges& ranges,
                 uint64_t* have) {
  const std::vector<size_t>& work = B.work;
  const uint64_t bs = B.bs;
  uint64_t seg = 0;
  for (size_t w : work) seg = std::max(seg, std::min<uint64_t>(B.items[w].size, bs));
  SlotSizes sz = slot_sizes(ctx->staging, seg, scan_ramp());
  RangeCursor cur(
      work.size(),
      [&](size_t i) { return std::make_pair(B.items[work[i]].first_blk, B.items[work[i]].nblk); },
      ranges, B.nblk_total);
  Seen seen;             // of the file whose look passed (cur.looked)
  uint64_t cur_len = 0;  // and its length at that look
  DirCache dir(B);       // the packer's directory
  std::vector<BitRun> runs[Device::kSlots];  // per slot in flight
  Batch b;
  uint64_t file_bytes = 0;
  uint64_t nscat = 0, nunits = 0;  // the batch's scatter table (with B.dests)
  std::vector<ReadJob> jobs;
  auto retire = [&](int k, Slot& s) {
    const uint64_t* bits = reinterpret_cast<const uint64_t*>(s.h_bits + kBitsResHead);
    for (const BitRun& r : runs[k]) copy_bits(have, r.global, bits, r.at, r.count);
    if (B.dests) B.n_scat_bad.fetch_add(s.h_scat[0]);
  };
  auto pack = [&](int k, Slot& s) {
    std::vector<BitRun>& rs = runs[k];
    rs.clear();
    jobs.clear();
    b = Batch();
    file_bytes = 0;
    nscat = nunits = 0;
    while (cur.here() && b.n < sz.cap_blk) {
      const size_t item = work[cur.ui];
      const Item& it = B.items[item];
      const uint64_t in_range = cur.left();
      uint64_t wanted = in_range;  // the blocks at the cursor that a run may take
      if (B.want) {
        // unwanted blocks are passed over before any look at the file
        const uint64_t pass = run_bits(B.want, cur.at(), in_range, false);
        if (pass) {
          cur.advance(pass);
          continue;
        }
        wanted = run_bits(B.want, cur.at(), in_range, true);
      }
      // the blocks that lie wholly inside the length the packer saw; the
      // others of this range are passed over (their bits stay 0), and so are
      // all of them when the look fails
      uint64_t avail = 0;
      if (cur.looked == cur.ui ||
          examine_block_file(B, dir.of(B.root, it.dir), item, &seen, &cur_len)) {
        cur.looked = cur.ui;
        avail = cur_len >= it.size ? it.nblk : cur_len / bs;
      }
      const uint64_t fblk = cur.fblk;
      if (fblk >= avail) {
        B.n_unread.fetch_add(B.want ? count_bits(B.want, cur.at(), in_range) : in_range);
        cur.advance(in_range);
        continue;
      }
      const Run r = pack_run(b, sz.fill, sz.cap_blk, bs, it.size, fblk,
                             std::min<uint64_t>(avail - fblk, wanted), s.h_off, s.h_len);
      if (!r.take) break;
      // the entry's digests of these blocks travel up through h_out
      memcpy(s.h_out + 32 * r.at, B.digests(it, fblk), 32 * r.take);
      // (a file that grew is fine; one that is another file, or shorter than
      // the packer saw it, blocks itself and nothing else)
      cut_pieces(jobs, ReadJob{B.root, it.dir, &it.name, seen, cur_len, UINT64_MAX, fblk * bs,
                               r.bytes, s.h_data + r.pos, item});
      if (!rs.empty() && rs.back().at + rs.back().count == r.at &&
          rs.back().global + rs.back().count == it.first_blk + fblk)
        rs.back().count += r.take;  // (neighbouring files, both complete: one run)
      else
        rs.push_back({r.at, it.first_blk + fblk, r.take});
      if (B.dests)  // (at most one record per block: <= cap_blk)
        nunits = scatter::record_of(r, (uint64_t)reinterpret_cast<uintptr_t>(B.dests[item]), fblk,
                                    bs, nunits,
                                    s.h_scat + kScatHead + scatter::kRunWords * nscat++);
      file_bytes += r.bytes;
      cur.advance(r.take);
    }
    return b.n > 0;
  };
  auto read = [&](int, Slot&) {
    run_reads(B, jobs, threads, [&](size_t i, int e) { B.report(jobs[i].tag, kLookBlocked, e); });
  };
  auto submit = [&](int, Slot& s) -> int {
    const uint64_t used = std::max<uint64_t>(b.used, 16);
    const int rc = B.dests ? slot_submit_load(d, s, used, b.n, B.ht, nscat, nunits)
                           : slot_submit_blocks(d, s, used, b.n, B.ht);
    if (rc) return rc;
    if (B.dests) {
      B.n_scat_bytes.fetch_add(file_bytes);
      B.n_scat_recs.fetch_add(nscat);
    }
    B.n_bytes.fetch_add(file_bytes);
    B.n_batches.fetch_add(1);
    return CIR_OK;
  };
  Laps laps(trace_enabled());
  const int rc = rotate_slots(
      d, sz, B.dests ? &Device::ensure_load : &Device::ensure_blocks, laps,
      [&] { return cur.more(); }, retire, pack, read, submit);
  if (rc) return rc;
  if (laps.on) {
    fprintf(stderr,
            "cir %s dev %d: %llu batches; packer's look and run table %.2f ms, "
            "reads %.2f ms, submit %.2f ms, waiting for results and bit runs %.2f ms\n",
            B.dests ? "load_blocks" : "check_blocks", d.id, (unsigned long long)laps.batches,
            laps.pack, laps.read, laps.submit, laps.wait);
    if (B.dests)
      fprintf(stderr, "cir load_blocks dev %d: %llu scatter records, %.1f per batch, %llu bytes\n",
              d.id, (unsigned long long)B.n_scat_recs.load(),
              laps.batches ? (double)B.n_scat_recs.load() / (double)laps.batches : 0.0,
              (unsigned long long)B.n_scat_bytes.load());
  }
  return CIR_OK;
}

// cir_load_blocks' own arguments: a device buffer per file entry, and the
// caller's stream.
struct LoadArgs {
  void* const* d_data;
  size_t ndata;
  void* stream;
  // cir_reload_blocks: what fills the destinations from resident buffers and
  // says which blocks it filled (reload.hpp); null: cir_load_blocks
  const ResidentFn* resident = nullptr;
};

// load == nullptr: cir_check_blocks.
int blocks_impl(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                uint32_t threads, uint64_t** have_out, uint64_t* nblk_out, uint8_t** state_out,
                int32_t** errno_out, size_t* nfiles_out, uint64_t* stats,
                const LoadArgs* load = nullptr) {
  if (!ctx || !index || !have_out || !nblk_out || !state_out || !nfiles_out || !stats)
    return fail(CIR_EINVAL, "null pointer");
  *have_out = nullptr;
  *nblk_out = 0;
  *state_out = nullptr;
  if (errno_out) *errno_out = nullptr;
  *nfiles_out = 0;
  for (int i = 0; i < (load ? CIR_LOAD_STATS_FIELDS : CIR_BLOCKS_STATS_FIELDS); ++i) stats[i] = 0;
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  Blocks B;
  int rc = load_index(index, len, &B);
  if (rc) return rc;
  const size_t nfiles = B.items.size();
  uint64_t n_skipped = 0;
  Device* load_dev = nullptr;
  if (load) {
    if (load->ndata != nfiles)
      return fail(CIR_EINVAL, "ndata is " + std::to_string(load->ndata) + ", the index has " +
                                  std::to_string(nfiles) + " file entries");
    if (nfiles && !load->d_data) return fail(CIR_EINVAL, "null pointer");
    load_dev = stream_device(ctx, (hipStream_t)load->stream);
    if (!load_dev) return fail(CIR_EINVAL, "stream device is not part of the context");
    B.dests = load->d_data;
  }
  // (a non-empty file without a destination is no work: it is not looked at)
  for (size_t i = 0; i < nfiles; ++i)
    if (B.items[i].nblk) {
      if (!load || load->d_data[i])
        B.work.push_back(i);
      else
        ++n_skipped;
    }
  // ---- nothing above touched a file or a device (a load asked which device
  // its stream belongs to)
  const double ms_parse = ms_since(t_start);
  const size_t nwords = (size_t)((B.nblk_total + 63) / 64);
  // cir_reload_blocks: the blocks taken from memory (empty: none were), and
  // with them the blocks still wanted
  std::vector<uint64_t> mem, want;
  if (load && load->resident) {
    rc = (*load->resident)(B, *load_dev, &mem);
    if (rc) return rc;
    if (!mem.empty()) {
      want.resize(nwords);
      for (size_t w = 0; w < nwords; ++w) want[w] = ~mem[w];
      B.want = want.data();
    }
  }
  const auto t_empty = std::chrono::steady_clock::now();
  rc = open_image(B, dirfd, dir);
  if (rc) return rc;
  B.look.assign(nfiles, 0);
  B.err.assign(nfiles, 0);
  // the outputs (calloc: every bit starts as "not have")
  struct Outs {
    uint64_t* have = nullptr;
    uint8_t* state = nullptr;
    int32_t* err = nullptr;
    ~Outs() {
      free(have);
      free(state);
      free(err);
    }
  } outs;
  if (nwords && !(outs.have = (uint64_t*)calloc(nwords, 8))) return fail(CIR_ENOMEM, "malloc");
  if (nfiles && !(outs.state = (uint8_t*)calloc(nfiles, 1))) return fail(CIR_ENOMEM, "malloc");
  if (nfiles && errno_out && !(outs.err = (int32_t*)calloc(nfiles, 4)))
    return fail(CIR_ENOMEM, "malloc");
  // the size-0 entries, by the host alone
  {
    DirCache cur(B);
    for (size_t i = 0; i < nfiles; ++i)
      if (!B.items[i].nblk) examine_block_empty(B, cur.of(B.root, B.items[i].dir), i);
  }
  const double ms_empty = ms_since(t_empty);
  const auto t_pipe = std::chrono::steady_clock::now();
  // a bitmap per device (stripes do not end on word boundaries); device 0
  // writes into the result itself
  std::vector<std::vector<uint64_t>> part(ctx->devs.size());
  if (!load) {
    rc = run_striped(ctx, B.nblk_total, B.bs, threads,
                     [&](size_t i, Device& d, unsigned per, const BlockRanges& ranges) {
                       if (i) part[i].assign(nwords, 0);
                       return blocks_range(ctx, d, B, per, ranges, i ? part[i].data() : outs.have);
                     });
    for (const std::vector<uint64_t>& p : part)
      for (size_t w = 0; w < p.size(); ++w) outs.have[w] |= p[w];
  } else if (!B.work.empty()) {
    // One device, the stream's.  Its compute stream -- the scatters run there
    // -- first waits for what the caller queued on `stream`: a producer or an
    // earlier user of the buffers is done before the first byte lands.
    rc = [&]() -> int {
      DeviceGuard guard;
      CIR_HIP(hipSetDevice(load_dev->id));
      hipEvent_t ev = nullptr;
      CIR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      hipError_t e = hipEventRecord(ev, (hipStream_t)load->stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(load_dev->compute, ev, 0);
      (void)hipEventDestroy(ev);  // (released once it has completed)
      if (e != hipSuccess) return hip_fail(e, "ordering the compute stream behind the caller's");
      return blocks_range(ctx, *load_dev, B, threads ? threads : host_copy_threads((size_t)1),
                          BlockRanges{{0, B.nblk_total}}, outs.have);
    }();
    if (!rc && B.n_scat_bad.load())
      rc = fail(CIR_EIO, "the scatter kernel met a record outside its slot");
  }
  stats[8] = B.fds.peak.load();
  if (trace_enabled())
    fprintf(stderr,
            "cir %s: %zu files, %llu blocks; index parse %.2f ms, root and size-0 "
            "entries %.2f ms, pipeline %.2f ms\n",
            load ? "load_blocks" : "check_blocks", nfiles, (unsigned long long)B.nblk_total,
            ms_parse, ms_empty, ms_since(t_pipe));
  if (rc) return rc;
  // (the pipeline read no block that memory gave: the two bitmaps are disjoint)
  for (size_t w = 0; B.want && w < nwords; ++w) outs.have[w] |= mem[w];
  // the files' states.  A file that is absent or blocked has none of its
  // blocks: whatever a range packed of it before it went is cleared (what
  // memory gave of it stays: those bytes stand in its destination).
  for (size_t i = 0; i < nfiles; ++i) {
    const Item& it = B.items[i];
    const uint8_t lk = B.look[i];
    uint8_t st;
    if (load && it.nblk && !load->d_data[i]) {  // (no bit of it was ever set)
      outs.state[i] = CIR_FILE_SKIPPED;
      continue;
    }
    if (B.want && it.nblk && count_bits(mem.data(), it.first_blk, it.nblk) == it.nblk) {
      outs.state[i] = CIR_FILE_COMPLETE | CIR_FILE_RESIDENT;  // (never looked at)
      ++stats[2];
      continue;
    }
    if (lk & kLookBlocked)
      st = CIR_FILE_BLOCKED;
    else if (lk & kLookAbsent)
      st = CIR_FILE_ABSENT;
    else if (!(lk & (kLookShort | kLookLong)) &&
             count_bits(outs.have, it.first_blk, it.nblk) == it.nblk)
      st = CIR_FILE_COMPLETE;
    else
      st = CIR_FILE_PARTIAL;
    if (st == CIR_FILE_BLOCKED || st == CIR_FILE_ABSENT) {
      if (B.want)
        copy_bits(outs.have, it.first_blk, mem.data(), it.first_blk, it.nblk);
      else
        clear_bits(outs.have, it.first_blk, it.nblk);
    } else if (lk & kLookLong) {
      st |= CIR_FILE_LONG;
    }
    outs.state[i] = st;
    if (outs.err) outs.err[i] = st == CIR_FILE_BLOCKED ? B.err[i] : 0;
    ++stats[2 + (st & 3)];
  }
  stats[0] = nwords ? count_bits(outs.have, 0, B.nblk_total) : 0;
  stats[1] = B.nblk_total - stats[0];
  stats[6] = B.n_bytes.load();
  stats[7] = B.n_batches.load();
  stats[9] = B.n_unread.load();
  if (load) {
    stats[10] = B.n_scat_bytes.load();
    stats[11] = n_skipped;
  }
  *have_out = outs.have;
  *nblk_out = B.nblk_total;
  *state_out = outs.state;
  if (errno_out) *errno_out = outs.err;
  *nfiles_out = nfiles;
  outs.have = nullptr;
  outs.state = nullptr;
  outs.err = nullptr;
  return CIR_OK;
}

// ---- cir_scatter_runs, cir_scatter_runs_dev: the scatter on its own ----------

int check_scatter(const void* src, const void* runs, uint64_t nruns, uint64_t nunits,
                  const void* res) {
  if ((nunits && !src) || (nruns && !runs) || !res) return fail(CIR_EINVAL, "null pointer");
  if (nruns > scatter::kMaxRuns) return fail(CIR_EINVAL, "more than 2^32-1 records");
  if (nunits > scatter::kMaxUnits) return fail(CIR_EINVAL, "more than 2^32-1 units");
  return CIR_OK;
}

int scatter_host_impl(const uint8_t* src, uint64_t src_bytes, const uint64_t* runs, uint64_t nruns,
                      uint64_t nunits, uint64_t* res) {
  const int rc = check_scatter(src, runs, nruns, nunits, res);
  if (rc) return rc;
  res[0] = scatter::apply_host(src, src_bytes, runs, nruns, nunits);
  return CIR_OK;
}

int scatter_dev_impl(const uint8_t* d_src, uint64_t src_bytes, const uint64_t* d_runs,
                     uint64_t nruns, uint64_t nunits, uint64_t* d_res, void* stream) {
  const int rc = check_scatter(d_src, d_runs, nruns, nunits, d_res);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(d_src) & 15u)
    return fail(CIR_EINVAL, "d_src must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_runs) | reinterpret_cast<uintptr_t>(d_res)) & 7u)
    return fail(CIR_EINVAL, "d_runs and d_res must be 8-byte aligned");
  CIR_HIP(dev::launch_scatter_runs(d_src, src_bytes, d_runs, nruns, nunits, d_res,
                                   (hipStream_t)stream));
  return CIR_OK;
}

}  // namespace

int load_blocks_resident(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                         uint32_t threads, void* const* d_data, size_t ndata, void* stream,
                         const ResidentFn* resident, uint64_t** have_out, uint64_t* nblk_out,
                         uint8_t** state_out, int32_t** errno_out, size_t* nfiles_out,
                         uint64_t* stats) {
  const LoadArgs load{d_data, ndata, stream, resident};
  return blocks_impl(ctx, dirfd, dir, index, len, threads, have_out, nblk_out, state_out,
                     errno_out, nfiles_out, stats, &load);
}

}  // namespace cir

extern "C" int cir_scatter_runs(const uint8_t* src, uint64_t src_bytes, const uint64_t* runs,
                                uint64_t nruns, uint64_t nunits,
                                uint64_t res[CIR_SCATTER_RES_FIELDS]) try {
  return cir::scatter_host_impl(src, src_bytes, runs, nruns, nunits, res);
} CIR_CATCH_BOUNDARY

extern "C" int cir_scatter_runs_dev(cir_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes,
                                    const uint64_t* d_runs, uint64_t nruns, uint64_t nunits,
                                    uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::scatter_dev_impl(d_src, src_bytes, d_runs, nruns, nunits, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_load_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index,
                               size_t len, uint32_t threads, void* const* d_data, size_t ndata,
                               void* stream, uint64_t** have_out, uint64_t* nblk_out,
                               uint8_t** state_out, int32_t** errno_out, size_t* nfiles_out,
                               uint64_t stats[CIR_LOAD_STATS_FIELDS]) try {
  const cir::LoadArgs load{d_data, ndata, stream};
  return cir::blocks_impl(ctx, dirfd, dir, index, len, threads, have_out, nblk_out, state_out,
                          errno_out, nfiles_out, stats, &load);
} CIR_CATCH_BOUNDARY

extern "C" int cir_check_blocks(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index,
                                size_t len, uint32_t threads, uint64_t** have_out,
                                uint64_t* nblk_out, uint8_t** state_out, int32_t** errno_out,
                                size_t* nfiles_out, uint64_t stats[CIR_BLOCKS_STATS_FIELDS]) try {
  return cir::blocks_impl(ctx, dirfd, dir, index, len, threads, have_out, nblk_out, state_out,
                          errno_out, nfiles_out, stats);
} CIR_CATCH_BOUNDARY

extern "C" int cir_check_links(cir_ctx* ctx, const uint8_t* index, size_t len,
                               const int* src_dirfd, const char* const* src_dir, size_t nsrc,
                               const uint64_t* link_file, const uint32_t* link_src, size_t nlinks,
                               uint32_t threads, uint8_t* kind_out, int32_t* errno_out,
                               uint64_t stats[CIR_LINKS_STATS_FIELDS]) try {
  return cir::links_impl(ctx, index, len, src_dirfd, src_dir, nsrc, link_file, link_src, nullptr,
                         nullptr, nlinks, threads, kind_out, errno_out, stats);
} CIR_CATCH_BOUNDARY

extern "C" int cir_check_links_at(cir_ctx* ctx, const uint8_t* index, size_t len,
                                  const int* src_dirfd, const char* const* src_dir, size_t nsrc,
                                  const uint64_t* link_file, const uint32_t* link_src,
                                  const uint64_t* link_path_off, const uint8_t* link_paths,
                                  size_t nlinks, uint32_t threads, uint8_t* kind_out,
                                  int32_t* errno_out, uint64_t stats[CIR_LINKS_STATS_FIELDS]) try {
  return cir::links_impl(ctx, index, len, src_dirfd, src_dir, nsrc, link_file, link_src,
                         link_path_off, link_paths, nlinks, threads, kind_out, errno_out, stats);
} CIR_CATCH_BOUNDARY

extern "C" int cir_check_index(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index,
                               size_t len, uint32_t threads, int* kind_out, uint8_t** path_out,
                               size_t* path_len, uint64_t stats[CIR_CHECK_STATS_FIELDS]) try {
  return cir::check_impl(ctx, dirfd, dir, index, len, threads, kind_out, path_out, path_len, stats);
} CIR_CATCH_BOUNDARY
