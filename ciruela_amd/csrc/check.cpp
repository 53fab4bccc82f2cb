// cir_check_index: the re-hash loop of commit_image over a whole image
// (and, below it, cir_check_links: the same pipeline with a verdict per file
// for the hardlink candidates of check_and_hardlink, and cir_check_blocks: the
// same pipeline with a verdict per block, for the resume of a partial image).
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
#include <mutex>
#include <string>
#include <vector>

#include "bits.hpp"
#include "dirsig.hpp"
#include "runtime.hpp"
#include "stripes.hpp"

namespace cir {
namespace {

constexpr uint64_t kNone = ~0ull;
// (scan.cpp's read piece: `threads` readers stay busy on large files)
constexpr uint64_t kReadPiece = 4ull << 20;

// The fds the check itself holds, and their peak (stats[5]).
struct FdCount {
  std::atomic<uint64_t> cur{0}, peak{0};
  int took(int fd) {
    if (fd >= 0) {
      const uint64_t c = cur.fetch_add(1) + 1;
      uint64_t p = peak.load();
      while (c > p && !peak.compare_exchange_weak(p, c)) {
      }
    }
    return fd;
  }
  void close(int fd) {
    if (fd < 0) return;
    ::close(fd);
    cur.fetch_sub(1);
  }
};

// One file entry of the index, in index order.
struct Item {
  size_t entry = 0;        // index into Index::entries
  size_t dir = 0;          // index into Image::dirs
  std::string name;        // the entry's name in its directory
  uint64_t size = 0;
  uint64_t nblk = 0;
  uint64_t first_blk = 0;  // global index of block 0 (an empty file: the next file's)
};

struct Failure {
  size_t item = SIZE_MAX;
  uint64_t blk = kNone;  // second half of the key
  int kind = CIR_CHECK_OK;
  int err = 0;
  uint64_t bad_blk = kNone;  // the first bad block, when that is what failed
  bool before(size_t it, uint64_t b) const { return item < it || (item == it && blk < b); }
};

struct Image {
  const dirsig::Index* idx = nullptr;
  uint64_t bs = 0;
  int ht = CIR_HASH_BLAKE2B_256;
  int root = -1;
  std::vector<std::vector<std::string>> dirs;  // a directory line's components below the root
  std::vector<Item> items;
  uint64_t nblk_total = 0;
  FdCount fds;
  // the smallest failure reported so far
  std::mutex mu;
  Failure best;
  std::atomic<uint64_t> n_files{0}, n_blocks{0}, n_bytes{0}, n_batches{0}, n_empty{0};

  void report(const Failure& f) {
    std::lock_guard<std::mutex> lk(mu);
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

// A directory below the root, opened one component at a time, never through
// a symlink.  No components: the root fd itself (not ours to close).
struct DirFd {
  int fd = -1;
  bool own = false;
  int err = 0;  // errno when fd < 0
};

DirFd open_dir_at(FdCount& fds, int root, const std::vector<std::string>& comps) {
  DirFd d;
  d.fd = root;
  for (const std::string& c : comps) {
    const int nfd =
        fds.took(::openat(d.fd, c.c_str(), O_RDONLY | O_DIRECTORY | O_NOFOLLOW | O_CLOEXEC));
    const int e = errno;
    if (d.own) fds.close(d.fd);
    if (nfd < 0) {
      d.fd = -1;
      d.own = false;
      d.err = e;
      return d;
    }
    d.fd = nfd;
    d.own = true;
  }
  return d;
}

DirFd open_dir(Image& im, const std::vector<std::string>& comps) {
  return open_dir_at(im.fds, im.root, comps);
}

void close_dir_at(FdCount& fds, DirFd& d) {
  if (d.own) fds.close(d.fd);
  d = DirFd();
}

void close_dir(Image& im, DirFd& d) { close_dir_at(im.fds, d); }

// What the packer saw of a file it is about to pack.
struct Seen {
  dev_t dev = 0;
  ino_t ino = 0;
};

// openat + fstat of a listed non-empty file: 0 with *fd_out open, or the
// failure's kind with *err.  (O_NONBLOCK: a fifo in the file's place fails
// the fstat test below instead of blocking the open.)
int open_listed_at(FdCount& fds, const DirFd& d, const Item& it, int* fd_out, struct stat* st,
                   int* err) {
  *fd_out = -1;
  *err = 0;
  if (d.fd < 0) {
    *err = d.err;
    return CIR_CHECK_READ;
  }
  const int fd = fds.took(
      ::openat(d.fd, it.name.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC | O_NONBLOCK));
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

int open_listed(Image& im, const DirFd& d, const Item& it, int* fd_out, struct stat* st, int* err) {
  return open_listed_at(im.fds, d, it, fd_out, st, err);
}

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
  const int kind = open_listed(im, d, it, &fd, &st, err);
  if (kind) return kind;
  im.fds.close(fd);
  if ((uint64_t)st.st_size != it.size) return CIR_CHECK_CHECKSUM;
  seen->dev = st.st_dev;
  seen->ino = st.st_ino;
  return CIR_CHECK_OK;
}

struct ReadJob {
  size_t item;
  Seen seen;
  uint64_t file_off, len;
  uint8_t* dst;
  uint64_t seg_blk;  // the batch's block index where this item's segment starts
  uint64_t seg_pos;  // and its byte offset in the slot
};

// Read the batch's jobs on `threads` readers.  Returns the index of the first
// job (in job order, whatever the timing: a reader skips only jobs after a
// failed one) that failed, with its errno, or jobs.size().
size_t run_reads(Image& im, const std::vector<ReadJob>& jobs, unsigned threads, int* err_out) {
  std::atomic<size_t> next{0}, first_bad{jobs.size()};
  std::mutex mu;
  int first_err = 0;
  const bool nt = stage_copy_nt();
  auto worker = [&] {
    DirFd d;  // this reader's directory, kept across the jobs that share it
    size_t d_dir = SIZE_MAX;
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= jobs.size() || i > first_bad.load()) break;
      const ReadJob& j = jobs[i];
      const Item& it = im.items[j.item];
      if (d_dir != it.dir) {
        close_dir(im, d);
        d = open_dir(im, im.dirs[it.dir]);
        d_dir = it.dir;
      }
      int fd = -1, e = 0;
      struct stat st;
      bool ok = open_listed(im, d, it, &fd, &st, &e) == CIR_CHECK_OK;
      if (ok && (st.st_dev != j.seen.dev || st.st_ino != j.seen.ino ||
                 (uint64_t)st.st_size != it.size)) {
        ok = false;  // not the file that was packed
        e = ESTALE;
      }
      uint64_t got = 0;
      while (ok && got < j.len) {
        const ssize_t r =
            pread_staged(fd, j.dst + got, j.len - got, (off_t)(j.file_off + got), nt);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          ok = false;
          e = r == 0 ? ENODATA : errno;  // the file shrank under the read
          break;
        }
        got += (uint64_t)r;
      }
      im.fds.close(fd);
      if (!ok) {
        std::lock_guard<std::mutex> lk(mu);
        if (i < first_bad.load()) {
          first_bad.store(i);
          first_err = e;
        }
      }
    }
    close_dir(im, d);
  };
  parallel_run(std::max(1u, std::min<unsigned>(threads, (unsigned)jobs.size())), worker);
  *err_out = first_err;
  return first_bad.load();
}

using BlockRanges = std::vector<std::pair<uint64_t, uint64_t>>;

// hash_range (scan.cpp) in check mode: the block ranges `ranges` (increasing)
// on device d, with the entries each range owns -- those whose first block
// lies in it, the trailing empty files with the last range -- examined in
// order as the packer reaches them.  Every failure goes to im.report().
int check_range(cir_ctx* ctx, Device& d, Image& im, unsigned threads, const BlockRanges& ranges) {
  if (ranges.empty()) return CIR_OK;
  std::lock_guard<std::mutex> lk(d.mu);
  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d.id));
  SlotDrain drain{d};  // an early return leaves no slot busy
  const std::vector<Item>& items = im.items;
  const uint64_t bs = im.bs;
  uint64_t seg = 0;
  for (const Item& it : items) seg = std::max(seg, std::min<uint64_t>(it.size, bs));
  const uint64_t cap = (std::max<uint64_t>(ctx->staging, seg + 16) + 15) & ~15ull;
  const uint64_t cap_blk = std::max<uint64_t>(cap / 512, 4096);
  uint64_t fill = scan_ramp() ? std::max<uint64_t>(seg + 16, cap >> 3) : cap;

  size_t ri = 0;
  uint64_t b0 = 0, b1 = 0;
  size_t ii = 0;           // the item being packed
  uint64_t fblk = 0;       // its next block
  size_t examined = SIZE_MAX;  // the item whose host-side look passed (in this range)
  Seen seen;
  bool stopped = false;    // nothing further is packed
  DirFd cur;               // the packer's directory
  size_t cur_dir = SIZE_MAX;
  struct CloseCur {
    Image& im;
    DirFd& d;
    ~CloseCur() { close_dir(im, d); }
  } close_cur{im, cur};
  auto dir_of = [&](const Item& it) -> const DirFd& {
    if (cur_dir != it.dir) {
      close_dir(im, cur);
      cur = open_dir(im, im.dirs[it.dir]);
      cur_dir = it.dir;
    }
    return cur;
  };
  auto start_range = [&](size_t r) {
    ri = r;
    b0 = ranges[r].first;
    b1 = ranges[r].second;
    // the first item at or past b0, or the file b0 falls inside
    ii = std::lower_bound(items.begin(), items.end(), b0,
                          [](const Item& x, uint64_t b) { return x.first_blk < b; }) -
         items.begin();
    fblk = 0;
    if (ii > 0 && items[ii - 1].first_blk + items[ii - 1].nblk > b0) {
      --ii;
      fblk = b0 - items[ii].first_blk;
    }
    examined = SIZE_MAX;
  };
  // is items[ii] (from block fblk on) this range's to look at?
  auto here = [&] {
    if (ii >= items.size()) return false;
    const uint64_t at = items[ii].first_blk + fblk;
    return at < b1 || (b1 == im.nblk_total && at == b1 && items[ii].nblk == 0);
  };
  auto more = [&] {
    if (stopped) return false;
    while (!here()) {
      if (ri + 1 >= ranges.size()) return false;
      start_range(ri + 1);
    }
    return true;
  };
  auto busy = [&] {
    for (const Slot& s : d.slot)
      if (s.busy) return true;
    return false;
  };
  auto fail_here = [&](int kind, int err) {
    Failure f;
    f.item = ii;
    f.blk = items[ii].first_blk + fblk;
    f.kind = kind;
    f.err = err;
    im.report(f);
    stopped = true;
  };
  start_range(0);
  constexpr int kS = Device::kSlots;
  int k = 0;
  while (more() || busy()) {
    Slot& s = d.slot[k];
    if (s.busy) {
      int rc = slot_wait(d, s);
      if (rc) return rc;
      const uint64_t first = s.h_cell[0];
      if (first != kNone) {
        Failure f;
        f.item = im.item_of(first);
        f.blk = first;
        f.kind = CIR_CHECK_CHECKSUM;
        f.bad_blk = first;
        im.report(f);
        stopped = true;  // what is still in flight lies above it and is only drained
      }
    }
    // (another device's failure below everything left here ends this one)
    if (more() && im.decided_before(ii, items[ii].first_blk + fblk)) stopped = true;
    if (more()) {
      int rc = d.ensure_slot(s, cap, cap_blk);
      if (rc) return rc;
      rc = d.ensure_check(s);
      if (rc) return rc;
      std::vector<ReadJob> jobs;
      uint64_t pos = 0, n = 0, used = 0;
      const uint64_t first = items[ii].first_blk + fblk;
      uint64_t new_files = 0, file_bytes = 0;
      while (!stopped && here() && n < cap_blk) {
        const Item& it = items[ii];
        const DirFd& dfd = dir_of(it);
        if (it.nblk == 0) {
          int err = 0;
          const int kind = examine_empty(dfd, it, &err);
          if (kind) {
            fail_here(kind, err);
            break;
          }
          im.n_empty.fetch_add(1);
          ++ii;
          continue;
        }
        if (examined != ii) {
          int err = 0;
          const int kind = examine_file(im, dfd, it, &seen, &err);
          if (kind) {
            fail_here(kind, err);
            break;
          }
          examined = ii;
        }
        const uint64_t left_blk = std::min<uint64_t>(it.nblk - fblk, b1 - (it.first_blk + fblk));
        pos = (pos + 15) & ~15ull;
        if (pos + std::min<uint64_t>(bs, it.size - fblk * bs) > fill) break;
        uint64_t take = std::min<uint64_t>(left_blk, cap_blk - n);
        take = std::min<uint64_t>(take, std::max<uint64_t>((fill - pos) / bs, 1));
        const uint64_t off0 = fblk * bs;
        const uint64_t bytes = std::min<uint64_t>(take * bs, it.size - off0);
        if (pos + bytes > fill) break;
        for (uint64_t j = 0; j < take; ++j) {
          s.h_off[n + j] = pos + j * bs;
          s.h_len[n + j] = (uint32_t)std::min<uint64_t>(bs, it.size - off0 - j * bs);
        }
        // the index's digests of these blocks, in block order (nothing comes
        // back through h_out in this mode: it carries them up)
        memcpy(s.h_out + 32 * n, im.idx->entries[it.entry].hashes.data() + 32 * fblk, 32 * take);
        for (uint64_t piece = 0; piece < bytes; piece += kReadPiece)
          jobs.push_back({ii, seen, off0 + piece, std::min<uint64_t>(kReadPiece, bytes - piece),
                          s.h_data + pos + piece, n, pos});
        if (fblk == 0) ++new_files;
        file_bytes += bytes;
        pos += bytes;
        used = pos;
        n += take;
        fblk += take;
        if (fblk == it.nblk) {
          ++ii;
          fblk = 0;
        }
      }
      fill = std::min(cap, fill * 2);
      if (n > 0) {
        int rerr = 0;
        const size_t bad = run_reads(im, jobs, threads, &rerr);
        if (bad < jobs.size()) {
          // READ at that file: the batch keeps the blocks before its segment
          // (any of them may still be the verdict), nothing further is packed
          const ReadJob& j = jobs[bad];
          Failure f;
          f.item = j.item;
          f.blk = first + j.seg_blk;
          f.kind = CIR_CHECK_READ;
          f.err = rerr;
          im.report(f);
          stopped = true;
          n = j.seg_blk;
          used = j.seg_pos;
        }
      }
      if (n > 0) {
        rc = slot_submit_check(d, s, std::max<uint64_t>(used, 16), n, im.ht, first);
        if (rc) return rc;
        im.n_files.fetch_add(new_files);
        im.n_blocks.fetch_add(n);
        im.n_bytes.fetch_add(file_bytes);
        im.n_batches.fetch_add(1);
      }
    }
    k = (k + 1) % kS;
  }
  return CIR_OK;
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
  dirsig::Index idx;
  std::string err;
  if (!dirsig::parse(index, len, &idx, &err))
    return idx.bad_hash_size ? fail(CIR_EHASHSIZE, "hash size is unsupported: " + err)
                             : fail(CIR_EPARSE, "error parsing index: " + err);
  if (dirsig::digest_len(idx.header.hash) != 32)
    return fail(CIR_EHASHSIZE, "hash size is unsupported");
  if (idx.header.block_size > 0xffffffffull)
    return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  Image im;
  im.idx = &idx;
  im.bs = idx.header.block_size;
  im.ht = idx.header.hash == dirsig::HashType::kSha512_256 ? CIR_HASH_SHA512_256
                                                            : CIR_HASH_BLAKE2B_256;
  // the entries' places: directory lines as components, files with the
  // global index of their first block
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
      im.dirs.push_back(std::move(comps));
    } else if (en.kind == dirsig::EntryKind::kFile) {
      if (im.dirs.empty()) return fail(CIR_EPARSE, "error parsing index: entry before a directory");
      Item it;
      it.entry = e;
      it.dir = im.dirs.size() - 1;
      it.name = en.path.substr(en.path.rfind('/') + 1);
      it.size = en.size;
      it.nblk = en.hashes.size() / 32;
      it.first_blk = im.nblk_total;
      im.nblk_total += it.nblk;
      im.items.push_back(std::move(it));
    }
    // symlink entries are the caller's to create (commit.rs:118-126)
  }
  struct CloseRoot {
    Image& im;
    bool own = false;
    ~CloseRoot() {
      if (own) im.fds.close(im.root);
    }
  } close_root{im};
  if (dir) {
    im.root = im.fds.took(::openat(dirfd, dir, O_RDONLY | O_DIRECTORY | O_CLOEXEC));
    if (im.root < 0)
      return fail(CIR_EIO, std::string("error opening image ") + dir + ": " + strerror(errno));
    close_root.own = true;
  } else {
    struct stat st;
    if (::fstat(dirfd, &st) != 0 || !S_ISDIR(st.st_mode))
      return fail(CIR_EIO, "image root fd is not a directory");
    im.root = dirfd;
  }
  if (threads == 0) threads = host_copy_threads(ctx->devs.size());

  int rc = CIR_OK;
  const size_t nd = std::min<size_t>(ctx->devs.size(), (size_t)std::max<uint64_t>(im.nblk_total, 1));
  if (im.nblk_total == 0) {
    // only size-0 entries (or none): nothing for a device
    DirFd cur;
    size_t cur_dir = SIZE_MAX;
    for (size_t i = 0; i < im.items.size(); ++i) {
      const Item& it = im.items[i];
      if (cur_dir != it.dir) {
        close_dir(im, cur);
        cur = open_dir(im, im.dirs[it.dir]);
        cur_dir = it.dir;
      }
      int e = 0;
      const int kind = examine_empty(cur, it, &e);
      if (kind) {
        Failure f;
        f.item = i;
        f.blk = 0;
        f.kind = kind;
        f.err = e;
        im.report(f);
        break;
      }
      im.n_empty.fetch_add(1);
    }
    close_dir(im, cur);
  } else if (nd <= 1) {
    rc = check_range(ctx, *ctx->devs[0], im, threads, {{0, im.nblk_total}});
  } else {
    uint64_t stripe = std::max<uint64_t>(1, ctx->staging / im.bs);
    if (const char* e = getenv("CIR_DEBUG_STRIPE_BLOCKS"))  // tests: stripes of a few blocks
      if (atoll(e) > 0) stripe = (uint64_t)atoll(e);
    const StripePrefix order(im.nblk_total, stripe);
    std::vector<BlockRanges> dev_ranges(nd);
    for (size_t st = 0; st < order.stripes(); ++st)
      dev_ranges[st % nd].push_back({st * stripe, st * stripe + order.stripe_len(st)});
    const unsigned per = std::max(1u, threads / (unsigned)nd);
    std::vector<int> rcs(nd, 0);
    std::vector<std::string> errs(nd);
    fan_out(nd, [&](size_t i) {
      rcs[i] = check_range(ctx, *ctx->devs[i], im, per, dev_ranges[i]);
      if (rcs[i]) errs[i] = cir_last_error();
    });
    for (size_t i = 0; i < nd && !rc; ++i)
      if (rcs[i]) rc = fail(rcs[i], errs[i]);
  }
  stats[5] = im.fds.peak.load();
  if (rc) return rc;
  const Failure& f = im.best;
  if (f.kind != CIR_CHECK_OK) {
    const std::string& p = idx.entries[im.items[f.item].entry].path;
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

struct Cand {
  size_t item = 0;         // index into Links::items
  uint32_t src = 0;        // source root
  size_t out = 0;          // the caller's candidate number
  uint64_t first_blk = 0;  // global index of block 0 in the work order
};

struct Links {
  const dirsig::Index* idx = nullptr;
  uint64_t bs = 0;
  int ht = CIR_HASH_BLAKE2B_256;
  std::vector<std::vector<std::string>> dirs;
  std::vector<Item> items;  // every file entry, in index order
  std::vector<int> root;    // per source: its fd, or -1 with root_err
  std::vector<int> root_err;
  std::vector<Cand> cands;  // the non-empty candidates below a root that opened, in work order
  uint64_t nblk_total = 0;
  FdCount fds;
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
  bool exe(const Item& it) const { return idx->entries[it.entry].exe; }
};

// A directory of one source root, kept while the next candidate needs the same.
struct LinkDir {
  DirFd d;
  uint32_t src = UINT32_MAX;
  size_t dir = SIZE_MAX;
  const DirFd& of(Links& L, const Cand& c) {
    const Item& it = L.items[c.item];
    if (src != c.src || dir != it.dir) {
      close_dir_at(L.fds, d);
      d = open_dir_at(L.fds, L.root[c.src], L.dirs[it.dir]);
      src = c.src;
      dir = it.dir;
    }
    return d;
  }
  void close(Links& L) {
    close_dir_at(L.fds, d);
    src = UINT32_MAX;
    dir = SIZE_MAX;
  }
};

// The packer's look at a candidate (try_hardlink without the read): READ,
// CHECKSUM on a length or mode bits (public.rs:331-338) that are not the
// entry's, else what identifies the file to the readers.
int examine_link(Links& L, const DirFd& d, const Item& it, Seen* seen, int* err) {
  int fd = -1;
  struct stat st;
  const int kind = open_listed_at(L.fds, d, it, &fd, &st, err);
  if (kind) return kind;
  L.fds.close(fd);
  if ((uint64_t)st.st_size != it.size) return CIR_CHECK_CHECKSUM;
  if ((st.st_mode & 0777) != (L.exe(it) ? 0755u : 0644u)) return CIR_CHECK_CHECKSUM;
  seen->dev = st.st_dev;
  seen->ino = st.st_ino;
  return CIR_CHECK_OK;
}

struct LinkJob {
  size_t cand;  // index into Links::cands
  Seen seen;
  uint64_t file_off, len;
  uint8_t* dst;
};

// Read the batch's jobs on `threads` readers.  Every job is tried; a failed
// one makes READ of its own candidate and of nothing else (its bytes in the
// slot are then whatever they are: READ wins over what the compare finds).
void run_link_reads(Links& L, const std::vector<LinkJob>& jobs, unsigned threads) {
  std::atomic<size_t> next{0};
  const bool nt = stage_copy_nt();
  auto worker = [&] {
    LinkDir dir;
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= jobs.size()) break;
      const LinkJob& j = jobs[i];
      const Cand& c = L.cands[j.cand];
      const Item& it = L.items[c.item];
      int fd = -1, e = 0;
      struct stat st;
      bool ok = open_listed_at(L.fds, dir.of(L, c), it, &fd, &st, &e) == CIR_CHECK_OK;
      if (ok && (st.st_dev != j.seen.dev || st.st_ino != j.seen.ino ||
                 (uint64_t)st.st_size != it.size)) {
        ok = false;  // not the file that was packed
        e = ESTALE;
      }
      uint64_t got = 0;
      while (ok && got < j.len) {
        const ssize_t r =
            pread_staged(fd, j.dst + got, j.len - got, (off_t)(j.file_off + got), nt);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          ok = false;
          e = r == 0 ? ENODATA : errno;  // the file shrank under the read
          break;
        }
        got += (uint64_t)r;
      }
      L.fds.close(fd);
      if (!ok) L.report(c.out, CIR_CHECK_READ, e);
    }
    dir.close(L);
  };
  parallel_run(std::max(1u, std::min<unsigned>(threads, (unsigned)jobs.size())), worker);
}

// check_range for the candidates: the block ranges `ranges` (increasing, of
// the work order's global blocks) on device d.  A candidate is examined by
// every range that holds some of its blocks; what fails the look is reported
// and its blocks in the range are passed over.
int links_range(cir_ctx* ctx, Device& d, Links& L, unsigned threads, const BlockRanges& ranges) {
  if (ranges.empty()) return CIR_OK;
  std::lock_guard<std::mutex> lk(d.mu);
  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d.id));
  SlotDrain drain{d};  // an early return leaves no slot busy
  const std::vector<Cand>& cands = L.cands;
  const uint64_t bs = L.bs;
  uint64_t seg = 0;
  for (const Cand& c : cands) seg = std::max(seg, std::min<uint64_t>(L.items[c.item].size, bs));
  const uint64_t cap = (std::max<uint64_t>(ctx->staging, seg + 16) + 15) & ~15ull;
  const uint64_t cap_blk = std::max<uint64_t>(cap / 512, 4096);
  uint64_t fill = scan_ramp() ? std::max<uint64_t>(seg + 16, cap >> 3) : cap;

  size_t ri = 0;
  uint64_t b0 = 0, b1 = 0;
  size_t ci = 0;               // the candidate being packed
  uint64_t fblk = 0;           // its next block
  size_t examined = SIZE_MAX;  // the candidate whose look passed (in this range)
  Seen seen;
  LinkDir cur;  // the packer's directory
  struct CloseCur {
    Links& L;
    LinkDir& d;
    ~CloseCur() { d.close(L); }
  } close_cur{L, cur};
  constexpr int kS = Device::kSlots;
  std::vector<size_t> seg_cand[kS];  // per slot in flight: each segment's candidate (Cand::out)
  auto start_range = [&](size_t r) {
    ri = r;
    b0 = ranges[r].first;
    b1 = ranges[r].second;
    ci = std::lower_bound(cands.begin(), cands.end(), b0,
                          [](const Cand& x, uint64_t b) { return x.first_blk < b; }) -
         cands.begin();
    fblk = 0;
    if (ci > 0 && cands[ci - 1].first_blk + L.items[cands[ci - 1].item].nblk > b0) {
      --ci;
      fblk = b0 - cands[ci].first_blk;
    }
    examined = SIZE_MAX;
  };
  auto here = [&] { return ci < cands.size() && cands[ci].first_blk + fblk < b1; };
  auto more = [&] {
    while (!here()) {
      if (ri + 1 >= ranges.size()) return false;
      start_range(ri + 1);
    }
    return true;
  };
  auto busy = [&] {
    for (const Slot& s : d.slot)
      if (s.busy) return true;
    return false;
  };
  start_range(0);
  // CIR_TRACE: where this device's host thread spent the call
  const bool trace = trace_enabled();
  using Clock = std::chrono::steady_clock;
  double t_wait = 0, t_pack = 0, t_read = 0, t_submit = 0;
  uint64_t n_batches = 0;
  auto lap = [&](Clock::time_point& t0, double& acc) {
    if (!trace) return;
    const Clock::time_point t1 = Clock::now();
    acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  };
  int k = 0;
  while (more() || busy()) {
    Slot& s = d.slot[k];
    Clock::time_point t0 = trace ? Clock::now() : Clock::time_point();
    if (s.busy) {
      int rc = slot_wait(d, s);
      if (rc) return rc;
      uint32_t nbad = 0;
      memcpy(&nbad, s.h_seg_res, 4);
      if (nbad) {
        const uint8_t* flags = s.h_seg_res + kSegResHead;
        for (size_t g = 0; g < seg_cand[k].size(); ++g)
          if (flags[g]) L.report(seg_cand[k][g], CIR_CHECK_CHECKSUM, 0);
      }
    }
    lap(t0, t_wait);
    if (more()) {
      int rc = d.ensure_slot(s, cap, cap_blk);
      if (rc) return rc;
      rc = d.ensure_links(s);
      if (rc) return rc;
      std::vector<LinkJob> jobs;
      std::vector<size_t>& segs = seg_cand[k];
      segs.clear();
      uint64_t pos = 0, n = 0, used = 0, file_bytes = 0;
      while (here() && n < cap_blk) {
        const Cand& c = cands[ci];
        const Item& it = L.items[c.item];
        const uint64_t left_blk = std::min<uint64_t>(it.nblk - fblk, b1 - (c.first_blk + fblk));
        if (examined != ci) {
          int err = 0;
          const int kind = examine_link(L, cur.of(L, c), it, &seen, &err);
          if (kind) {
            L.report(c.out, kind, err);
            fblk += left_blk;  // its blocks in this range are passed over
            if (fblk == it.nblk) {
              ++ci;
              fblk = 0;
            }
            continue;
          }
          examined = ci;
        }
        pos = (pos + 15) & ~15ull;
        if (pos + std::min<uint64_t>(bs, it.size - fblk * bs) > fill) break;
        uint64_t take = std::min<uint64_t>(left_blk, cap_blk - n);
        take = std::min<uint64_t>(take, std::max<uint64_t>((fill - pos) / bs, 1));
        const uint64_t off0 = fblk * bs;
        const uint64_t bytes = std::min<uint64_t>(take * bs, it.size - off0);
        if (pos + bytes > fill) break;
        for (uint64_t j = 0; j < take; ++j) {
          s.h_off[n + j] = pos + j * bs;
          s.h_len[n + j] = (uint32_t)std::min<uint64_t>(bs, it.size - off0 - j * bs);
        }
        // the entry's digests of these blocks travel up through h_out
        memcpy(s.h_out + 32 * n, L.idx->entries[it.entry].hashes.data() + 32 * fblk, 32 * take);
        for (uint64_t piece = 0; piece < bytes; piece += kReadPiece)
          jobs.push_back({ci, seen, off0 + piece, std::min<uint64_t>(kReadPiece, bytes - piece),
                          s.h_data + pos + piece});
        file_bytes += bytes;
        pos += bytes;
        used = pos;
        n += take;
        fblk += take;
        s.h_seg_end[segs.size()] = (uint32_t)n;  // (at most one segment per block: <= cap_blk)
        segs.push_back(c.out);
        if (fblk == it.nblk) {
          ++ci;
          fblk = 0;
        }
      }
      fill = std::min(cap, fill * 2);
      lap(t0, t_pack);
      if (n > 0) {
        run_link_reads(L, jobs, threads);
        lap(t0, t_read);
        rc = slot_submit_links(d, s, std::max<uint64_t>(used, 16), n, L.ht, segs.size());
        if (rc) return rc;
        lap(t0, t_submit);
        ++n_batches;
        L.n_blocks.fetch_add(n);
        L.n_bytes.fetch_add(file_bytes);
        L.n_batches.fetch_add(1);
      }
    }
    k = (k + 1) % kS;
  }
  if (trace)
    fprintf(stderr,
            "cir check_links dev %d: %llu batches; packer's look and segment table %.2f ms, "
            "reads %.2f ms, submit %.2f ms, waiting for results and flags %.2f ms\n",
            d.id, (unsigned long long)n_batches, t_pack, t_read, t_submit, t_wait);
  return CIR_OK;
}

int links_impl(cir_ctx* ctx, const uint8_t* index, size_t len, const int* src_dirfd,
               const char* const* src_dir, size_t nsrc, const uint64_t* link_file,
               const uint32_t* link_src, size_t nlinks, uint32_t threads, uint8_t* kind_out,
               int32_t* errno_out, uint64_t* stats) {
  if (!ctx || !index || !stats || (nsrc && (!src_dirfd || !src_dir)) ||
      (nlinks && (!link_file || !link_src || !kind_out)))
    return fail(CIR_EINVAL, "null pointer");
  for (int i = 0; i < CIR_LINKS_STATS_FIELDS; ++i) stats[i] = 0;
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  for (size_t i = 0; i < nlinks; ++i)
    if (link_src[i] >= nsrc) return fail(CIR_EINVAL, "link_src names no source root");
  dirsig::Index idx;
  std::string perr;
  if (!dirsig::parse(index, len, &idx, &perr))
    return idx.bad_hash_size ? fail(CIR_EHASHSIZE, "hash size is unsupported: " + perr)
                             : fail(CIR_EPARSE, "error parsing index: " + perr);
  if (dirsig::digest_len(idx.header.hash) != 32)
    return fail(CIR_EHASHSIZE, "hash size is unsupported");
  if (idx.header.block_size > 0xffffffffull)
    return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  Links L;
  L.idx = &idx;
  L.bs = idx.header.block_size;
  L.ht = idx.header.hash == dirsig::HashType::kSha512_256 ? CIR_HASH_SHA512_256
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
      L.dirs.push_back(std::move(comps));
    } else if (en.kind == dirsig::EntryKind::kFile) {
      if (L.dirs.empty()) return fail(CIR_EPARSE, "error parsing index: entry before a directory");
      Item it;
      it.entry = e;
      it.dir = L.dirs.size() - 1;
      it.name = en.path.substr(en.path.rfind('/') + 1);
      it.size = en.size;
      it.nblk = en.hashes.size() / 32;
      L.items.push_back(std::move(it));
    }
  }
  for (size_t i = 0; i < nlinks; ++i)
    if (link_file[i] >= L.items.size())
      return fail(CIR_EINVAL, "link_file is past the last file entry");
  // ---- nothing above touched a file or a device
  const double ms_parse = ms_since(t_start);
  const auto t_roots = std::chrono::steady_clock::now();
  std::vector<int32_t> errs(nlinks, 0);
  L.kind = kind_out;
  L.err = errs.data();
  for (size_t i = 0; i < nlinks; ++i) kind_out[i] = CIR_CHECK_OK;
  // the roots some candidate names
  L.root.assign(nsrc, -1);
  L.root_err.assign(nsrc, 0);
  std::vector<char> own(nsrc, 0), used(nsrc, 0);
  struct CloseRoots {
    Links& L;
    std::vector<char>& own;
    ~CloseRoots() {
      for (size_t j = 0; j < own.size(); ++j)
        if (own[j]) L.fds.close(L.root[j]);
    }
  } close_roots{L, own};
  for (size_t i = 0; i < nlinks; ++i) used[link_src[i]] = 1;
  for (size_t j = 0; j < nsrc; ++j) {
    if (!used[j]) continue;
    if (src_dir[j]) {
      L.root[j] = L.fds.took(::openat(src_dirfd[j], src_dir[j], O_RDONLY | O_DIRECTORY | O_CLOEXEC));
      if (L.root[j] < 0)
        L.root_err[j] = errno;
      else
        own[j] = 1;
    } else {
      struct stat st;
      if (::fstat(src_dirfd[j], &st) != 0)
        L.root_err[j] = errno;
      else if (!S_ISDIR(st.st_mode))
        L.root_err[j] = ENOTDIR;
      else
        L.root[j] = src_dirfd[j];
    }
  }
  // the work order: by root, then by index order
  std::vector<size_t> order(nlinks);
  for (size_t i = 0; i < nlinks; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return link_src[a] != link_src[b] ? link_src[a] < link_src[b] : link_file[a] < link_file[b];
  });
  {
    LinkDir cur;
    for (size_t i : order) {
      Cand c;
      c.item = (size_t)link_file[i];
      c.src = link_src[i];
      c.out = i;
      const Item& it = L.items[c.item];
      if (L.root[c.src] < 0) {
        L.report(i, CIR_CHECK_READ, L.root_err[c.src]);
      } else if (it.nblk == 0) {
        // a size-0 candidate: an empty regular file of the right mode, seen by the host alone
        Seen seen;
        int e = 0;
        const int kind = examine_link(L, cur.of(L, c), it, &seen, &e);
        if (kind) L.report(i, kind, e);
        ++stats[7];
      } else {
        c.first_blk = L.nblk_total;
        L.nblk_total += it.nblk;
        L.cands.push_back(c);
      }
    }
    cur.close(L);
  }
  if (threads == 0) threads = host_copy_threads(ctx->devs.size());
  const double ms_roots = ms_since(t_roots);
  const auto t_pipe = std::chrono::steady_clock::now();

  int rc = CIR_OK;
  const size_t nd = std::min<size_t>(ctx->devs.size(), (size_t)std::max<uint64_t>(L.nblk_total, 1));
  if (L.nblk_total == 0) {
    // nothing for a device
  } else if (nd <= 1) {
    rc = links_range(ctx, *ctx->devs[0], L, threads, {{0, L.nblk_total}});
  } else {
    uint64_t stripe = std::max<uint64_t>(1, ctx->staging / L.bs);
    if (const char* e = getenv("CIR_DEBUG_STRIPE_BLOCKS"))  // tests: stripes of a few blocks
      if (atoll(e) > 0) stripe = (uint64_t)atoll(e);
    const StripePrefix sp(L.nblk_total, stripe);
    std::vector<BlockRanges> dev_ranges(nd);
    for (size_t st = 0; st < sp.stripes(); ++st)
      dev_ranges[st % nd].push_back({st * stripe, st * stripe + sp.stripe_len(st)});
    const unsigned per = std::max(1u, threads / (unsigned)nd);
    std::vector<int> rcs(nd, 0);
    std::vector<std::string> es(nd);
    fan_out(nd, [&](size_t i) {
      rcs[i] = links_range(ctx, *ctx->devs[i], L, per, dev_ranges[i]);
      if (rcs[i]) es[i] = cir_last_error();
    });
    for (size_t i = 0; i < nd && !rc; ++i)
      if (rcs[i]) rc = fail(rcs[i], es[i]);
  }
  stats[6] = L.fds.peak.load();
  if (trace_enabled())
    fprintf(stderr,
            "cir check_links: %zu candidates; index parse %.2f ms, roots, work order and size-0 "
            "candidates %.2f ms, pipeline %.2f ms\n",
            nlinks, ms_parse, ms_roots, ms_since(t_pipe));
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

// What the looks and the reads found of a file.
constexpr uint8_t kLookAbsent = 1, kLookBlocked = 2, kLookShort = 4, kLookLong = 8;

struct Blocks {
  const dirsig::Index* idx = nullptr;
  uint64_t bs = 0;
  int ht = CIR_HASH_BLAKE2B_256;
  int root = -1;
  std::vector<std::vector<std::string>> dirs;
  std::vector<Item> items;   // every file entry, in index order
  std::vector<size_t> work;  // the non-empty ones (indices into items), in index order
  uint64_t nblk_total = 0;
  FdCount fds;
  std::mutex mu;
  // what the looks and the reads found of each file (kLook* bits), and the
  // errno of the first thing that blocked it
  std::vector<uint8_t> look;
  std::vector<int32_t> err;
  std::atomic<uint64_t> n_bytes{0}, n_batches{0}, n_unread{0};

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
  if (open_listed_at(B.fds, d, it, &fd, &st, &e) != CIR_CHECK_OK) {
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

struct BlockJob {
  size_t item;
  Seen seen;
  uint64_t seen_len;  // the file's length at the packer's look
  uint64_t file_off, len;
  uint8_t* dst;
};

// Read the batch's jobs on `threads` readers.  Every job is tried; a failed
// one blocks its own file and nothing else.
void run_block_reads(Blocks& B, const std::vector<BlockJob>& jobs, unsigned threads) {
  std::atomic<size_t> next{0};
  const bool nt = stage_copy_nt();
  auto worker = [&] {
    DirFd d;  // this reader's directory, kept across the jobs that share it
    size_t d_dir = SIZE_MAX;
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= jobs.size()) break;
      const BlockJob& j = jobs[i];
      const Item& it = B.items[j.item];
      if (d_dir != it.dir) {
        close_dir_at(B.fds, d);
        d = open_dir_at(B.fds, B.root, B.dirs[it.dir]);
        d_dir = it.dir;
      }
      int fd = -1, e = 0;
      struct stat st;
      bool ok = open_listed_at(B.fds, d, it, &fd, &st, &e) == CIR_CHECK_OK;
      if (ok && (st.st_dev != j.seen.dev || st.st_ino != j.seen.ino ||
                 (uint64_t)st.st_size < j.seen_len)) {
        ok = false;  // not the file that was packed, or it shrank
        e = ESTALE;
      }
      uint64_t got = 0;
      while (ok && got < j.len) {
        const ssize_t r =
            pread_staged(fd, j.dst + got, j.len - got, (off_t)(j.file_off + got), nt);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          ok = false;
          e = r == 0 ? ENODATA : errno;  // the file shrank under the read
          break;
        }
        got += (uint64_t)r;
      }
      B.fds.close(fd);
      if (!ok) B.report(j.item, kLookBlocked, e);
    }
    close_dir_at(B.fds, d);
  };
  parallel_run(std::max(1u, std::min<unsigned>(threads, (unsigned)jobs.size())), worker);
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
  if (ranges.empty()) return CIR_OK;
  std::lock_guard<std::mutex> lk(d.mu);
  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d.id));
  SlotDrain drain{d};  // an early return leaves no slot busy
  const std::vector<size_t>& work = B.work;
  const uint64_t bs = B.bs;
  uint64_t seg = 0;
  for (size_t w : work) seg = std::max(seg, std::min<uint64_t>(B.items[w].size, bs));
  const uint64_t cap = (std::max<uint64_t>(ctx->staging, seg + 16) + 15) & ~15ull;
  const uint64_t cap_blk = std::max<uint64_t>(cap / 512, 4096);
  uint64_t fill = scan_ramp() ? std::max<uint64_t>(seg + 16, cap >> 3) : cap;

  size_t ri = 0;
  uint64_t b0 = 0, b1 = 0;
  size_t wi = 0;               // the file being packed (index into work)
  uint64_t fblk = 0;           // its next block
  size_t examined = SIZE_MAX;  // the file whose look passed (in this range)
  Seen seen;
  uint64_t cur_len = 0;        // its length at that look
  DirFd cur;                   // the packer's directory
  size_t cur_dir = SIZE_MAX;
  struct CloseCur {
    Blocks& B;
    DirFd& d;
    ~CloseCur() { close_dir_at(B.fds, d); }
  } close_cur{B, cur};
  auto dir_of = [&](const Item& it) -> const DirFd& {
    if (cur_dir != it.dir) {
      close_dir_at(B.fds, cur);
      cur = open_dir_at(B.fds, B.root, B.dirs[it.dir]);
      cur_dir = it.dir;
    }
    return cur;
  };
  constexpr int kS = Device::kSlots;
  std::vector<BitRun> runs[kS];  // per slot in flight
  auto start_range = [&](size_t r) {
    ri = r;
    b0 = ranges[r].first;
    b1 = ranges[r].second;
    wi = std::lower_bound(work.begin(), work.end(), b0,
                          [&](size_t x, uint64_t b) { return B.items[x].first_blk < b; }) -
         work.begin();
    fblk = 0;
    if (wi > 0 && B.items[work[wi - 1]].first_blk + B.items[work[wi - 1]].nblk > b0) {
      --wi;
      fblk = b0 - B.items[work[wi]].first_blk;
    }
    examined = SIZE_MAX;
  };
  auto here = [&] { return wi < work.size() && B.items[work[wi]].first_blk + fblk < b1; };
  auto more = [&] {
    while (!here()) {
      if (ri + 1 >= ranges.size()) return false;
      start_range(ri + 1);
    }
    return true;
  };
  auto busy = [&] {
    for (const Slot& s : d.slot)
      if (s.busy) return true;
    return false;
  };
  start_range(0);
  // CIR_TRACE: where this device's host thread spent the call
  const bool trace = trace_enabled();
  using Clock = std::chrono::steady_clock;
  double t_wait = 0, t_pack = 0, t_read = 0, t_submit = 0;
  uint64_t n_batches = 0;
  auto lap = [&](Clock::time_point& t0, double& acc) {
    if (!trace) return;
    const Clock::time_point t1 = Clock::now();
    acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  };
  int k = 0;
  while (more() || busy()) {
    Slot& s = d.slot[k];
    Clock::time_point t0 = trace ? Clock::now() : Clock::time_point();
    if (s.busy) {
      int rc = slot_wait(d, s);
      if (rc) return rc;
      const uint64_t* bits = reinterpret_cast<const uint64_t*>(s.h_bits + kBitsResHead);
      for (const BitRun& r : runs[k]) copy_bits(have, r.global, bits, r.at, r.count);
    }
    lap(t0, t_wait);
    if (more()) {
      int rc = d.ensure_slot(s, cap, cap_blk);
      if (rc) return rc;
      rc = d.ensure_blocks(s);
      if (rc) return rc;
      std::vector<BlockJob> jobs;
      std::vector<BitRun>& rs = runs[k];
      rs.clear();
      uint64_t pos = 0, n = 0, used = 0, file_bytes = 0;
      while (here() && n < cap_blk) {
        const size_t item = work[wi];
        const Item& it = B.items[item];
        const uint64_t in_range = std::min<uint64_t>(it.nblk - fblk, b1 - (it.first_blk + fblk));
        // its blocks in this range are passed over (their bits stay 0)
        auto pass_over = [&] {
          B.n_unread.fetch_add(in_range);
          fblk += in_range;
          if (fblk == it.nblk) {
            ++wi;
            fblk = 0;
          }
        };
        if (examined != wi) {
          if (!examine_block_file(B, dir_of(it), item, &seen, &cur_len)) {
            pass_over();
            continue;
          }
          examined = wi;
        }
        // the blocks that lie wholly inside the length the packer saw
        const uint64_t avail = cur_len >= it.size ? it.nblk : cur_len / bs;
        if (fblk >= avail) {
          pass_over();
          continue;
        }
        const uint64_t left_blk = std::min<uint64_t>(avail - fblk, in_range);
        pos = (pos + 15) & ~15ull;
        if (pos + std::min<uint64_t>(bs, it.size - fblk * bs) > fill) break;
        uint64_t take = std::min<uint64_t>(left_blk, cap_blk - n);
        take = std::min<uint64_t>(take, std::max<uint64_t>((fill - pos) / bs, 1));
        const uint64_t off0 = fblk * bs;
        const uint64_t bytes = std::min<uint64_t>(take * bs, it.size - off0);
        if (pos + bytes > fill) break;
        for (uint64_t j = 0; j < take; ++j) {
          s.h_off[n + j] = pos + j * bs;
          s.h_len[n + j] = (uint32_t)std::min<uint64_t>(bs, it.size - off0 - j * bs);
        }
        // the entry's digests of these blocks travel up through h_out
        memcpy(s.h_out + 32 * n, B.idx->entries[it.entry].hashes.data() + 32 * fblk, 32 * take);
        for (uint64_t piece = 0; piece < bytes; piece += kReadPiece)
          jobs.push_back({item, seen, cur_len, off0 + piece,
                          std::min<uint64_t>(kReadPiece, bytes - piece), s.h_data + pos + piece});
        if (!rs.empty() && rs.back().at + rs.back().count == n &&
            rs.back().global + rs.back().count == it.first_blk + fblk)
          rs.back().count += take;  // (neighbouring files, both complete: one run)
        else
          rs.push_back({n, it.first_blk + fblk, take});
        file_bytes += bytes;
        pos += bytes;
        used = pos;
        n += take;
        fblk += take;
        if (fblk == it.nblk) {
          ++wi;
          fblk = 0;
        }
      }
      fill = std::min(cap, fill * 2);
      lap(t0, t_pack);
      if (n > 0) {
        run_block_reads(B, jobs, threads);
        lap(t0, t_read);
        rc = slot_submit_blocks(d, s, std::max<uint64_t>(used, 16), n, B.ht);
        if (rc) return rc;
        lap(t0, t_submit);
        ++n_batches;
        B.n_bytes.fetch_add(file_bytes);
        B.n_batches.fetch_add(1);
      }
    }
    k = (k + 1) % kS;
  }
  if (trace)
    fprintf(stderr,
            "cir check_blocks dev %d: %llu batches; packer's look and run table %.2f ms, "
            "reads %.2f ms, submit %.2f ms, waiting for results and bit runs %.2f ms\n",
            d.id, (unsigned long long)n_batches, t_pack, t_read, t_submit, t_wait);
  return CIR_OK;
}

int blocks_impl(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                uint32_t threads, uint64_t** have_out, uint64_t* nblk_out, uint8_t** state_out,
                int32_t** errno_out, size_t* nfiles_out, uint64_t* stats) {
  if (!ctx || !index || !have_out || !nblk_out || !state_out || !nfiles_out || !stats)
    return fail(CIR_EINVAL, "null pointer");
  *have_out = nullptr;
  *nblk_out = 0;
  *state_out = nullptr;
  if (errno_out) *errno_out = nullptr;
  *nfiles_out = 0;
  for (int i = 0; i < CIR_BLOCKS_STATS_FIELDS; ++i) stats[i] = 0;
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  dirsig::Index idx;
  std::string perr;
  if (!dirsig::parse(index, len, &idx, &perr))
    return idx.bad_hash_size ? fail(CIR_EHASHSIZE, "hash size is unsupported: " + perr)
                             : fail(CIR_EPARSE, "error parsing index: " + perr);
  if (dirsig::digest_len(idx.header.hash) != 32)
    return fail(CIR_EHASHSIZE, "hash size is unsupported");
  if (idx.header.block_size > 0xffffffffull)
    return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  Blocks B;
  B.idx = &idx;
  B.bs = idx.header.block_size;
  B.ht = idx.header.hash == dirsig::HashType::kSha512_256 ? CIR_HASH_SHA512_256
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
      B.dirs.push_back(std::move(comps));
    } else if (en.kind == dirsig::EntryKind::kFile) {
      if (B.dirs.empty()) return fail(CIR_EPARSE, "error parsing index: entry before a directory");
      Item it;
      it.entry = e;
      it.dir = B.dirs.size() - 1;
      it.name = en.path.substr(en.path.rfind('/') + 1);
      it.size = en.size;
      it.nblk = en.hashes.size() / 32;
      it.first_blk = B.nblk_total;
      B.nblk_total += it.nblk;
      if (it.nblk) B.work.push_back(B.items.size());
      B.items.push_back(std::move(it));
    }
  }
  // ---- nothing above touched a file or a device
  const double ms_parse = ms_since(t_start);
  const auto t_empty = std::chrono::steady_clock::now();
  struct CloseRoot {
    Blocks& B;
    bool own = false;
    ~CloseRoot() {
      if (own) B.fds.close(B.root);
    }
  } close_root{B};
  if (dir) {
    B.root = B.fds.took(::openat(dirfd, dir, O_RDONLY | O_DIRECTORY | O_CLOEXEC));
    if (B.root < 0)
      return fail(CIR_EIO, std::string("error opening image ") + dir + ": " + strerror(errno));
    close_root.own = true;
  } else {
    struct stat st;
    if (::fstat(dirfd, &st) != 0 || !S_ISDIR(st.st_mode))
      return fail(CIR_EIO, "image root fd is not a directory");
    B.root = dirfd;
  }
  const size_t nfiles = B.items.size();
  const size_t nwords = (size_t)((B.nblk_total + 63) / 64);
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
    DirFd cur;
    size_t cur_dir = SIZE_MAX;
    for (size_t i = 0; i < nfiles; ++i) {
      const Item& it = B.items[i];
      if (it.nblk) continue;
      if (cur_dir != it.dir) {
        close_dir_at(B.fds, cur);
        cur = open_dir_at(B.fds, B.root, B.dirs[it.dir]);
        cur_dir = it.dir;
      }
      examine_block_empty(B, cur, i);
    }
    close_dir_at(B.fds, cur);
  }
  if (threads == 0) threads = host_copy_threads(ctx->devs.size());
  const double ms_empty = ms_since(t_empty);
  const auto t_pipe = std::chrono::steady_clock::now();

  int rc = CIR_OK;
  const size_t nd = std::min<size_t>(ctx->devs.size(), (size_t)std::max<uint64_t>(B.nblk_total, 1));
  if (B.nblk_total == 0) {
    // nothing for a device
  } else if (nd <= 1) {
    rc = blocks_range(ctx, *ctx->devs[0], B, threads, {{0, B.nblk_total}}, outs.have);
  } else {
    uint64_t stripe = std::max<uint64_t>(1, ctx->staging / B.bs);
    if (const char* e = getenv("CIR_DEBUG_STRIPE_BLOCKS"))  // tests: stripes of a few blocks
      if (atoll(e) > 0) stripe = (uint64_t)atoll(e);
    const StripePrefix sp(B.nblk_total, stripe);
    std::vector<BlockRanges> dev_ranges(nd);
    for (size_t st = 0; st < sp.stripes(); ++st)
      dev_ranges[st % nd].push_back({st * stripe, st * stripe + sp.stripe_len(st)});
    const unsigned per = std::max(1u, threads / (unsigned)nd);
    std::vector<int> rcs(nd, 0);
    std::vector<std::string> es(nd);
    // a bitmap per device (stripes do not end on word boundaries); device 0
    // writes into the result itself
    std::vector<std::vector<uint64_t>> part(nd);
    for (size_t i = 1; i < nd; ++i) part[i].assign(nwords, 0);
    fan_out(nd, [&](size_t i) {
      rcs[i] = blocks_range(ctx, *ctx->devs[i], B, per, dev_ranges[i],
                            i ? part[i].data() : outs.have);
      if (rcs[i]) es[i] = cir_last_error();
    });
    for (size_t i = 0; i < nd && !rc; ++i)
      if (rcs[i]) rc = fail(rcs[i], es[i]);
    for (size_t i = 1; i < nd; ++i)
      for (size_t w = 0; w < nwords; ++w) outs.have[w] |= part[i][w];
  }
  stats[8] = B.fds.peak.load();
  if (trace_enabled())
    fprintf(stderr,
            "cir check_blocks: %zu files, %llu blocks; index parse %.2f ms, root and size-0 "
            "entries %.2f ms, pipeline %.2f ms\n",
            nfiles, (unsigned long long)B.nblk_total, ms_parse, ms_empty, ms_since(t_pipe));
  if (rc) return rc;
  // the files' states.  A file that is absent or blocked has none of its
  // blocks: whatever a range packed of it before it went is cleared.
  for (size_t i = 0; i < nfiles; ++i) {
    const Item& it = B.items[i];
    const uint8_t lk = B.look[i];
    uint8_t st;
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

}  // namespace
}  // namespace cir

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
  return cir::links_impl(ctx, index, len, src_dirfd, src_dir, nsrc, link_file, link_src, nlinks,
                         threads, kind_out, errno_out, stats);
} CIR_CATCH_BOUNDARY

extern "C" int cir_check_index(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index,
                               size_t len, uint32_t threads, int* kind_out, uint8_t** path_out,
                               size_t* path_len, uint64_t stats[CIR_CHECK_STATS_FIELDS]) try {
  return cir::check_impl(ctx, dirfd, dir, index, len, threads, kind_out, path_out, path_len, stats);
} CIR_CATCH_BOUNDARY
