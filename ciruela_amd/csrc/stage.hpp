// What the staged pipelines over an image directory share (check.cpp's four
// entry points read one, store.cpp's cir_store_blocks writes one): the fds a
// call holds, the layout of an image as directories and file items, the image
// root, directories opened one component at a time and never through a
// symlink, the one-directory cache of a packer or a worker, the CIR_TRACE laps
// and the rotation over a device's staging slots.  Host only.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "dirsig.hpp"
#include "pack.hpp"
#include "runtime.hpp"

namespace cir {
namespace stage {

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
  size_t dir = 0;          // index into Layout::dirs
  std::string name;        // the entry's name in its directory
  uint64_t size = 0;
  uint64_t nblk = 0;
  uint64_t first_blk = 0;  // global index of block 0 (an empty file: the next file's)
};

using Dirs = std::vector<std::vector<std::string>>;

// What every entry point makes of its index before it touches a file.
struct Layout {
  dirsig::Index idx;
  uint64_t bs = 0;
  int ht = CIR_HASH_BLAKE2B_256;
  Dirs dirs;                // a directory line's components below the root
  std::vector<Item> items;  // every file entry, in index order
  uint64_t nblk_total = 0;
  FdCount fds;
  // an image root (open_image), closed with the layout when it is ours
  int root = -1;
  bool own_root = false;
  ~Layout() {
    if (own_root) fds.close(root);
  }
  const uint8_t* digests(const Item& it, uint64_t fblk) const {
    return idx.entries[it.entry].hashes.data() + 32 * fblk;
  }
};

// An image root by (dirfd, name-or-null): below dirfd by name (ours to
// close), or dirfd itself when it is a directory.  -1 with *err.
inline int open_root(FdCount& fds, int dirfd, const char* name, int* err) {
  *err = 0;
  if (name) {
    const int fd = fds.took(::openat(dirfd, name, O_RDONLY | O_DIRECTORY | O_CLOEXEC));
    if (fd < 0) *err = errno;
    return fd;
  }
  struct stat st;
  if (::fstat(dirfd, &st) != 0) {
    *err = errno;
    return -1;
  }
  if (!S_ISDIR(st.st_mode)) {
    *err = ENOTDIR;
    return -1;
  }
  return dirfd;
}

// The one root of cir_check_index and cir_check_blocks.
inline int open_image(Layout& t, int dirfd, const char* dir) {
  int e = 0;
  t.root = open_root(t.fds, dirfd, dir, &e);
  if (t.root >= 0) {
    t.own_root = dir != nullptr;
    return CIR_OK;
  }
  return dir ? fail(CIR_EIO, std::string("error opening image ") + dir + ": " + strerror(e))
             : fail(CIR_EIO, "image root fd is not a directory");
}

// A directory below the root, opened one component at a time, never through
// a symlink.  No components: the root fd itself (not ours to close).
struct DirFd {
  int fd = -1;
  bool own = false;
  int err = 0;  // errno when fd < 0
};

inline DirFd open_dir(FdCount& fds, int root, const std::vector<std::string>& comps) {
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

inline void close_dir(FdCount& fds, DirFd& d) {
  if (d.own) fds.close(d.fd);
  d = DirFd();
}

// The directory (of one root) a packer or a reader keeps while the next file
// needs the same one: at most one directory fd at a time.
class DirCache {
 public:
  explicit DirCache(Layout& t) : t_(t) {}
  ~DirCache() { close_dir(t_.fds, d_); }
  DirCache(const DirCache&) = delete;
  DirCache& operator=(const DirCache&) = delete;
  const DirFd& of(int root, size_t dir) {
    if (root_ != root || dir_ != dir) {
      close_dir(t_.fds, d_);
      d_ = open_dir(t_.fds, root, t_.dirs[dir]);
      root_ = root;
      dir_ = dir;
    }
    return d_;
  }

 private:
  Layout& t_;
  DirFd d_;
  int root_ = -1;
  size_t dir_ = SIZE_MAX;
};

// What the packer saw of a file it is about to pack.
struct Seen {
  dev_t dev = 0;
  ino_t ino = 0;
};

// CIR_TRACE: where a device's host thread spent a call.  (No clock is read
// when it is off.)
struct Laps {
  using Clock = std::chrono::steady_clock;
  const bool on;
  double wait = 0, pack = 0, read = 0, submit = 0;  // ms
  uint64_t batches = 0;
  Clock::time_point t0;
  explicit Laps(bool trace) : on(trace) {}
  void start() {
    if (on) t0 = Clock::now();
  }
  void lap(double& acc) {
    if (!on) return;
    const Clock::time_point t1 = Clock::now();
    acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// One pipeline on device d: its slots in turn, each waited for and retired
// (retire(k, slot)) when it is in flight, then -- while more() -- offered for
// packing: pack(k, slot) says whether it packed anything, read(k, slot) fills
// the slot and submit(k, slot) sends it (or not: what it submits it leaves
// busy).  `ensure` is the Device member that sizes the mode's own buffers of
// a slot.  Runs until nothing is left and nothing is in flight.
template <class More, class Retire, class Pack, class Read, class Submit>
int rotate_slots(Device& d, SlotSizes& sz, int (Device::*ensure)(Slot&), Laps& laps, More more,
                 Retire retire, Pack pack, Read read, Submit submit) {
  std::lock_guard<std::mutex> lk(d.mu);
  DeviceGuard guard;
  CIR_HIP(hipSetDevice(d.id));
  SlotDrain drain{d};  // an early return leaves no slot busy
  auto busy = [&] {
    for (const Slot& s : d.slot)
      if (s.busy) return true;
    return false;
  };
  int k = 0;
  while (more() || busy()) {
    Slot& s = d.slot[k];
    laps.start();
    if (s.busy) {
      const int rc = slot_wait(d, s);
      if (rc) return rc;
      retire(k, s);
    }
    laps.lap(laps.wait);
    if (more()) {
      int rc = d.ensure_slot(s, sz.cap, sz.cap_blk);
      if (rc) return rc;
      rc = (d.*ensure)(s);
      if (rc) return rc;
      const bool packed = pack(k, s);
      sz.offered();
      laps.lap(laps.pack);
      if (packed) {
        read(k, s);
        laps.lap(laps.read);
        rc = submit(k, s);
        if (rc) return rc;
        laps.lap(laps.submit);
        ++laps.batches;
      }
    }
    k = (k + 1) % Device::kSlots;
  }
  return CIR_OK;
}

}  // namespace stage
}  // namespace cir
