// cir_store_blocks: an image written out of device memory, indexed (and
// cir_gather_runs, cir_gather_runs_dev: its gather on its own).
//
// Reference: an image directory is filled block by block from the network
// (write_block, src/daemon/disk/public.rs) and its index comes from the
// uploader's scan (dir_signature::v1::scan, src/client/sync/uploads.rs:49-59);
// bytes that a process holds in device memory reach neither without one
// device-to-host copy and one file write per tensor.  Here the files' bytes are
// gathered into the packed staging slot on the device (gather.hpp, gather.hip),
// hashed there, and each slot comes down as one copy and is written out by the
// reader pool's threads while the next slots gather and download: cir_load_blocks
// (check.cpp) mirrored.  The index is made from the digests of the slot's bytes
// -- the bytes that were written -- by cir_index_emit's emitter, so it is
// cir_index_memory_dev's of the same list and cir_scan_v1's of the written tree.
//
// Files.  The packer walks the list in the caller's order and makes the
// directories a path implies with mkdirat below their parent's fd (an existing
// directory is accepted; each is then opened with O_DIRECTORY | O_NOFOLLOW).  A
// file is created with openat(O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW) and
// fchmod to exactly 0644 or 0755: by its writer when the whole file is one
// write job (the creates of many small files then run beside the writes), else
// by the packer, which remembers (st_dev, st_ino) and closes it; a writer then
// opens it again the way check.cpp's readers do and writes only if fstat shows
// the same file.  Writers reach a file through every directory component below
// the root fd, never by a path, never through a symlink.  So nothing is written
// through a symlink or outside the root, and a packer or a writer holds one
// directory fd and one file fd at a time.  The first failure on disk ends the
// call with CIR_EIO; what was written stays for the caller to remove.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "devcall.hpp"
#include "dirsig.hpp"
#include "emit.hpp"
#include "gather.hpp"
#include "memindex.hpp"
#include "pack.hpp"
#include "runtime.hpp"
#include "stage.hpp"

namespace cir {
namespace {

using namespace stage;

static_assert(CIR_GATHER_RUN_WORDS == gather::kRunWords &&
                  CIR_GATHER_RES_FIELDS == dev::kGatherResFields,
              "the header's constants are the rule's and the kernel's");

// One piece of a packed run for a writer: where to open the file again, what
// it must then be, and what to write of it.  (cut_pieces' field names: `dst`
// is the piece's place in the pinned slot, here the source of the write.)
struct WriteJob {
  size_t dir;
  const std::string* name;
  Seen seen;
  uint64_t file_off, len;
  const uint8_t* dst;
  size_t tag;  // the file
  // the whole file is this one job: the writer creates it (seen is unused)
  bool create;
};

// One run of a batch: `take` digests from block `at` of the batch are those of
// the global blocks from `global` on.
struct DigestRun {
  uint64_t at, global, take;
};

struct Store : Layout {
  emit::Layout lay;
  const uint8_t* exe = nullptr;
  const void* const* d_data = nullptr;
  std::vector<uint8_t> digests;  // 32 per block, the caller's file order
  // the first failure on disk
  std::mutex mu;
  std::atomic<bool> failed{false};
  std::string fail_msg;
  uint64_t n_dirs = 0, n_batches = 0, n_bad = 0;
  std::atomic<uint64_t> n_files{0}, n_bytes{0};

  std::string path_of(size_t item) const {
    std::string p;
    for (const std::string& c : dirs[items[item].dir]) p += "/" + c;
    return dirsig::escape(p + "/" + items[item].name);
  }
  void disk_fail(const char* what, size_t item, int e) {
    std::lock_guard<std::mutex> lk(mu);
    if (failed.load()) return;
    fail_msg = std::string("error ") + what + " " + path_of(item) + ": " + strerror(e) +
               " (errno " + std::to_string(e) + ")";
    failed.store(true);
  }
};

// The items and directories of the caller's list (valid: emit::build passed).
void lay_files(Store& S, const emit::Files& f, uint64_t bs) {
  std::map<std::vector<std::string>, size_t> interned;
  std::vector<std::string> comps;
  S.items.resize((size_t)f.nfiles);
  for (size_t i = 0; i < (size_t)f.nfiles; ++i) {
    const char* p = (const char*)f.paths + f.path_off[i];
    const size_t n = (size_t)(f.path_off[i + 1] - f.path_off[i]);
    comps.clear();
    size_t c0 = 1;
    for (size_t j = 1; j <= n; ++j)
      if (j == n || p[j] == '/') {
        comps.emplace_back(p + c0, j - c0);
        c0 = j + 1;
      }
    Item& it = S.items[i];
    it.entry = i;
    it.name = std::move(comps.back());
    comps.pop_back();
    const auto at = interned.emplace(comps, S.dirs.size());
    if (at.second) S.dirs.push_back(comps);
    it.dir = at.first->second;
    it.size = f.sizes[i];
    it.nblk = emit::blocks_of(it.size, bs);
    it.first_blk = S.lay.first_block[i];
  }
  S.nblk_total = S.lay.nblocks;
}

// open_dir that first makes each component (an existing one is accepted: what
// it is shows when it is opened).  *made += the directories made.
DirFd make_dir(FdCount& fds, int root, const std::vector<std::string>& comps, uint64_t* made) {
  DirFd d;
  d.fd = root;
  for (const std::string& c : comps) {
    int e = 0;
    bool fresh = false;
    if (::mkdirat(d.fd, c.c_str(), 0755) == 0)
      fresh = true;
    else if (errno != EEXIST)
      e = errno;
    int nfd = -1;
    if (!e) {
      nfd = fds.took(::openat(d.fd, c.c_str(), O_RDONLY | O_DIRECTORY | O_NOFOLLOW | O_CLOEXEC));
      if (nfd < 0) e = errno;
    }
    if (d.own) fds.close(d.fd);
    if (nfd < 0) {
      d.fd = -1;
      d.own = false;
      d.err = e;
      return d;
    }
    if (fresh) {
      (void)::fchmod(nfd, 0755);  // (whatever the umask is)
      ++*made;
    }
    d.fd = nfd;
    d.own = true;
  }
  return d;
}

// File `item` created in its directory `dfd`: new (O_EXCL), never through a
// symlink, of exactly its mode whatever the umask.  The open fd (the caller's
// to S.fds.close), or -1 with the failure reported.
int create_in(Store& S, int dfd, size_t item) {
  const int fd =
      S.fds.took(::openat(dfd, S.items[item].name.c_str(),
                          O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600));
  if (fd < 0) {
    S.disk_fail("creating", item, errno);
    return -1;
  }
  if (::fchmod(fd, S.exe && S.exe[item] ? 0755 : 0644) != 0) {
    const int e = errno;
    S.fds.close(fd);
    S.disk_fail("creating", item, e);
    return -1;
  }
  S.n_files.fetch_add(1);
  return fd;
}

// The packer's side of the tree: the directories made and the files that are
// not one write job created, in the caller's order, one directory fd kept while
// the next file needs the same one.
class Creator {
 public:
  explicit Creator(Store& S) : S_(S), made_(S.dirs.size(), 0) {}
  ~Creator() { close_dir(S_.fds, d_); }
  // Makes (once) and enters the directory of file `item`; false with the
  // failure reported.
  bool enter(size_t item) {
    const Item& it = S_.items[item];
    if (dir_ != it.dir) {
      close_dir(S_.fds, d_);
      d_ = made_[it.dir] ? open_dir(S_.fds, S_.root, S_.dirs[it.dir])
                         : make_dir(S_.fds, S_.root, S_.dirs[it.dir], &S_.n_dirs);
      dir_ = it.dir;
      if (d_.fd >= 0) made_[it.dir] = 1;
    }
    if (d_.fd < 0) {
      S_.disk_fail("making the directory of", item, d_.err);
      return false;
    }
    return true;
  }
  // Creates file `item` (empty, of its mode) and says what it is; false with
  // the failure reported.
  bool create(size_t item, Seen* seen) {
    if (!enter(item)) return false;
    const int fd = create_in(S_, d_.fd, item);
    if (fd < 0) return false;
    struct stat st;
    const int e = ::fstat(fd, &st) != 0 ? errno : 0;
    S_.fds.close(fd);
    if (e) {
      S_.disk_fail("creating", item, e);
      return false;
    }
    seen->dev = st.st_dev;
    seen->ino = st.st_ino;
    return true;
  }

 private:
  Store& S_;
  std::vector<char> made_;  // per directory: its components exist
  DirFd d_;
  size_t dir_ = SIZE_MAX;
};

// Write the batch's jobs on `threads` writers, each with a directory of its
// own kept across the jobs that share it.  The first failure is reported and
// ends the others' work: ESTALE when the file is not the one the packer made.
void run_writes(Store& S, const std::vector<WriteJob>& jobs, unsigned threads) {
  std::atomic<size_t> next{0};
  auto worker = [&] {
    DirCache dir(S);
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= jobs.size() || S.failed.load()) break;
      const WriteJob& j = jobs[i];
      const DirFd& d = dir.of(S.root, j.dir);
      int e = 0;
      int fd = -1;
      if (d.fd < 0) {
        e = d.err;
      } else if (j.create) {
        fd = create_in(S, d.fd, j.tag);
        if (fd < 0) continue;  // (reported)
      } else {
        fd = S.fds.took(::openat(d.fd, j.name->c_str(), O_WRONLY | O_NOFOLLOW | O_CLOEXEC));
        if (fd < 0) e = errno;
      }
      struct stat st;
      if (!e && !j.create) {
        if (::fstat(fd, &st) != 0)
          e = errno;
        else if (st.st_dev != j.seen.dev || st.st_ino != j.seen.ino)
          e = ESTALE;
      }
      uint64_t put = 0;
      while (!e && put < j.len) {
        const ssize_t r = ::pwrite(fd, j.dst + put, j.len - put, (off_t)(j.file_off + put));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          e = r == 0 ? ENOSPC : errno;
          break;
        }
        put += (uint64_t)r;
      }
      S.fds.close(fd);
      if (e)
        S.disk_fail("writing", j.tag, e);
      else
        S.n_bytes.fetch_add(j.len);
    }
  };
  parallel_run(std::max(1u, std::min<unsigned>(threads, (unsigned)jobs.size())), worker);
}

// The whole list on device d, in the caller's order.
int store_range(cir_ctx* ctx, Device& d, Store& S, unsigned threads) {
  const std::vector<Item>& items = S.items;
  const uint64_t bs = S.bs;
  uint64_t seg = 0;
  for (const Item& it : items) seg = std::max(seg, std::min<uint64_t>(it.size, bs));
  SlotSizes sz = slot_sizes(ctx->staging, seg, scan_ramp());
  Creator creator(S);
  size_t fi = 0;       // the file being packed
  uint64_t fblk = 0;   // its next block
  Seen seen;           // of file fi, when the packer created it
  bool whole = false;  // file fi is one write job: its writer creates it
  std::vector<WriteJob> jobs[Device::kSlots];  // per slot in flight
  std::vector<DigestRun> runs[Device::kSlots];
  Batch b;
  uint64_t ngath = 0, nunits = 0;  // the batch's gather table
  double write_ms = 0;
  auto more = [&] { return !S.failed.load() && fi < items.size(); };
  auto retire = [&](int k, Slot& s) {
    S.n_bad += s.h_scat[0];
    for (const DigestRun& r : runs[k])
      memcpy(S.digests.data() + 32 * r.global, s.h_out + 32 * r.at, 32 * r.take);
    if (S.failed.load()) return;  // (only drained)
    const auto t0 = Clock::now();
    run_writes(S, jobs[k], threads);
    if (trace_enabled()) write_ms += ms_between(t0, Clock::now());
  };
  auto pack = [&](int k, Slot& s) {
    jobs[k].clear();
    runs[k].clear();
    b = Batch();
    ngath = nunits = 0;
    while (fi < items.size() && b.n < sz.cap_blk) {
      const Item& it = items[fi];
      if (it.nblk == 0) {
        if (!creator.create(fi, &seen)) break;
        ++fi;
        continue;
      }
      const Batch before = b;
      const Run r =
          pack_run(b, sz.fill, sz.cap_blk, bs, it.size, fblk, it.nblk - fblk, s.h_off, s.h_len);
      if (!r.take) break;
      // A file that is one write job is created by its writer, beside the others'
      // writes (20,000 small files: the creates are half the call when the packer
      // makes them); the packer makes its directory.  Any other file the packer
      // creates when it packs the first run.
      if (fblk == 0) {
        whole = r.take == it.nblk && r.bytes <= kReadPiece;
        if (!(whole ? creator.enter(fi) : creator.create(fi, &seen))) {
          b = before;  // (the run is not part of the batch)
          break;
        }
      }
      // (at most one record per block: <= cap_blk)
      nunits = gather::record_of(r, (uint64_t)reinterpret_cast<uintptr_t>(S.d_data[fi]), fblk, bs,
                                 nunits, s.h_scat + kScatHead + gather::kRunWords * ngath++);
      cut_pieces(jobs[k], WriteJob{it.dir, &it.name, seen, fblk * bs, r.bytes, s.h_data + r.pos,
                                   fi, whole});
      runs[k].push_back({r.at, it.first_blk + fblk, r.take});
      fblk += r.take;
      if (fblk == it.nblk) {
        ++fi;
        fblk = 0;
      }
    }
    return b.n > 0;
  };
  auto read = [&](int, Slot&) {};  // (the slot is filled on the device)
  auto submit = [&](int, Slot& s) -> int {
    const int rc = slot_submit_store(d, s, b.used, b.n, S.ht, ngath, nunits);
    if (rc) return rc;
    ++S.n_batches;
    return CIR_OK;
  };
  Laps laps(trace_enabled());
  const int rc =
      rotate_slots(d, sz, &Device::ensure_store, laps, more, retire, pack, read, submit);
  if (rc) return rc;
  if (laps.on)
    fprintf(stderr,
            "cir store_blocks: dev %d, %llu batches; waiting for gather, hash and download %.2f "
            "ms, creating files and gather table %.2f ms, writes %.2f ms, submit %.2f ms\n",
            d.id, (unsigned long long)laps.batches, laps.wait - write_ms, laps.pack, write_ms,
            laps.submit);
  return CIR_OK;
}

int store_impl(cir_ctx* ctx, int dirfd, const char* dir, int hash_type, uint64_t bs,
               const uint8_t* paths, const uint64_t* path_off, const uint64_t* sizes,
               const uint8_t* exe, size_t nfiles, const void* const* d_data, void* stream,
               uint32_t threads, uint8_t** index_out, size_t* len_out, uint8_t* image_id,
               uint64_t* stats) {
  if (!index_out || !len_out || !stats) return fail(CIR_EINVAL, "null pointer");
  *index_out = nullptr;
  *len_out = 0;
  for (int i = 0; i < CIR_STORE_STATS_FIELDS; ++i) stats[i] = 0;
  if (!ctx) return fail(CIR_EINVAL, "null ctx");
  int rc = check_files(paths, path_off, sizes, nfiles);
  if (rc) return rc;
  if (nfiles && !d_data) return fail(CIR_EINVAL, "null pointer");
  if (!valid_hash_type(hash_type)) return fail(CIR_EINVAL, "unknown hash type");
  dirsig::Header h;
  if (!header_of(hash_type, bs, &h)) return fail(CIR_EINVAL, "block_size must be in 1 .. 2^32-1");
  Store S;
  std::string err;
  const emit::Files files{paths, path_off, sizes, exe, nfiles};
  if (!emit::build(files, bs, (uint64_t)INT32_MAX, &S.lay, &err)) return fail(CIR_EINVAL, err);
  if (S.lay.body_len > dev::kEmitMaxBody) return fail(CIR_EINVAL, "body longer than 2^40 bytes");
  for (size_t i = 0; i < nfiles; ++i)
    if (sizes[i] && !d_data[i])
      return fail(CIR_EINVAL, "null device pointer of a non-empty file");
  Device* dev = stream_device(ctx, (hipStream_t)stream);
  if (!dev) return fail(CIR_EINVAL, "stream device is not part of the context");
  // ---- nothing above touched a file or queued device work
  S.bs = bs;
  S.ht = hash_type;
  S.exe = exe;
  S.d_data = d_data;
  lay_files(S, files, bs);
  S.digests.resize((size_t)(32 * S.lay.nblocks));
  rc = open_image(S, dirfd, dir);
  if (rc) return rc;
  if (S.lay.nblocks == 0) {
    // only size-0 files (or none): nothing for a device
    Creator creator(S);
    Seen seen;
    for (size_t i = 0; i < nfiles && !S.failed.load(); ++i) creator.create(i, &seen);
  } else {
    // The compute stream -- the gathers run there -- first waits for what the
    // caller queued on `stream`: whatever produces the data is done before the
    // first byte is read.
    rc = [&]() -> int {
      DeviceGuard guard;
      CIR_HIP(hipSetDevice(dev->id));
      hipEvent_t ev = nullptr;
      CIR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      hipError_t e = hipEventRecord(ev, (hipStream_t)stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(dev->compute, ev, 0);
      (void)hipEventDestroy(ev);  // (released once it has completed)
      if (e != hipSuccess) return hip_fail(e, "ordering the compute stream behind the caller's");
      return store_range(ctx, *dev, S, threads ? threads : host_copy_threads((size_t)1));
    }();
    if (rc) return rc;
  }
  if (S.failed.load()) return fail(CIR_EIO, S.fail_msg);
  if (S.n_bad) return fail(CIR_EIO, "the gather kernel met a record outside its slot");
  rc = emit_index_host(S.lay, h, S.digests.data(), index_out, len_out, image_id);
  if (rc) return rc;
  stats[0] = S.lay.nblocks;
  stats[1] = S.n_files;
  stats[2] = S.n_dirs;
  stats[3] = S.n_bytes.load();
  stats[4] = S.n_batches;
  stats[5] = S.lay.body_len;
  return CIR_OK;
}

// ---- cir_gather_runs, cir_gather_runs_dev: the gather on its own ---------------

int check_gather(const void* dst, const void* runs, uint64_t nruns, uint64_t nunits,
                 const void* res) {
  if ((nunits && !dst) || (nruns && !runs) || !res) return fail(CIR_EINVAL, "null pointer");
  if (nruns > gather::kMaxRuns) return fail(CIR_EINVAL, "more than 2^32-1 records");
  if (nunits > gather::kMaxUnits) return fail(CIR_EINVAL, "more than 2^32-1 units");
  return CIR_OK;
}

int gather_host_impl(uint8_t* dst, uint64_t dst_bytes, const uint64_t* runs, uint64_t nruns,
                     uint64_t nunits, uint64_t* res) {
  const int rc = check_gather(dst, runs, nruns, nunits, res);
  if (rc) return rc;
  res[0] = gather::apply_host(dst, dst_bytes, runs, nruns, nunits);
  return CIR_OK;
}

int gather_dev_impl(uint8_t* d_dst, uint64_t dst_bytes, const uint64_t* d_runs, uint64_t nruns,
                    uint64_t nunits, uint64_t* d_res, void* stream) {
  const int rc = check_gather(d_dst, d_runs, nruns, nunits, d_res);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(d_dst) & 15u)
    return fail(CIR_EINVAL, "d_dst must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_runs) | reinterpret_cast<uintptr_t>(d_res)) & 7u)
    return fail(CIR_EINVAL, "d_runs and d_res must be 8-byte aligned");
  CIR_HIP(dev::launch_gather_runs(d_dst, dst_bytes, d_runs, nruns, nunits, d_res,
                                  (hipStream_t)stream));
  return CIR_OK;
}

}  // namespace
}  // namespace cir

extern "C" int cir_gather_runs(uint8_t* dst, uint64_t dst_bytes, const uint64_t* runs,
                               uint64_t nruns, uint64_t nunits,
                               uint64_t res[CIR_GATHER_RES_FIELDS]) try {
  return cir::gather_host_impl(dst, dst_bytes, runs, nruns, nunits, res);
} CIR_CATCH_BOUNDARY

extern "C" int cir_gather_runs_dev(cir_ctx* ctx, uint8_t* d_dst, uint64_t dst_bytes,
                                   const uint64_t* d_runs, uint64_t nruns, uint64_t nunits,
                                   uint64_t* d_res, void* stream) try {
  (void)ctx;  // no scratch of the context's, no side streams
  return cir::gather_dev_impl(d_dst, dst_bytes, d_runs, nruns, nunits, d_res, stream);
} CIR_CATCH_BOUNDARY

extern "C" int cir_store_blocks(cir_ctx* ctx, int dirfd, const char* dir, int hash_type,
                                uint64_t block_size, const uint8_t* paths,
                                const uint64_t* path_off, const uint64_t* sizes,
                                const uint8_t* exe, size_t nfiles, const void* const* d_data,
                                void* stream, uint32_t threads, uint8_t** index_out,
                                size_t* len_out, uint8_t image_id[CIR_DIGEST_BYTES],
                                uint64_t stats[CIR_STORE_STATS_FIELDS]) try {
  return cir::store_impl(ctx, dirfd, dir, hash_type, block_size, paths, path_off, sizes, exe,
                         nfiles, d_data, stream, threads, index_out, len_out, image_id, stats);
} CIR_CATCH_BOUNDARY
