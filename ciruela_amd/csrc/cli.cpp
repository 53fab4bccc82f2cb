// ciruela-index: the indexing half of `ciruela sync`, on the GPU path.
//
// Reference: `ciruela sync` (src/client/main.rs:94-99 -> src/client/sync/
// mod.rs:168-220 -> uploads::prepare, src/client/sync/uploads.rs:61-105).
// For every --append / --append-weak / --replace SRC:DEST it runs the scan
// (uploads.rs:49-59, threads = --disk-threads), registers the
// index (InMemoryIndexes::register_index -> ImageId) and prints
//   <image id> <kind> <dest> <src>
// Signing and the upload itself (networking, src/client/sync/network.rs) are
// out of scope; --index-dir writes each index as
// <dir>/<image id>.ds1 so a separate uploader can pick it up.
//
//   ciruela-index sync [--disk-threads N] [--block-size N] [--index-dir D]
//                      --append SRC:/DEST [--append-weak SRC:/DEST]
//                      [--replace SRC:/DEST[:OLD_IMAGE_ID]] ...
//   ciruela-index hash [--block-size N] FILE...   (per-block BlockHash list)
//   ciruela-index check DIR INDEX_FILE [--disk-threads N]
//       the daemon's commit-time re-hash (commit_image, src/daemon/disk/
//       commit.rs:51-117) of the image in DIR against INDEX_FILE: silent and
//       exit 0 when every listed file matches, else exit 1 with one line,
//       `checksum: <path>` or `read: <path>: <strerror>`
//   ciruela-index links INDEX SRCDIR=SRCINDEX [SRCDIR=SRCINDEX ...] [--disk-threads N] [--host]
//                       [--any-path]
//       the daemon's hardlink step before a download (scan_links, src/daemon/
//       metadata/hardlink_sources.rs:107-153, then check_and_hardlink, src/
//       daemon/disk/public.rs:285-346): which files of the new image INDEX
//       can be linked from the older images -- SRCDIR with its index
//       SRCINDEX (split at the last `=`), best source first.  Prints
//       `SRCDIR<TAB>PATH` (the path as the index spells it) for every
//       candidate that passed the re-hash and the mode test, a summary on
//       stderr, and exits 0 when the check ran.  Nothing is linked.  The
//       candidates come from cir_file_sources on the context the check uses;
//       --host takes them from cir_link_candidates (the output is the same).
//       --any-path adds, for the files without such a candidate, the ones
//       cir_file_copies finds by content at another path, and verifies all of
//       them in one cir_check_links_at call; those print
//       `SRCDIR<TAB>PATH<TAB>SRCPATH` (the path in the source, escaped).
//   ciruela-index candidates INDEX SRCINDEX [SRCINDEX ...] [--host]
//       the first half of that step alone (cir_file_sources; no file is
//       read): one line `FILE# SRC# PATH` per candidate -- the file ordinal in
//       INDEX, the ordinal of the first SRCINDEX (best first) that lists the
//       path with equal exe flag, size and digests, the path as the index
//       spells it.  --host passes no context and opens no device.
//   ciruela-index copies INDEX SRCINDEX [SRCINDEX ...] [--host] [--unlinked]
//       the step behind that one (cir_file_copies; no file is read): the
//       files an older image holds unchanged at any path -- below a renamed
//       directory, moved, vendored twice.  One line `FILE# SRC# SRCFILE# PATH
//       SRCPATH` per candidate: the file ordinal in INDEX, the first SRCINDEX
//       (best first) that holds a file with equal exe flag, size and digests,
//       the first such file's ordinal in it, the path in INDEX as the index
//       spells it and the path in the source, escaped.  --unlinked first runs
//       the `candidates` rule and leaves out the files it found.  --host
//       passes no context and opens no device.
//   ciruela-index plan INDEX SRCINDEX [SRCINDEX ...] [--host]
//       the whole download plan in one call (cir_fetch_plan; no file is
//       read): the counts and bytes per class -- files to link at their own
//       path, files to link by content, extents to copy from older images,
//       extents to copy inside the image, blocks to fetch.  --host passes no
//       context and opens no device.
//   ciruela-index blocks DIR INDEX_FILE [--list] [--disk-threads N]
//       which blocks of INDEX_FILE the partial image in DIR already holds
//       (cir_check_blocks); --list prints `PATH OFFSET` per missing block
//   ciruela-index sources INDEX SRCINDEX [SRCINDEX ...] [--list] [--host] [--extents]
//       what fill_blocks (src/daemon/tracking/progress.rs:129-170) need not
//       fetch: which blocks of the new image INDEX the older images'
//       indexes SRCINDEX (best first) list, by digest, and where
//       (cir_block_sources; no file is read).  Prints one summary line --
//       blocks, found, bytes found, sources used and skipped -- and with
//       --list one line per found block, `PATH OFFSET LENGTH SRC# SRCPATH
//       SRCOFFSET` (paths escaped as in the index).  --host passes no
//       context: the join runs on the host and no device is opened.
//       --extents (cir_block_extents): the copies merged into extents, one
//       line of the same form per extent (one copy_file_range each), behind
//       a summary line that also counts the extents and the blocks left to
//       fetch.
//   ciruela-index repeats INDEX [--host]
//       what is left after that: which blocks of INDEX carry a digest that an
//       earlier block of INDEX carries, so that they are copied inside the
//       image instead of fetched twice (cir_block_repeats with every block
//       wanted and none present; no file is read).  Prints one summary line --
//       blocks, repeats, extents, bytes, left to fetch -- and one line per
//       extent, `PATH OFFSET LENGTH CLASS SRCPATH SRCOFFSET` (CLASS 1: the
//       source block is one of those fetched).  --host opens no device.
//   ciruela-index sketch INDEX [-k N] [-o FILE] [--host]
//       the content sketch of INDEX (cir_index_sketch): the N (default 1024)
//       smallest distinct keys of its block digests, a blob of at most 40 + 8 N
//       bytes to keep beside the index, written to FILE (default: standard
//       output).  --host passes no context and opens no device.
//   ciruela-index rank NEED SRC [SRC ...] [-k N] [--host]
//       which older images are worth handing to `plan` (cir_sketch_rank): the
//       sources ordered by how much of NEED each holds, one line `ORDINAL SHARED
//       EXAMINED PATH` per ranked source, best first; a source of another hash
//       type or block size, or one that is neither a sketch nor an index, is
//       left out and counted on stderr.  Each argument is a sketch file or an
//       index file, told apart by its first bytes; an index is sketched on the
//       spot (size N).  A device is opened only when an index is among them.
#include <dirent.h>
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "ciruela_blockhash.h"

static void usage() {
  fprintf(stderr,
          "usage: ciruela-index sync [--disk-threads N] [--block-size N] [--index-dir D]\n"
          "                          (--append|--append-weak|--replace) SRC:/DEST ...\n"
          "       ciruela-index hash [--block-size N] FILE...\n"
          "       ciruela-index check DIR INDEX_FILE [--disk-threads N]\n"
          "       ciruela-index links INDEX SRCDIR=SRCINDEX [SRCDIR=SRCINDEX ...]"
          " [--disk-threads N] [--host] [--any-path]\n"
          "       ciruela-index candidates INDEX SRCINDEX [SRCINDEX ...] [--host]\n"
          "       ciruela-index copies INDEX SRCINDEX [SRCINDEX ...] [--host] [--unlinked]\n"
          "       ciruela-index plan INDEX SRCINDEX [SRCINDEX ...] [--host]\n"
          "       ciruela-index blocks DIR INDEX_FILE [--list] [--disk-threads N]\n"
          "       ciruela-index sources INDEX SRCINDEX [SRCINDEX ...] [--list] [--host]"
          " [--extents]\n"
          "       ciruela-index repeats INDEX [--host]\n"
          "       ciruela-index sketch INDEX [-k N] [-o FILE] [--host]\n"
          "       ciruela-index rank NEED SRC [SRC ...] [-k N] [--host]\n");
}

static std::string hex(const uint8_t* p, size_t n) {
  static const char k[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += k[p[i] >> 4];
    s += k[p[i] & 15];
  }
  return s;
}

// A decoded path as an index spells it: bytes outside printable ASCII, the
// space and the backslash as \xNN.
static std::string escape_path(const uint8_t* p, size_t n) {
  static const char k[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    if (p[i] > 0x20 && p[i] < 0x7f && p[i] != '\\') {
      s += (char)p[i];
    } else {
      s += "\\x";
      s += k[p[i] >> 4];
      s += k[p[i] & 15];
    }
  }
  return s;
}

static int die(int rc, const char* what) {
  fprintf(stderr, "%s: %s: %s\n", what, cir_strerror(rc), cir_last_error());
  return rc == CIR_EIO ? 1 : 2;
}

// Bytes of the regular files under path, counted only until they reach cap.
// The top-level argument is followed as the scan and the hash path follow it
// (open): a symlinked SRC or FILE counts its target; entries inside
// directories are not followed (fstatat AT_SYMLINK_NOFOLLOW), as the scan's
// walk does, and each directory is read through its own fd opened from its
// parent's (openat), so a tree nested past PATH_MAX is counted too.  A
// top-level argument that is neither a regular file nor a directory (a pipe,
// /dev/stdin) has no size to count and gets the default staging (returns cap).
static uint64_t dir_bytes(int dfd, uint64_t cap, uint64_t acc) {
  const int lfd = fcntl(dfd, F_DUPFD_CLOEXEC, 0);
  DIR* d = lfd >= 0 ? fdopendir(lfd) : nullptr;
  if (!d) {
    if (lfd >= 0) close(lfd);
    return acc;
  }
  while (struct dirent* e = readdir(d)) {
    if (!strcmp(e->d_name, ".") || !strcmp(e->d_name, "..")) continue;
    struct stat st;
    if (fstatat(dfd, e->d_name, &st, AT_SYMLINK_NOFOLLOW) != 0) continue;
    if (S_ISREG(st.st_mode)) {
      acc += (uint64_t)st.st_size;
    } else if (S_ISDIR(st.st_mode)) {
      const int cfd = openat(dfd, e->d_name, O_RDONLY | O_DIRECTORY | O_NOFOLLOW | O_CLOEXEC);
      if (cfd >= 0) {
        acc = dir_bytes(cfd, cap, acc);
        close(cfd);
      }
    }
    if (acc >= cap) break;
  }
  closedir(d);
  return acc;
}

static uint64_t tree_bytes(const std::string& path, uint64_t cap, uint64_t acc) {
  struct stat st;
  if (acc >= cap) return acc;
  if (stat(path.c_str(), &st) != 0) return cap;
  if (S_ISREG(st.st_mode)) return acc + (uint64_t)st.st_size;
  if (!S_ISDIR(st.st_mode)) return cap;
  const int fd = open(path.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
  if (fd < 0) return acc;
  acc = dir_bytes(fd, cap, acc);
  close(fd);
  return acc;
}

// Bytes of every input, counted up to what decides the device count: two
// default staging slots per device for 32 devices (cir_devices_for_bytes).
static uint64_t input_bytes(const std::vector<std::string>& paths) {
  constexpr uint64_t kCap = 32 * 2 * (256ull << 20);
  uint64_t total = 0;
  for (const std::string& p : paths) total = tree_bytes(p, kCap, total);
  return total;
}

// Staging per slot: the library default (256 MiB) for large inputs; a small
// input gets slots just big enough to hold it, so a one-shot `sync` of a few
// MiB does not pin 3 x 256 MiB of host memory it never fills (cir_init
// allocates the slots up front).
static uint64_t staging_for(uint64_t total) {
  constexpr uint64_t kMax = 256ull << 20, kMin = 1ull << 20;
  if (total >= kMax) return 0;
  return std::max<uint64_t>(kMin, (total + kMin - 1) / kMin * kMin);
}

// A profiling tool library loaded into this process (rocprofv3's
// environment), which writes its output from the exit handlers.
static bool profiled() {
  extern char** environ;
  for (char** e = environ; e && *e; ++e)
    if (!strncmp(*e, "ROCP_TOOL_LIBRARIES=", 20) || !strncmp(*e, "ROCPROF", 7)) return true;
  return false;
}

struct Job {
  std::string kind, src, dest;
};

static bool read_file(const std::string& path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    perror(path.c_str());
    return false;
  }
  uint8_t buf[65536];
  size_t r;
  while ((r = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + r);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) fprintf(stderr, "%s: read error\n", path.c_str());
  return !bad;
}

// The paths of an index's file entries, in index order and as the index
// spells them (escaped): a directory line starts with '/', an entry line with
// two spaces, and its second field is f or x for a file.
static std::vector<std::string> index_file_paths(const std::vector<uint8_t>& index,
                                                 std::vector<uint64_t>* sizes = nullptr,
                                                 uint64_t* block_size = nullptr) {
  std::vector<std::string> out;
  std::string dir;
  size_t pos = 0;
  bool header = true;
  while (pos < index.size()) {
    const void* nl = memchr(index.data() + pos, '\n', index.size() - pos);
    const size_t e = nl ? (size_t)((const uint8_t*)nl - index.data()) : index.size();
    const std::string line(reinterpret_cast<const char*>(index.data()) + pos, e - pos);
    pos = e + 1;
    if (header) {
      header = false;
      const size_t b = line.find(" block_size=");
      if (block_size && b != std::string::npos)
        *block_size = strtoull(line.c_str() + b + 12, nullptr, 10);
      continue;
    }
    if (!line.empty() && line[0] == '/') {
      dir = line;
    } else if (line.size() > 2 && line[0] == ' ' && line[1] == ' ') {
      const size_t sp = line.find(' ', 2);
      if (sp == std::string::npos || sp + 1 >= line.size()) continue;
      if ((line[sp + 1] == 'f' || line[sp + 1] == 'x') &&
          (sp + 2 == line.size() || line[sp + 2] == ' ')) {
        out.push_back((dir == "/" ? "" : dir) + "/" + line.substr(2, sp - 2));
        if (sizes)
          sizes->push_back(sp + 3 < line.size() ? strtoull(line.c_str() + sp + 3, nullptr, 10) : 0);
      }
    }
  }
  return out;
}

// Does a file hold a sketch blob (cir_index_sketch's magic) rather than an index?
static bool is_sketch(const std::vector<uint8_t>& data) {
  return data.size() >= 8 && memcmp(data.data(), "CIRSKv1", 8) == 0;
}

// split "source:/dir/dest" (src/client/sync/uploads.rs:25-33)
static bool split(const std::string& cli, std::string* src, std::string* dest) {
  const size_t c = cli.find(':');
  if (c == std::string::npos) return false;
  *src = cli.substr(0, c);
  std::string rest = cli.substr(c + 1);
  const size_t c2 = rest.find(':');
  *dest = c2 == std::string::npos ? rest : rest.substr(0, c2);
  return !dest->empty() && (*dest)[0] == '/';
}

int main(int argc, char** argv) {
  if (argc < 2) {
    usage();
    return 2;
  }
  const std::string cmd = argv[1];
  // --disk-threads N is GlobalOptions.threads (src/client/global_options.rs:13,
  // default 4), the reference's CPU hashing pool.  Here the host threads
  // only read files into the staging buffers, and 4 readers hold a large
  // tree to ~22 GiB/s, so without the flag the library picks
  // its reader count (0: min(12, 3/4 of the CPU share)); given, N is used.
  uint32_t threads = 0;
  uint64_t bs = CIR_DEFAULT_BLOCK_SIZE;
  std::string index_dir;
  bool list_blocks = false, host_only = false, extents = false, host_candidates = false;
  bool unlinked = false, any_path = false;
  const bool sketching = cmd == "sketch" || cmd == "rank";
  uint32_t sketch_k = CIR_SKETCH_DEFAULT_K;
  std::string out_path;
  std::vector<Job> jobs;
  std::vector<std::string> files;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> std::string {
      if (i + 1 >= argc) {
        usage();
        exit(2);
      }
      return argv[++i];
    };
    if (a == "--disk-threads" || a == "--block-size") {
      // a decimal count (clap's usize parse in the reference): anything else
      // is a usage error, not an exception out of main
      const std::string v = val();
      char* end = nullptr;
      errno = 0;
      const unsigned long long n = strtoull(v.c_str(), &end, 10);
      if (v.empty() || v[0] == '-' || *end || errno ||
          (a == "--disk-threads" && n > 0xffffffffull)) {
        fprintf(stderr, "invalid value for %s: %s\n", a.c_str(), v.c_str());
        return 2;
      }
      if (a == "--disk-threads")
        threads = (uint32_t)n;
      else
        bs = n;
    }
    else if (a == "--index-dir") index_dir = val();
    else if (a == "-k" && sketching) {
      const std::string v = val();
      char* end = nullptr;
      const unsigned long long n = strtoull(v.c_str(), &end, 10);
      if (v.empty() || v[0] == '-' || *end || n < 1 || n > CIR_SKETCH_MAX_K) {
        fprintf(stderr, "invalid value for -k: %s (1 .. %d)\n", v.c_str(), CIR_SKETCH_MAX_K);
        return 2;
      }
      sketch_k = (uint32_t)n;
    }
    else if (a == "-o" && cmd == "sketch") out_path = val();
    else if (a == "--host" && sketching) host_only = true;
    else if (a == "--list" && (cmd == "blocks" || cmd == "sources")) list_blocks = true;
    else if (a == "--host" &&
             (cmd == "sources" || cmd == "repeats" || cmd == "candidates" || cmd == "copies" ||
       cmd == "plan"))
      host_only = true;
    else if (a == "--unlinked" && cmd == "copies") unlinked = true;
    else if (a == "--host" && cmd == "links") host_candidates = true;
    else if (a == "--any-path" && cmd == "links") any_path = true;
    else if (a == "--extents" && cmd == "sources") extents = true;
    else if (a == "--append" || a == "--append-weak" || a == "--replace") {
      Job j;
      j.kind = a.substr(2);
      if (!split(val(), &j.src, &j.dest)) {
        fprintf(stderr, "Destination directory is invalid, must be `source:/dir/dest`\n");
        return 2;
      }
      jobs.push_back(j);
    } else if ((cmd == "hash" || cmd == "check" || cmd == "links" || cmd == "blocks" ||
                cmd == "sources" || cmd == "repeats" || cmd == "candidates" || cmd == "copies" ||
       cmd == "plan" || sketching) &&
               a.size() &&
               a[0] != '-') {
      files.push_back(a);
    } else {
      usage();
      return 2;
    }
  }
  if ((cmd == "check" || cmd == "blocks") && files.size() != 2) {
    usage();
    return 2;
  }
  std::vector<std::string> link_dirs;
  std::vector<std::vector<uint8_t>> link_indexes;
  if (cmd == "links") {
    if (files.size() < 2) {
      usage();
      return 2;
    }
    for (size_t i = 1; i < files.size(); ++i) {
      const size_t eq = files[i].rfind('=');
      if (eq == std::string::npos || eq == 0 || eq + 1 == files[i].size()) {
        usage();
        return 2;
      }
      link_dirs.push_back(files[i].substr(0, eq));
      link_indexes.emplace_back();
      if (!read_file(files[i].substr(eq + 1), &link_indexes.back())) return 2;
    }
  }
  if (cmd == "sources" || cmd == "candidates" || cmd == "copies" ||
       cmd == "plan") {
    // the indexes are read (and a missing one reported) before any device is opened
    if (files.size() < 2) {
      usage();
      return 2;
    }
    for (size_t i = 1; i < files.size(); ++i) {
      link_indexes.emplace_back();
      if (!read_file(files[i], &link_indexes.back())) return 2;
    }
  }
  if ((cmd == "repeats" || cmd == "sketch") && files.size() != 1) {
    usage();
    return 2;
  }
  if (cmd == "rank") {
    // every argument is read before any device is opened; sketches alone need none
    if (files.size() < 2) {
      usage();
      return 2;
    }
    bool any_index = false;
    for (const std::string& f : files) {
      link_indexes.emplace_back();
      if (!read_file(f, &link_indexes.back())) return 2;
      any_index = any_index || !is_sketch(link_indexes.back());
    }
    if (!any_index) host_only = true;
  }
  std::vector<std::string> inputs = cmd == "links" ? link_dirs : files;
  if (cmd == "sources" || cmd == "repeats" || cmd == "candidates" || cmd == "copies" ||
       cmd == "plan" || sketching)
    inputs.clear();  // (indexes only: nothing is staged)
  std::vector<uint8_t> check_index;
  // (read, and a missing one reported, before any device is opened)
  if ((cmd == "sources" || cmd == "repeats" || cmd == "candidates" || cmd == "copies" ||
       cmd == "plan" || cmd == "sketch") &&
      !read_file(files[0], &check_index))
    return 2;
  if (cmd == "links" && !read_file(files[0], &check_index)) return 2;
  if (cmd == "check" || cmd == "blocks") {
    // the index is read (and a missing one reported) before any device is
    // opened; the staging slots are sized from the image alone
    inputs.pop_back();
    FILE* f = fopen(files[1].c_str(), "rb");
    if (!f) {
      perror(files[1].c_str());
      return 2;
    }
    uint8_t buf[65536];
    size_t r;
    while ((r = fread(buf, 1, sizeof buf, f)) > 0) check_index.insert(check_index.end(), buf, buf + r);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) {
      fprintf(stderr, "%s: read error\n", files[1].c_str());
      return 2;
    }
  }
  for (const Job& j : jobs) inputs.push_back(j.src);
  cir_ctx* ctx = nullptr;
  const uint64_t total = input_bytes(inputs);
  const uint64_t staging = staging_for(total);
  const char* tv = getenv("CIR_TRACE");
  const bool trace = tv && *tv && strcmp(tv, "0") != 0;
  // An input below one staging slot is one small batch: its copies go
  // through the runtime's blit kernels instead of the SDMA engines, whose
  // first use in a process costs ~16-17 ms (cir_init's first uploads) -- a
  // tenth of a one-shot `sync` of config 1's 10 MiB tree
  // (profiles/r05/cli_sdma_ab.log).  Large inputs keep SDMA (the link's full
  // rate); a caller's own HSA_ENABLE_SDMA wins.  Set before the first HIP
  // call, when the runtime reads it.
  const bool small = staging != 0;
  if (small && !getenv("HSA_ENABLE_SDMA")) setenv("HSA_ENABLE_SDMA", "0", 0);
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  if (trace && !host_only) {
    fprintf(stderr, "ciruela-index: staging %llu bytes per slot (0 = library default), %s copies\n",
            (unsigned long long)staging,
            strcmp(getenv("HSA_ENABLE_SDMA") ? getenv("HSA_ENABLE_SDMA") : "1", "0") == 0
                ? "blit" : "SDMA");
    // the HIP runtime's own start-up (device discovery), apart from cir_init
    const auto t0 = std::chrono::steady_clock::now();
    const int n = cir_device_count();
    fprintf(stderr, "ciruela-index: HIP runtime start %.1f ms (%d devices)\n", ms_since(t0), n);
  }
  // open only the GPUs the input can use: one per two staging batches of it
  // (cir_devices_for_bytes), the lowest-numbered first -- a tree below one
  // slot (256 MiB) is one batch on one GPU -- instead of every GPU of the
  // node (each costs its device context, streams and 834 MiB of pinned
  // staging at start-up, include/ciruela_blockhash.h)
  // (an empty input -- empty files, an empty tree -- is measured, not
  // unknown: one device, not cir_devices_for_bytes' "0 = every device")
  const uint32_t ndev = cir_devices_for_bytes(std::max<uint64_t>(total, 1), staging, 32);
  const auto t_init = std::chrono::steady_clock::now();
  // and a small input is one short job: one stream and one slot per device
  // (CIR_INIT_ONE_SHOT; the other streams' hardware queues were ~25 ms of
  // cir_init, profiles/r05/start_env.log)
  int rc = host_only ? CIR_OK : cir_init_n(&ctx, 0, staging, ndev, small ? CIR_INIT_ONE_SHOT : 0u);
  if (rc) return die(rc, "cir_init");
  if (trace && !host_only) {
    int ids[64];
    const int opened = cir_ctx_devices(ctx, ids, 64);
    fprintf(stderr, "ciruela-index: cir_init %.1f ms, %d device(s) for %llu input bytes\n",
            ms_since(t_init), opened, (unsigned long long)total);
  }
  if (cmd == "hash") {
    for (const std::string& f : files) {
      const int fd = open(f.c_str(), O_RDONLY);
      if (fd < 0) {
        perror(f.c_str());
        return 1;
      }
      uint64_t size = 0;
      uint8_t* h = nullptr;
      size_t n = 0;
      rc = cir_hash_file(ctx, fd, bs, &size, &h, &n);
      close(fd);
      if (rc) return die(rc, f.c_str());
      printf("%s %llu", f.c_str(), (unsigned long long)size);
      for (size_t k = 0; k < n; ++k) printf(" %s", hex(h + 32 * k, 32).c_str());
      printf("\n");
      cir_free(h);
    }
  } else if (cmd == "check") {
    int kind = CIR_CHECK_OK;
    uint8_t* path = nullptr;
    size_t plen = 0;
    uint64_t st[CIR_CHECK_STATS_FIELDS];
    static const uint8_t none = 0;
    rc = cir_check_index(ctx, AT_FDCWD, files[0].c_str(),
                         check_index.empty() ? &none : check_index.data(), check_index.size(),
                         threads, &kind, &path, &plen, st);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    if (kind != CIR_CHECK_OK) {
      const std::string p(reinterpret_cast<const char*>(path), plen);
      if (kind == CIR_CHECK_CHECKSUM)
        printf("checksum: %s\n", p.c_str());
      else
        printf("read: %s: %s\n", p.c_str(), strerror((int)st[6]));
      fflush(stdout);
      return 1;
    }
  } else if (cmd == "blocks") {
    // exit statuses as `check`: 0 when every file is complete, 1 otherwise
    uint64_t* have = nullptr;
    uint64_t nblk = 0;
    uint8_t* state = nullptr;
    size_t nfiles = 0;
    uint64_t st[CIR_BLOCKS_STATS_FIELDS];
    static const uint8_t none = 0;
    rc = cir_check_blocks(ctx, AT_FDCWD, files[0].c_str(),
                          check_index.empty() ? &none : check_index.data(), check_index.size(),
                          threads, &have, &nblk, &state, nullptr, &nfiles, st);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    printf("blocks: %llu of %llu; files: %llu complete, %llu absent, %llu partial, %llu blocked\n",
           (unsigned long long)st[0], (unsigned long long)nblk, (unsigned long long)st[2],
           (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[5]);
    if (list_blocks) {
      std::vector<uint64_t> sizes;
      uint64_t ibs = 0;
      const std::vector<std::string> paths = index_file_paths(check_index, &sizes, &ibs);
      uint64_t g = 0;
      for (size_t i = 0; i < paths.size() && ibs; ++i) {
        const uint64_t n = (sizes[i] + ibs - 1) / ibs;
        for (uint64_t j = 0; j < n && g + j < nblk; ++j)
          if (!(have[(g + j) >> 6] >> ((g + j) & 63) & 1))
            printf("%s %llu\n", paths[i].c_str(), (unsigned long long)(j * ibs));
        g += n;
      }
    }
    fflush(stdout);
    const bool complete = st[2] == nfiles;
    cir_free(have);
    cir_free(state);
    if (!complete) return 1;
  } else if (cmd == "links") {
    static const uint8_t none = 0;
    const uint8_t* index = check_index.empty() ? &none : check_index.data();
    std::vector<const uint8_t*> sidx;
    std::vector<size_t> slen;
    for (const std::vector<uint8_t>& v : link_indexes) {
      sidx.push_back(v.empty() ? &none : v.data());
      slen.push_back(v.size());
    }
    uint64_t* lf = nullptr;
    uint32_t* ls = nullptr;
    size_t nl = 0, skipped = 0;
    uint64_t fst[CIR_FILE_SOURCES_STATS_FIELDS];
    rc = host_candidates
             ? cir_link_candidates(index, check_index.size(), sidx.data(), slen.data(), sidx.size(),
                                   &lf, &ls, &nl, &skipped)
             : cir_file_sources(ctx, index, check_index.size(), sidx.data(), slen.data(),
                                sidx.size(), &lf, &ls, &nl, &skipped, fst);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    std::vector<int> dirfds(link_dirs.size(), AT_FDCWD);
    std::vector<const char*> dirs;
    for (const std::string& d : link_dirs) dirs.push_back(d.c_str());
    const std::vector<std::string> paths = index_file_paths(check_index);
    uint64_t st[CIR_LINKS_STATS_FIELDS];
    if (any_path) {
      // the files without a same-path candidate, matched by content; all verified in one call
      std::vector<uint64_t> skip(paths.size() / 64 + 1, 0);
      for (size_t i = 0; i < nl; ++i)
        if (lf[i] < paths.size()) skip[lf[i] >> 6] |= 1ull << (lf[i] & 63);
      uint64_t* cf = nullptr;
      uint32_t* cs = nullptr;
      uint64_t* csf = nullptr;
      uint64_t* off = nullptr;
      uint8_t* sp = nullptr;
      size_t nc = 0;
      uint64_t cst[CIR_FILE_COPIES_STATS_FIELDS];
      rc = cir_file_copies(host_candidates ? nullptr : ctx, index, check_index.size(), sidx.data(),
                           slen.data(), sidx.size(), skip.data(), &cf, &cs, &csf, &off, &sp, &nc,
                           nullptr, cst);
      if (rc) {
        die(rc, files[0].c_str());
        return 2;
      }
      std::vector<uint64_t> all_f(lf, lf + nl), all_off(nl + 1, 0);  // (an empty path: the entry's own)
      std::vector<uint32_t> all_s(ls, ls + nl);
      all_f.insert(all_f.end(), cf, cf + nc);
      all_s.insert(all_s.end(), cs, cs + nc);
      for (size_t i = 0; i < nc; ++i) all_off.push_back(off[i + 1]);
      std::vector<uint8_t> kinds(nl + nc);
      rc = cir_check_links_at(ctx, index, check_index.size(), dirfds.data(), dirs.data(),
                              dirs.size(), all_f.data(), all_s.data(), all_off.data(), sp, nl + nc,
                              threads, kinds.data(), nullptr, st);
      if (rc) {
        die(rc, files[0].c_str());
        return 2;
      }
      for (size_t i = 0; i < nl + nc; ++i) {
        if (kinds[i] != CIR_CHECK_OK || all_f[i] >= paths.size()) continue;
        if (i < nl)
          printf("%s\t%s\n", link_dirs[all_s[i]].c_str(), paths[all_f[i]].c_str());
        else
          printf("%s\t%s\t%s\n", link_dirs[all_s[i]].c_str(), paths[all_f[i]].c_str(),
                 escape_path(sp + off[i - nl], off[i - nl + 1] - off[i - nl]).c_str());
      }
      fflush(stdout);
      fprintf(stderr,
              "links: %zu candidates (%zu at their own path, %zu by content): %llu ok, %llu "
              "checksum, %llu read; %zu source index(es) skipped\n",
              nl + nc, nl, nc, (unsigned long long)st[0], (unsigned long long)st[1],
              (unsigned long long)st[2], skipped);
      for (void* p : {(void*)cf, (void*)cs, (void*)csf, (void*)off, (void*)sp}) cir_free(p);
    } else {
      std::vector<uint8_t> kinds(nl);
      rc = cir_check_links(ctx, index, check_index.size(), dirfds.data(), dirs.data(), dirs.size(),
                           lf, ls, nl, threads, kinds.data(), nullptr, st);
      if (rc) {
        die(rc, files[0].c_str());
        return 2;
      }
      for (size_t i = 0; i < nl; ++i)
        if (kinds[i] == CIR_CHECK_OK && lf[i] < paths.size())
          printf("%s\t%s\n", link_dirs[ls[i]].c_str(), paths[lf[i]].c_str());
      fflush(stdout);
      fprintf(stderr,
              "links: %zu candidates: %llu ok, %llu checksum, %llu read; %zu source index(es) "
              "skipped\n",
              nl, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
              skipped);
    }
    cir_free(lf);
    cir_free(ls);
  } else if (cmd == "candidates") {
    static const uint8_t none = 0;
    std::vector<const uint8_t*> sidx;
    std::vector<size_t> slen;
    for (const std::vector<uint8_t>& v : link_indexes) {
      sidx.push_back(v.empty() ? &none : v.data());
      slen.push_back(v.size());
    }
    uint64_t* lf = nullptr;
    uint32_t* ls = nullptr;
    size_t nl = 0, skipped = 0;
    uint64_t fst[CIR_FILE_SOURCES_STATS_FIELDS];
    rc = cir_file_sources(ctx, check_index.empty() ? &none : check_index.data(), check_index.size(),
                          sidx.data(), slen.data(), sidx.size(), &lf, &ls, &nl, &skipped, fst);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    const std::vector<std::string> paths = index_file_paths(check_index);
    for (size_t i = 0; i < nl; ++i)
      if (lf[i] < paths.size())
        printf("%llu %u %s\n", (unsigned long long)lf[i], ls[i], paths[lf[i]].c_str());
    fflush(stdout);
    fprintf(stderr,
            "candidates: %llu files, %zu candidates, %llu bytes; %llu source index(es) used, %zu "
            "skipped; matched on the %s\n",
            (unsigned long long)fst[0], nl, (unsigned long long)fst[2], (unsigned long long)fst[4],
            skipped, fst[6] ? "device" : "host");
    cir_free(lf);
    cir_free(ls);
  } else if (cmd == "copies") {
    static const uint8_t none = 0;
    const uint8_t* index = check_index.empty() ? &none : check_index.data();
    std::vector<const uint8_t*> sidx;
    std::vector<size_t> slen;
    for (const std::vector<uint8_t>& v : link_indexes) {
      sidx.push_back(v.empty() ? &none : v.data());
      slen.push_back(v.size());
    }
    const std::vector<std::string> paths = index_file_paths(check_index);
    std::vector<uint64_t> skip;
    if (unlinked) {  // the files the same-path rule links are left out
      uint64_t* lf = nullptr;
      uint32_t* ls = nullptr;
      size_t nl = 0;
      uint64_t fst[CIR_FILE_SOURCES_STATS_FIELDS];
      rc = cir_file_sources(ctx, index, check_index.size(), sidx.data(), slen.data(), sidx.size(),
                            &lf, &ls, &nl, nullptr, fst);
      if (rc) {
        die(rc, files[0].c_str());
        return 2;
      }
      skip.assign(paths.size() / 64 + 1, 0);
      for (size_t i = 0; i < nl; ++i)
        if (lf[i] < paths.size()) skip[lf[i] >> 6] |= 1ull << (lf[i] & 63);
      cir_free(lf);
      cir_free(ls);
    }
    uint64_t* cf = nullptr;
    uint32_t* cs = nullptr;
    uint64_t* csf = nullptr;
    uint64_t* off = nullptr;
    uint8_t* sp = nullptr;
    size_t nc = 0, skipped = 0;
    uint64_t cst[CIR_FILE_COPIES_STATS_FIELDS];
    rc = cir_file_copies(ctx, index, check_index.size(), sidx.data(), slen.data(), sidx.size(),
                         unlinked ? skip.data() : nullptr, &cf, &cs, &csf, &off, &sp, &nc, &skipped,
                         cst);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    for (size_t i = 0; i < nc; ++i)
      if (cf[i] < paths.size())
        printf("%llu %u %llu %s %s\n", (unsigned long long)cf[i], cs[i], (unsigned long long)csf[i],
               paths[cf[i]].c_str(), escape_path(sp + off[i], off[i + 1] - off[i]).c_str());
    fflush(stdout);
    fprintf(stderr,
            "copies: %llu files, %llu left out, %zu candidates (%llu at their own path), %llu bytes; "
            "%llu source index(es) used, %zu skipped; matched on the %s\n",
            (unsigned long long)cst[0], (unsigned long long)cst[8], nc, (unsigned long long)cst[9],
            (unsigned long long)cst[2], (unsigned long long)cst[4], skipped,
            cst[6] ? "device" : "host");
    for (void* p : {(void*)cf, (void*)cs, (void*)csf, (void*)off, (void*)sp}) cir_free(p);
  } else if (cmd == "plan") {
    static const uint8_t none = 0;
    const uint8_t* index = check_index.empty() ? &none : check_index.data();
    std::vector<const uint8_t*> sidx;
    std::vector<size_t> slen;
    for (const std::vector<uint8_t>& v : link_indexes) {
      sidx.push_back(v.empty() ? &none : v.data());
      slen.push_back(v.size());
    }
    uint64_t* lf = nullptr;
    uint32_t* ls = nullptr;
    uint64_t* cf = nullptr;
    uint32_t* cs = nullptr;
    uint64_t* csf = nullptr;
    uint64_t* off = nullptr;
    uint8_t* sp = nullptr;
    uint64_t* ext = nullptr;
    uint64_t* rep = nullptr;
    uint64_t* fetch = nullptr;
    size_t nl = 0, nc = 0, ne = 0, nr = 0, skipped = 0;
    uint64_t nblk = 0;
    uint64_t pst[CIR_PLAN_STATS_FIELDS];
    rc = cir_fetch_plan(ctx, index, check_index.size(), sidx.data(), slen.data(), sidx.size(),
                        nullptr, nullptr, &lf, &ls, &nl, &cf, &cs, &csf, &off, &sp, &nc, &ext, &ne,
                        &rep, &nr, &fetch, &nblk, &skipped, pst);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    // every byte of a file entry is in exactly one class (nothing is denied or held here)
    std::vector<uint64_t> sizes;
    index_file_paths(check_index, &sizes);
    uint64_t total = 0, left = 0;
    for (uint64_t s : sizes) total += s;
    for (uint64_t w = 0; w < (nblk + 63) / 64; ++w) left += (uint64_t)__builtin_popcountll(fetch[w]);
    const uint64_t placed = pst[2] + pst[8 + 2] + pst[18 + 2] + pst[28 + 2];
    printf("link %zu files at their own path, %llu bytes\n", nl, (unsigned long long)pst[2]);
    printf("link %zu files by content, %llu bytes\n", nc, (unsigned long long)pst[8 + 2]);
    printf("copy %zu extents from older images, %llu blocks, %llu bytes\n", ne,
           (unsigned long long)pst[18 + 1], (unsigned long long)pst[18 + 2]);
    printf("copy %zu extents inside the image, %llu blocks, %llu bytes\n", nr,
           (unsigned long long)pst[28 + 1], (unsigned long long)pst[28 + 2]);
    printf("fetch %llu blocks of %llu, %llu bytes\n", (unsigned long long)left,
           (unsigned long long)nblk, (unsigned long long)(total >= placed ? total - placed : 0));
    fflush(stdout);
    fprintf(stderr,
            "plan: %llu files, %llu blocks; %llu source index(es) used, %zu skipped; planned on the "
            "%s\n",
            (unsigned long long)pst[0], (unsigned long long)nblk, (unsigned long long)pst[4], skipped,
            pst[42] ? "device" : "host");
    for (void* p : {(void*)lf, (void*)ls, (void*)cf, (void*)cs, (void*)csf, (void*)off, (void*)sp,
                    (void*)ext, (void*)rep, (void*)fetch})
      cir_free(p);
  } else if (cmd == "sources") {
    static const uint8_t none = 0;
    std::vector<const uint8_t*> sidx;
    std::vector<size_t> slen;
    for (const std::vector<uint8_t>& v : link_indexes) {
      sidx.push_back(v.empty() ? &none : v.data());
      slen.push_back(v.size());
    }
    if (extents) {
      uint64_t* ext = nullptr;
      uint64_t* fetch = nullptr;
      size_t next = 0, eskipped = 0;
      uint64_t enblk = 0;
      uint64_t est[CIR_EXTENTS_STATS_FIELDS];
      rc = cir_block_extents(ctx, check_index.empty() ? &none : check_index.data(),
                             check_index.size(), sidx.data(), slen.data(), sidx.size(), nullptr,
                             &ext, &next, &fetch, &enblk, &eskipped, est);
      if (rc) {
        die(rc, files[0].c_str());
        return 2;
      }
      printf("extents: %llu blocks, %llu found in %zu extent(s), %llu bytes found, %llu left to "
             "fetch; %llu source index(es) used, %zu skipped\n",
             (unsigned long long)enblk, (unsigned long long)est[1], next,
             (unsigned long long)est[2], (unsigned long long)est[9], (unsigned long long)est[4],
             eskipped);
      uint64_t ibs = 0;
      const std::vector<std::string> paths = index_file_paths(check_index, nullptr, &ibs);
      std::vector<std::vector<std::string>> spaths(link_indexes.size());
      std::vector<bool> loaded(link_indexes.size(), false);
      for (size_t k = 0; k < next; ++k) {
        const uint64_t* e = ext + CIR_EXTENT_WORDS * k;
        const uint64_t s = e[4];
        if (e[2] >= paths.size() || s >= link_indexes.size()) continue;
        if (!loaded[s]) {
          spaths[s] = index_file_paths(link_indexes[s]);
          loaded[s] = true;
        }
        if (e[5] >= spaths[s].size()) continue;
        printf("%s %llu %llu %llu %s %llu\n", paths[e[2]].c_str(),
               (unsigned long long)(e[3] * ibs), (unsigned long long)e[7], (unsigned long long)s,
               spaths[s][e[5]].c_str(), (unsigned long long)(e[6] * ibs));
      }
      fflush(stdout);
      cir_free(ext);
      cir_free(fetch);
      return 0;
    }
    uint32_t* bsrc = nullptr;
    uint64_t* bfile = nullptr;
    uint64_t* bblock = nullptr;
    uint64_t nblk = 0;
    size_t skipped = 0;
    uint64_t st[CIR_SOURCES_STATS_FIELDS];
    rc = cir_block_sources(ctx, check_index.empty() ? &none : check_index.data(),
                           check_index.size(), sidx.data(), slen.data(), sidx.size(), nullptr,
                           &bsrc, &bfile, &bblock, &nblk, &skipped, st);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    printf("sources: %llu blocks, %llu found, %llu bytes found; %llu source index(es) used, %zu "
           "skipped\n",
           (unsigned long long)nblk, (unsigned long long)st[1], (unsigned long long)st[2],
           (unsigned long long)st[4], skipped);
    if (list_blocks) {
      std::vector<uint64_t> sizes;
      uint64_t ibs = 0;
      const std::vector<std::string> paths = index_file_paths(check_index, &sizes, &ibs);
      std::vector<std::vector<std::string>> spaths(link_indexes.size());
      std::vector<bool> loaded(link_indexes.size(), false);
      uint64_t g = 0;
      for (size_t i = 0; i < paths.size() && ibs; ++i) {
        const uint64_t n = (sizes[i] + ibs - 1) / ibs;
        for (uint64_t j = 0; j < n && g + j < nblk; ++j) {
          const uint32_t s = bsrc[g + j];
          if (s == UINT32_MAX || s >= link_indexes.size()) continue;
          if (!loaded[s]) {
            spaths[s] = index_file_paths(link_indexes[s]);
            loaded[s] = true;
          }
          if (bfile[g + j] >= spaths[s].size()) continue;
          printf("%s %llu %llu %u %s %llu\n", paths[i].c_str(), (unsigned long long)(j * ibs),
                 (unsigned long long)std::min<uint64_t>(ibs, sizes[i] - j * ibs), s,
                 spaths[s][bfile[g + j]].c_str(), (unsigned long long)(bblock[g + j] * ibs));
        }
        g += n;
      }
    }
    fflush(stdout);
    cir_free(bsrc);
    cir_free(bfile);
    cir_free(bblock);
  } else if (cmd == "repeats") {
    static const uint8_t none = 0;
    uint64_t* ext = nullptr;
    uint64_t* fetch = nullptr;
    size_t next = 0;
    uint64_t nblk = 0;
    uint64_t st[CIR_REPEATS_STATS_FIELDS];
    rc = cir_block_repeats(ctx, check_index.empty() ? &none : check_index.data(),
                           check_index.size(), nullptr, nullptr, &ext, &next, &fetch, &nblk, st);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    printf("repeats: %llu blocks, %llu repeat in %zu extent(s), %llu bytes, %llu left to fetch\n",
           (unsigned long long)nblk, (unsigned long long)st[1], next, (unsigned long long)st[2],
           (unsigned long long)st[9]);
    uint64_t ibs = 0;
    const std::vector<std::string> paths = index_file_paths(check_index, nullptr, &ibs);
    for (size_t k = 0; k < next; ++k) {
      const uint64_t* e = ext + CIR_EXTENT_WORDS * k;
      if (e[2] >= paths.size() || e[5] >= paths.size()) continue;
      printf("%s %llu %llu %llu %s %llu\n", paths[e[2]].c_str(), (unsigned long long)(e[3] * ibs),
             (unsigned long long)e[7], (unsigned long long)e[4], paths[e[5]].c_str(),
             (unsigned long long)(e[6] * ibs));
    }
    fflush(stdout);
    cir_free(ext);
    cir_free(fetch);
  } else if (cmd == "sketch") {
    static const uint8_t none = 0;
    uint8_t* blob = nullptr;
    size_t blob_len = 0;
    uint64_t st[CIR_SKETCH_STATS_FIELDS];
    rc = cir_index_sketch(ctx, check_index.empty() ? &none : check_index.data(),
                          check_index.size(), sketch_k, &blob, &blob_len, st);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    FILE* out = out_path.empty() ? stdout : fopen(out_path.c_str(), "wb");
    if (!out) {
      perror(out_path.c_str());
      return 1;
    }
    const bool bad = fwrite(blob, 1, blob_len, out) != blob_len || fflush(out) != 0;
    if (out != stdout && fclose(out) != 0) {
      perror(out_path.c_str());
      return 1;
    }
    if (bad) {
      perror(out_path.empty() ? "stdout" : out_path.c_str());
      return 1;
    }
    cir_free(blob);
    fprintf(stderr, "sketch: %llu keys of %llu blocks, %zu bytes, sketched on the %s\n",
            (unsigned long long)st[3], (unsigned long long)st[2], blob_len,
            st[0] ? "device" : "host");
  } else if (cmd == "rank") {
    // an index among the arguments is replaced by its sketch
    for (size_t i = 0; i < link_indexes.size(); ++i) {
      std::vector<uint8_t>& data = link_indexes[i];
      if (is_sketch(data)) continue;
      uint8_t* blob = nullptr;
      size_t blob_len = 0;
      uint64_t st[CIR_SKETCH_STATS_FIELDS];
      static const uint8_t none = 0;
      rc = cir_index_sketch(ctx, data.empty() ? &none : data.data(), data.size(), sketch_k, &blob,
                            &blob_len, st);
      if (rc && i == 0) {
        die(rc, files[0].c_str());
        return 2;
      }
      if (rc) {  // (a source that does not parse is left out, as the planning calls leave it)
        data.clear();
        continue;
      }
      data.assign(blob, blob + blob_len);
      cir_free(blob);
    }
    const size_t nsrc = link_indexes.size() - 1;
    std::vector<const uint8_t*> sp(nsrc);
    std::vector<size_t> sl(nsrc);
    for (size_t i = 0; i < nsrc; ++i) {
      sp[i] = link_indexes[i + 1].empty() ? nullptr : link_indexes[i + 1].data();
      sl[i] = link_indexes[i + 1].size();
    }
    std::vector<uint64_t> order(nsrc), shared(nsrc), examined(nsrc);
    size_t nranked = 0, nskipped = 0;
    rc = cir_sketch_rank(link_indexes[0].data(), link_indexes[0].size(), sp.data(), sl.data(), nsrc,
                         order.data(), shared.data(), examined.data(), &nranked, &nskipped);
    if (rc) {
      die(rc, files[0].c_str());
      return 2;
    }
    for (size_t i = 0; i < nranked; ++i)
      printf("%llu %llu %llu %s\n", (unsigned long long)order[i], (unsigned long long)shared[i],
             (unsigned long long)examined[i], files[order[i] + 1].c_str());
    fflush(stdout);
    fprintf(stderr, "rank: %zu source(s) ranked, %zu left out\n", nranked, nskipped);
  } else if (cmd == "sync") {
    if (jobs.empty()) {
      usage();
      return 2;
    }
    cir_indexes* idx = cir_indexes_new();
    cir_blocks* blocks = cir_blocks_new();
    for (const Job& j : jobs) {
      const auto t0 = std::chrono::steady_clock::now();
      const char* dirs[1] = {j.src.c_str()};
      const char* pre[1] = {"/"};
      uint8_t* index = nullptr;
      size_t len = 0;
      rc = cir_scan_v1(ctx, dirs, pre, 1, bs, CIR_HASH_BLAKE2B_256, threads, &index, &len);
      if (rc) return die(rc, ("error indexing dir " + j.src).c_str());
      uint8_t id[64];
      size_t idl = 0;
      rc = cir_indexes_register(idx, index, len, id, &idl);
      if (rc) return die(rc, "register_index");
      rc = cir_blocks_register_dir(blocks, j.src.c_str(), index, len);
      if (rc) return die(rc, "register_dir");
      const double s =
          std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      printf("%s %s %s %s\n", hex(id, idl).c_str(), j.kind.c_str(), j.dest.c_str(),
             j.src.c_str());
      fprintf(stderr, "Indexed %s (%zu index bytes, %zu blocks) in %.3f s\n", j.src.c_str(), len,
              cir_blocks_len(blocks), s);
      if (!index_dir.empty()) {
        const std::string p = index_dir + "/" + hex(id, idl) + ".ds1";
        FILE* f = fopen(p.c_str(), "wb");
        // (a full disk can surface only at fclose, when the buffer is written)
        const bool ok = f && fwrite(index, 1, len, f) == len;
        if (!ok || (f && fclose(f) != 0)) {
          perror(p.c_str());
          if (!ok && f) fclose(f);
          return 1;
        }
      }
      cir_free(index);
    }
    cir_blocks_free(blocks);
    cir_indexes_free(idx);
  } else {
    usage();
    return 2;
  }
  // A one-shot process: every result is written and every GPU call has
  // completed (the scan synchronises before it returns), so the context's
  // teardown -- freeing the pinned staging, streams and device buffers one by
  // one, ~17 ms of a ~0.2 s run (profiles/r04/cli_startup.log) -- is left to
  // process exit, as the error paths above already do.  CIR_CLI_TEARDOWN=1
  // destroys the context first (leak checks).  Under a profiler (rocprofv3
  // sets ROCP_TOOL_LIBRARIES / ROCPROF_* for its tool library) the process
  // still skips cir_destroy but returns normally, so the exit handlers run
  // and the tool writes its trace at finalisation.
  const char* td = getenv("CIR_CLI_TEARDOWN");
  if (!(td && *td && strcmp(td, "0") != 0)) {
    if (fflush(stdout) != 0) {
      perror("stdout");
      return 1;
    }
    if (profiled()) {
      if (trace) fprintf(stderr, "ciruela-index: profiler present: normal exit, no cir_destroy\n");
      return 0;
    }
    if (trace) fprintf(stderr, "ciruela-index: exit without cir_destroy\n");
    fflush(stderr);
    _exit(0);
  }
  const auto t_destroy = std::chrono::steady_clock::now();
  if (ctx) cir_destroy(ctx);
  if (trace) fprintf(stderr, "ciruela-index: cir_destroy %.1f ms\n", ms_since(t_destroy));
  return 0;
}
