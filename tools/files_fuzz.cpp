// Seeded fuzz of the file-record rule (ciruela_amd/csrc/files.hpp: scan_host,
// next_byte, path_hash, same_path, fold_term, host_match -- the text the
// kernels of files.hip compile) against dirsig::parse and against
// candidates_impl (links.cpp, the host rule of cir_link_candidates).
// Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iciruela_amd/csrc \
//       tools/files_fuzz.cpp ciruela_amd/csrc/dirsig.cpp ciruela_amd/csrc/links.cpp \
//       -o build/files_fuzz
// and run it; tests/test_file_sources_cpu.py does.  Every case holds the
// arena, the records, the digests and the results in heap buffers of exactly
// their size, so a read or a write one element outside is an AddressSanitizer
// report.
//
// Per case: a new index and 0-4 older ones over a small universe of
// directories, names (escaped and unescaped spellings of the same bytes),
// sizes and digests, so that equal paths, duplicate paths inside a source,
// exe and size mismatches and near-equal digest lists abound; one text in
// five is mutated.
//   1. every text idxscan::scan_host accepts: files::scan_host counts the same
//      files and blocks, dirsig::parse accepts it, and every record decodes to
//      the parser's path, exe flag, size and first block;
//   2. when every text is accepted: files::host_match over one arena equals
//      candidates_impl, and a pool digest changed behind the folds gives
//      kCollision exactly when it belongs to a candidate.
//
// usage: files_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dirsig.hpp"
#include "files.hpp"
#include "idxscan.hpp"
#include "links.hpp"

using namespace cir;

// (what links.cpp takes from the runtime)
namespace cir {
int fail(int code, const std::string&) { return code; }
int boundary_error() noexcept { return -1; }
}  // namespace cir

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

static uint64_t g_case, g_texts, g_joins, g_cands, g_collisions;
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      fprintf(stderr, "files_fuzz: %s:%d: %s (case %llu)\n", __FILE__, __LINE__, #c, \
              (unsigned long long)g_case);                                      \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

// A heap array of exactly n elements (none at all for n == 0).
template <typename T>
struct Exact {
  T* p;
  uint64_t n;
  explicit Exact(uint64_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

static const char* kDirs[] = {"/", "/d", "/\\x64", "/d/e", "/sp\\x20ace", "/d/"};
static const char* kNames[] = {"a", "\\x61", "b", "A", "\\x41", "long-name.txt", "x\\x5cy", "\\xffq"};

static std::string hex_of(uint64_t id) {  // a digest from a small universe
  char buf[80];
  uint64_t s = id * 0x9e3779b97f4a7c15ULL + 1;
  std::string out;
  for (int i = 0; i < 4; ++i) {
    s ^= s >> 29;
    s *= 0xbf58476d1ce4e5b9ULL;
    snprintf(buf, sizeof buf, "%016llx", (unsigned long long)s);
    out += buf;
  }
  return out;
}

static std::string make_index(uint64_t bs) {
  std::string t = "DIRSIGNATURE.v1 blake2b/256 block_size=" + std::to_string(bs) + "\n";
  const int ndirs = 1 + (int)(rnd() % 3);
  for (int d = 0; d < ndirs; ++d) {
    t += d == 0 && rnd() % 4 ? "/" : kDirs[rnd() % 6];
    t += "\n";
    const int n = (int)(rnd() % 5);
    for (int f = 0; f < n; ++f) {
      t += "  ";
      t += kNames[rnd() % 8];
      if (rnd() % 9 == 0) {
        t += " s target\n";
        continue;
      }
      const uint64_t nb = rnd() % 4;
      const uint64_t size = nb == 0 ? 0 : (nb - 1) * bs + 1 + rnd() % bs;
      t += rnd() % 4 == 0 ? " x " : " f ";
      t += std::to_string(size);
      for (uint64_t k = 0; k < nb; ++k) t += " " + hex_of(rnd() % 3);
      t += "\n";
    }
  }
  t += hex_of(99) + "\n";
  if (rnd() % 5 == 0 && t.size() > 50) {  // one mutation
    const size_t at = 45 + rnd() % (t.size() - 50);
    switch (rnd() % 4) {
      case 0: t[at] = (char)(rnd() & 0xff); break;
      case 1: t.insert(at, " "); break;
      case 2: t.erase(at, 1); break;
      default: t.insert(at, "\\x2f"); break;
    }
  }
  return t;
}

static std::string decode(const uint8_t* t, uint64_t len, uint64_t off) {
  std::string out;
  uint64_t i = off;
  const uint64_t lim = files::walk_lim(off, len);
  for (int c; (c = files::next_byte(t, &i, lim)) >= 0;) out.push_back((char)c);
  return out;
}

struct Parsed {
  bool ok = false;
  size_t body_off = 0, body_end = 0;
  uint64_t nfiles = 0, nblk = 0;
};

// Step 1 for one text that sits at arena[off, off + len).
static Parsed check_text(const uint8_t* arena, uint64_t arena_len, uint64_t off, uint64_t len,
                         uint64_t bs) {
  Parsed r;
  const uint8_t* t = arena + off;
  dirsig::Header h;
  std::string err;
  if (!dirsig::frame(t, len, &h, &r.body_off, &r.body_end, &err) || h.block_size != bs) return r;
  const idxscan::Counts ic = idxscan::scan_host(t, r.body_off, r.body_end, bs, nullptr, nullptr);
  const files::Counts fc = files::scan_host(t, r.body_off, r.body_end, bs, 0, 0, nullptr);
  CHECK(fc.declined == ic.declined || ic.declined != idxscan::kBad);  // (tokens are idxscan's)
  if (ic.declined != idxscan::kBad) return r;
  CHECK(fc.files == ic.files && fc.blocks == ic.blocks);
  dirsig::Index idx;
  CHECK(dirsig::parse(t, len, &idx, &err));
  Exact<files::Rec> rec(fc.files);
  const uint64_t bias = 1000;
  files::scan_host(t, r.body_off, r.body_end, bs, off, bias, rec.p);
  uint64_t f = 0, blk = 0;
  for (const dirsig::Entry& e : idx.entries) {
    if (e.kind != dirsig::EntryKind::kFile) continue;
    CHECK(f < fc.files);
    const files::Rec& x = rec.p[f];
    const std::string dir = decode(arena, arena_len, x.dir_off), name = decode(arena, arena_len, x.name_off);
    CHECK((dir == "/" ? "/" + name : dir + "/" + name) == e.path);
    CHECK(x.size == e.size && ((x.first & files::kExeBit) != 0) == e.exe);
    CHECK((x.first & ~files::kExeBit) == blk + bias);
    blk += e.hashes.size() / 32;
    ++f;
  }
  CHECK(f == fc.files && blk == fc.blocks);
  r.ok = true;
  ++g_texts;
  r.nfiles = fc.files;
  r.nblk = fc.blocks;
  return r;
}

static void one_case() {
  const uint64_t bs = 1 + rnd() % 5;
  const size_t nsrc = rnd() % 5;
  std::vector<std::string> texts;
  for (size_t k = 0; k <= nsrc; ++k) {
    texts.push_back(make_index(bs));
    if (k && rnd() % 3 == 0) texts.back() = texts[rnd() % k];  // a copy of an earlier text
  }
  // one arena, 16-byte aligned offsets, exactly sized
  std::vector<uint64_t> off;
  uint64_t total = 0;
  for (const std::string& t : texts) {
    off.push_back(total);
    total += (t.size() + 15) & ~(size_t)15;
  }
  total = off.back() + texts.back().size();
  Exact<uint8_t> arena(total);
  for (size_t k = 0; k <= nsrc; ++k) memcpy(arena.p + off[k], texts[k].data(), texts[k].size());
  std::vector<Parsed> ps;
  bool all = true;
  for (size_t k = 0; k <= nsrc; ++k) {
    ps.push_back(check_text(arena.p, total, off[k], texts[k].size(), bs));
    all = all && ps.back().ok;
  }
  if (!all) return;
  // step 2: text 0 is the new index, the others the sources in order
  uint64_t pool_files = 0, pool_blocks = 0;
  std::vector<uint64_t> src_first;
  for (size_t k = 1; k <= nsrc; ++k) {
    src_first.push_back(pool_files);
    pool_files += ps[k].nfiles;
    pool_blocks += ps[k].nblk;
  }
  src_first.push_back(pool_files);
  Exact<files::Rec> nrec(ps[0].nfiles), prec(pool_files);
  Exact<uint8_t> ndig(32 * ps[0].nblk), pdig(32 * pool_blocks), pver(32 * pool_blocks);
  idxscan::scan_host(arena.p + off[0], ps[0].body_off, ps[0].body_end, bs, ndig.p, nullptr);
  files::scan_host(arena.p + off[0], ps[0].body_off, ps[0].body_end, bs, off[0], 0, nrec.p);
  uint64_t fa = 0, ba = 0;
  for (size_t k = 1; k <= nsrc; ++k) {
    idxscan::scan_host(arena.p + off[k], ps[k].body_off, ps[k].body_end, bs,
                       ps[k].nblk ? pdig.p + 32 * ba : nullptr, nullptr);
    files::scan_host(arena.p + off[k], ps[k].body_off, ps[k].body_end, bs, off[k], ba,
                     ps[k].nfiles ? prec.p + fa : nullptr);
    fa += ps[k].nfiles;
    ba += ps[k].nblk;
  }
  if (pool_blocks) memcpy(pver.p, pdig.p, 32 * pool_blocks);
  const files::Side need{arena.p, total, nrec.p, ps[0].nfiles, ndig.p, ps[0].nblk};
  const files::Side pool{arena.p, total, prec.p, pool_files, pdig.p, pool_blocks};
  Exact<uint32_t> csrc(ps[0].nfiles);
  Exact<uint64_t> cfile(ps[0].nfiles);
  uint64_t res[files::kResFields];
  files::host_match(need, pool, src_first.data(), nsrc, bs, pver.p, rnd(), csrc.p, cfile.p, res);
  CHECK(res[0] == files::kOk && res[3] == ps[0].nfiles);
  // the host rule
  std::vector<const uint8_t*> sp;
  std::vector<size_t> sl;
  for (size_t k = 1; k <= nsrc; ++k) {
    sp.push_back(arena.p + off[k]);
    sl.push_back(texts[k].size());
  }
  uint64_t* fo = nullptr;
  uint32_t* so = nullptr;
  size_t n = 0, skipped = 0;
  uint64_t counts[5];
  CHECK(candidates_impl(arena.p + off[0], texts[0].size(), sp.data(), sl.data(), nsrc, &fo, &so, &n,
                        &skipped, counts) == 0);
  CHECK(skipped == 0 && counts[0] == ps[0].nfiles && counts[3] == pool_files);
  CHECK(res[1] == n && res[2] == counts[2]);
  size_t at = 0;
  for (uint64_t i = 0; i < ps[0].nfiles; ++i) {
    if (csrc.p[i] == files::kNoSrc) {
      CHECK(cfile.p[i] == files::kNoFile);
      continue;
    }
    CHECK(at < n && fo[at] == i && so[at] == csrc.p[i]);
    CHECK(cfile.p[i] < ps[1 + csrc.p[i]].nfiles);
    ++at;
  }
  CHECK(at == n);
  ++g_joins;
  g_cands += n;
  // a digest changed behind the folds: a collision exactly when a candidate holds it
  if (pool_blocks) {
    const uint64_t g = rnd() % pool_blocks;
    pver.p[32 * g + rnd() % 32] ^= 1;
    bool held = false;
    for (uint64_t i = 0; i < ps[0].nfiles; ++i) {
      if (csrc.p[i] == files::kNoSrc) continue;
      const files::Rec& r = prec.p[src_first[csrc.p[i]] + cfile.p[i]];
      const uint64_t first = r.first & ~files::kExeBit;
      held = held || (g >= first && g - first < files::blocks_of(r.size, bs));
    }
    Exact<uint32_t> csrc2(ps[0].nfiles);
    Exact<uint64_t> cfile2(ps[0].nfiles);
    uint64_t res2[files::kResFields];
    files::host_match(need, pool, src_first.data(), nsrc, bs, pver.p, rnd(), csrc2.p, cfile2.p, res2);
    CHECK(res2[0] == (held ? files::kCollision : files::kOk));
    g_collisions += held;
    for (uint64_t i = 0; i < ps[0].nfiles; ++i)  // (the answer does not depend on the seed)
      CHECK(csrc2.p[i] == csrc.p[i] && cfile2.p[i] == cfile.p[i]);
  }
  free(fo);
  free(so);
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (g_case = 0; g_case < cases; ++g_case) one_case();
  fprintf(stderr, "files_fuzz: %llu texts accepted, %llu joins, %llu candidates, %llu collisions\n",
          (unsigned long long)g_texts, (unsigned long long)g_joins, (unsigned long long)g_cands,
          (unsigned long long)g_collisions);
  printf("files_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
