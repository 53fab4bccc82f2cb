// Seeded fuzz of the content-match rule (ciruela_amd/csrc/copies.hpp: skipped,
// home_slot, same_key, host_match -- the text the kernels k_copies_build and
// k_copies_probe of files.hip compile) against a brute-force loop over
// dirsig::parse's entries, and of copies::compact, the host's reading of the
// device's answer.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iciruela_amd/csrc \
//       tools/copies_fuzz.cpp ciruela_amd/csrc/dirsig.cpp -o build/copies_fuzz
// and run it; tests/test_file_copies_cpu.py does.  Every case holds the
// records, the digests, the skip bitmap and the results in heap buffers of
// exactly their size, so a read or a write one element outside is an
// AddressSanitizer report.
//
// Per case: a new index and 0-4 older ones over a small universe of
// directories, names, sizes and digests, so that one content under several
// paths and in several sources, exe and size mismatches, empty files and
// near-equal digest lists abound; a random skip bitmap in every second case.
//   1. copies::host_match (fold + build + probe + verify, no text read: the
//      sides' text pointers are null) equals the brute-force rule: per need
//      file that is not empty and not skipped, the first pool file in pool
//      order with equal exe flag, size and digests; the places are that pool
//      record's offsets and decode to the parser's path;
//   2. another seed gives the same answer;
//   3. a pool digest changed in a second verify array gives kCollision exactly
//      when it belongs to a candidate;
//   4. linkpath::split (linkpath.hpp: the paths cir_check_links_at takes) on a
//      random byte string over '/', '.', NUL and two letters, held in a buffer of
//      exactly its length, against a restatement that goes byte by byte;
//   5. copies::compact (what cir_file_copies and cir_fetch_plan make of the
//      join's downloaded answer) on the answer of 1, the texts laid out as in
//      the device's arena and held in buffers of exactly their length: the
//      candidates, the sources' ordinals and the decoded paths are the
//      parser's, `same` and `left_out` counted here; then one candidate's
//      answer spoilt -- a source ordinal >= used, a file >= the source's
//      files, a place of either side at len, text_off - 1 or ~0 -- must give
//      the out-of-range result, and a place at len - 1 none, with no byte
//      read outside.
//
// usage: copies_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "copies.hpp"
#include "dirsig.hpp"
#include "files.hpp"
#include "idxscan.hpp"
#include "linkpath.hpp"

using namespace cir;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

static uint64_t g_case, g_joins, g_cands, g_collisions, g_moved, g_paths[4], g_compact[3];
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      fprintf(stderr, "copies_fuzz: %s:%d: %s (case %llu)\n", __FILE__, __LINE__, #c, \
              (unsigned long long)g_case);                                       \
      exit(1);                                                                   \
    }                                                                            \
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

static const char* kDirs[] = {"/", "/d", "/v-1", "/v-2", "/sp\\x20ace", "/d/e"};
static const char* kNames[] = {"a", "b", "A", "long-name.txt", "x\\x5cy", "\\xffq", "c\\x20d"};

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
    t += d == 0 ? "/" : kDirs[1 + rnd() % 5];
    t += "\n";
    const int n = (int)(rnd() % 6);
    for (int f = 0; f < n; ++f) {
      t += "  ";
      t += kNames[rnd() % 7];
      if (rnd() % 9 == 0) {
        t += " s target\n";
        continue;
      }
      const uint64_t nb = rnd() % 4;
      const uint64_t size = nb == 0 ? 0 : (nb - 1) * bs + (rnd() % 3 ? bs : 1 + rnd() % bs);
      t += rnd() % 5 == 0 ? " x " : " f ";
      t += std::to_string(size);
      for (uint64_t k = 0; k < nb; ++k) t += " " + hex_of(rnd() % 2);
      t += "\n";
    }
  }
  return t + hex_of(99) + "\n";
}

static std::string decode(const std::string& t, uint64_t off) {
  std::string out;
  uint64_t i = off;
  const uint64_t lim = files::walk_lim(off, t.size());
  for (int c; (c = files::next_byte((const uint8_t*)t.data(), &i, lim)) >= 0;) out.push_back((char)c);
  return out;
}

struct Text {
  std::string t;
  size_t body_off = 0, body_end = 0;
  std::vector<const dirsig::Entry*> files;  // file entries, in index order
  dirsig::Index idx;
  uint64_t nblk = 0;
};

static void parse_text(Text* x, uint64_t bs) {
  dirsig::Header h;
  std::string err;
  const uint8_t* t = (const uint8_t*)x->t.data();
  CHECK(dirsig::frame(t, x->t.size(), &h, &x->body_off, &x->body_end, &err) && h.block_size == bs);
  CHECK(dirsig::parse(t, x->t.size(), &x->idx, &err));
  for (const dirsig::Entry& e : x->idx.entries)
    if (e.kind == dirsig::EntryKind::kFile) {
      x->files.push_back(&e);
      x->nblk += e.hashes.size() / 32;
    }
  const files::Counts c = files::scan_host(t, x->body_off, x->body_end, bs, 0, 0, nullptr);
  CHECK(c.declined == idxscan::kBad && c.files == x->files.size() && c.blocks == x->nblk);
}

// Check 5.  The answer of a join over tx (offsets relative to each text) as the
// device would give it: every offset biased by the text's place in the arena.
static void check_compact(const std::vector<Text>& tx, const files::Rec* nrec, const uint32_t* csrc,
                          const uint64_t* cfile, const uint64_t* cplace, const uint64_t* skip) {
  const size_t used = tx.size() - 1;
  const uint64_t nf = tx[0].files.size();
  std::vector<std::unique_ptr<Exact<uint8_t>>> bytes;
  Exact<copies::PlacedText> pt(used + 1);
  uint64_t at = 16 * (rnd() % 3);
  for (size_t k = 0; k <= used; ++k) {
    const std::string& t = tx[k].t;
    bytes.emplace_back(new Exact<uint8_t>(t.size()));
    memcpy(bytes[k]->p, t.data(), t.size());
    pt.p[k] = {bytes[k]->p, t.size(), at, tx[k].files.size(), (uint32_t)(7 * k + 3)};
    at += (t.size() + 15) & ~(uint64_t)15;
  }
  Exact<files::Rec> nr(nf);
  Exact<uint32_t> cs(nf);
  Exact<uint64_t> cf(nf), cp(copies::kPlaceWords * nf);
  auto reset = [&] {
    for (uint64_t i = 0; i < nf; ++i) {
      nr.p[i] = nrec[i];
      nr.p[i].name_off += pt.p[0].text_off;
      nr.p[i].dir_off += pt.p[0].text_off;
      cs.p[i] = csrc[i];
      cf.p[i] = cfile[i];
      for (int w = 0; w < copies::kPlaceWords; ++w)
        cp.p[2 * i + w] = cplace[2 * i + w] +
                          (csrc[i] == files::kNoSrc ? 0 : pt.p[1 + csrc[i]].text_off);
    }
  };
  auto run = [&](copies::Found* f) {
    return copies::compact(cs.p, cf.p, cp.p, nr.p, nf, pt.p, used, skip, f);
  };
  reset();
  copies::Found f;
  CHECK(run(&f) == copies::kCompacted);
  uint64_t n = 0, same = 0, left = 0;
  std::vector<uint64_t> hits;
  for (uint64_t i = 0; i < nf; ++i) {
    left += copies::skipped(skip, i);
    if (csrc[i] == files::kNoSrc) continue;
    const dirsig::Entry& want = *tx[1 + csrc[i]].files[cfile[i]];
    CHECK(n < f.file.size() && f.file[n] == i && f.src[n] == pt.p[1 + csrc[i]].ordinal &&
          f.src_file[n] == cfile[i]);
    CHECK(f.paths.substr(f.path_off[n], f.path_off[n + 1] - f.path_off[n]) == want.path);
    same += want.path == tx[0].files[i]->path;
    hits.push_back(i);
    ++n;
  }
  CHECK(f.file.size() == n && f.path_off.size() == n + 1 && f.path_off[n] == f.paths.size());
  CHECK(f.same == same && f.left_out == left);
  uint64_t *o_file, *o_sfile, *o_off;
  uint32_t* o_src;
  uint8_t* o_paths;
  CHECK(f.give(&o_file, &o_src, &o_sfile, &o_off, &o_paths));
  CHECK(n ? o_file && o_src && o_sfile && o_off && o_paths && o_off[n] == f.paths.size()
          : !o_file && !o_src && !o_sfile && !o_off && !o_paths);
  for (void* p : {(void*)o_file, (void*)o_src, (void*)o_sfile, (void*)o_off, (void*)o_paths})
    free(p);
  ++g_compact[0];
  if (!n) return;
  // one candidate's answer spoilt, one word at a time
  const uint64_t i = hits[rnd() % n];
  const copies::PlacedText &st = pt.p[1 + csrc[i]], &nt = pt.p[0];
  auto spoilt = [&](copies::Compacted want) {
    copies::Found g;
    CHECK(run(&g) == want);
    ++g_compact[want == copies::kCompacted ? 1 : 2];
    reset();
  };
  cs.p[i] = (uint32_t)(used + rnd() % 3);
  spoilt(copies::kBadSource);
  cs.p[i] = 0xFFFFFFFEu;
  spoilt(copies::kBadSource);
  cf.p[i] = st.nfiles + rnd() % 2;
  spoilt(copies::kBadPlace);
  cf.p[i] = ~0ull;
  spoilt(copies::kBadPlace);
  uint64_t* const words[4] = {&cp.p[2 * i], &cp.p[2 * i + 1], &nr.p[i].name_off, &nr.p[i].dir_off};
  for (int w = 0; w < 4; ++w) {
    const copies::PlacedText& t = w < 2 ? st : nt;
    *words[w] = t.text_off + t.len - 1;  // (the last byte: in range, whatever it decodes to)
    spoilt(copies::kCompacted);
    for (uint64_t bad : {t.text_off + t.len, t.text_off - 1, ~(uint64_t)0}) {
      *words[w] = bad;
      spoilt(copies::kBadPlace);
    }
  }
}

static void one_case() {
  const uint64_t bs = 1 + rnd() % 4;
  const size_t nsrc = rnd() % 5;
  std::vector<Text> tx(nsrc + 1);
  for (size_t k = 0; k <= nsrc; ++k) {
    tx[k].t = make_index(bs);
    if (k && rnd() % 4 == 0) tx[k].t = tx[rnd() % k].t;  // a copy of an earlier text
  }
  for (Text& x : tx) parse_text(&x, bs);
  uint64_t pool_files = 0, pool_blocks = 0;
  std::vector<uint64_t> src_first;
  for (size_t k = 1; k <= nsrc; ++k) {
    src_first.push_back(pool_files);
    pool_files += tx[k].files.size();
    pool_blocks += tx[k].nblk;
  }
  src_first.push_back(pool_files);
  const uint64_t nf = tx[0].files.size(), nb = tx[0].nblk;
  Exact<files::Rec> nrec(nf), prec(pool_files);
  Exact<uint8_t> ndig(32 * nb), pdig(32 * pool_blocks), pver(32 * pool_blocks);
  auto text = [&](size_t k) { return (const uint8_t*)tx[k].t.data(); };
  idxscan::scan_host(text(0), tx[0].body_off, tx[0].body_end, bs, ndig.p, nullptr);
  files::scan_host(text(0), tx[0].body_off, tx[0].body_end, bs, 0, 0, nrec.p);
  uint64_t fa = 0, ba = 0;
  for (size_t k = 1; k <= nsrc; ++k) {  // (offsets stay relative to the source's own text)
    idxscan::scan_host(text(k), tx[k].body_off, tx[k].body_end, bs,
                       tx[k].nblk ? pdig.p + 32 * ba : nullptr, nullptr);
    files::scan_host(text(k), tx[k].body_off, tx[k].body_end, bs, 0, ba,
                     tx[k].files.empty() ? nullptr : prec.p + fa);
    fa += tx[k].files.size();
    ba += tx[k].nblk;
  }
  if (pool_blocks) memcpy(pver.p, pdig.p, 32 * pool_blocks);
  const bool with_skip = rnd() % 2;
  Exact<uint64_t> skip(with_skip ? (nf + 63) / 64 : 0);
  for (uint64_t i = 0; i < nf && with_skip; ++i)
    if (rnd() % 4 == 0) skip.p[i >> 6] |= 1ull << (i & 63);
  const files::Side need{nullptr, 0, nrec.p, nf, ndig.p, nb};
  const files::Side pool{nullptr, 0, prec.p, pool_files, pdig.p, pool_blocks};
  Exact<uint32_t> csrc(nf);
  Exact<uint64_t> cfile(nf), cplace(copies::kPlaceWords * nf);
  uint64_t res[files::kResFields];
  copies::host_match(need, pool, src_first.data(), nsrc, bs, skip.p, pver.p, rnd(), csrc.p, cfile.p,
                     cplace.p, res);
  CHECK(res[0] == files::kOk && res[3] == nf);
  // the brute-force rule over the parsed entries
  uint64_t n = 0, bytes = 0;
  for (uint64_t i = 0; i < nf; ++i) {
    const dirsig::Entry& e = *tx[0].files[i];
    uint32_t ws = files::kNoSrc;
    uint64_t wf = files::kNoFile;
    const bool takes_part = e.size != 0 && !(with_skip && ((skip.p[i >> 6] >> (i & 63)) & 1));
    for (size_t k = 1; k <= nsrc && takes_part && ws == files::kNoSrc; ++k)
      for (uint64_t j = 0; j < tx[k].files.size(); ++j) {
        const dirsig::Entry& p = *tx[k].files[j];
        if (p.size == e.size && p.exe == e.exe && p.hashes == e.hashes) {
          ws = (uint32_t)(k - 1);
          wf = j;
          break;
        }
      }
    CHECK(csrc.p[i] == ws && cfile.p[i] == wf);
    if (ws == files::kNoSrc) {
      CHECK(cplace.p[2 * i] == copies::kNoPlace && cplace.p[2 * i + 1] == copies::kNoPlace);
      continue;
    }
    const files::Rec& r = prec.p[src_first[ws] + wf];
    CHECK(cplace.p[2 * i] == r.name_off && cplace.p[2 * i + 1] == r.dir_off);
    const std::string dir = decode(tx[1 + ws].t, r.dir_off), name = decode(tx[1 + ws].t, r.name_off);
    const std::string path = dir == "/" ? "/" + name : dir + "/" + name;
    CHECK(path == tx[1 + ws].files[wf]->path);
    g_moved += path != e.path;
    ++n;
    bytes += e.size;
  }
  CHECK(res[1] == n && res[2] == bytes);
  ++g_joins;
  g_cands += n;
  check_compact(tx, nrec.p, csrc.p, cfile.p, cplace.p, skip.p);
  // a digest changed behind the folds: a collision exactly when a candidate holds it
  if (pool_blocks) {
    const uint64_t g = rnd() % pool_blocks;
    pver.p[32 * g + rnd() % 32] ^= 1;
    bool held = false;
    for (uint64_t i = 0; i < nf; ++i) {
      if (csrc.p[i] == files::kNoSrc) continue;
      const files::Rec& r = prec.p[src_first[csrc.p[i]] + cfile.p[i]];
      const uint64_t first = r.first & ~files::kExeBit;
      held = held || (g >= first && g - first < files::blocks_of(r.size, bs));
    }
    Exact<uint32_t> csrc2(nf);
    Exact<uint64_t> cfile2(nf), cplace2(copies::kPlaceWords * nf);
    uint64_t res2[files::kResFields];
    copies::host_match(need, pool, src_first.data(), nsrc, bs, skip.p, pver.p, rnd(), csrc2.p,
                       cfile2.p, cplace2.p, res2);
    CHECK(res2[0] == (held ? files::kCollision : files::kOk));
    g_collisions += held;
    for (uint64_t i = 0; i < nf; ++i)  // (the answer does not depend on the seed)
      CHECK(csrc2.p[i] == csrc.p[i] && cfile2.p[i] == cfile.p[i] &&
            cplace2.p[2 * i] == cplace.p[2 * i] && cplace2.p[2 * i + 1] == cplace.p[2 * i + 1]);
  }
}

// The rule of linkpath.hpp, one byte at a time: components end at a '/' or at
// the end; empty ones are dropped; "." or ".." anywhere, or no component in a
// non-empty path, is invalid; else a NUL anywhere in a component is kNul.
static linkpath::Verdict restate_split(const uint8_t* p, size_t n, std::vector<std::string>* comps) {
  comps->clear();
  if (n == 0) return linkpath::kOwn;
  std::string cur;
  bool dots = false, nul = false;
  for (size_t i = 0; i <= n; ++i) {
    if (i < n && p[i] != '/') {
      cur.push_back((char)p[i]);
      nul = nul || p[i] == 0;
      continue;
    }
    if (cur.empty()) continue;
    dots = dots || cur == "." || cur == "..";
    comps->push_back(cur);
    cur.clear();
  }
  if (dots || comps->empty()) return linkpath::kInvalid;
  return nul ? linkpath::kNul : linkpath::kOk;
}

static void one_path() {
  static const uint8_t kBytes[] = {'/', '/', '.', '.', 'a', 'b', 0};
  const size_t n = rnd() % 4 == 0 ? rnd() % 3 : rnd() % 14;
  Exact<uint8_t> p(n);
  for (size_t i = 0; i < n; ++i) p.p[i] = kBytes[rnd() % (rnd() % 8 ? 6 : 7)];
  std::vector<std::string> got, want;
  const linkpath::Verdict v = linkpath::split(p.p, n, &got), w = restate_split(p.p, n, &want);
  CHECK(v == w);
  if (v == linkpath::kOk || v == linkpath::kNul) CHECK(got == want);
  ++g_paths[v];
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  for (g_case = 0; g_case < cases; ++g_case) {
    one_case();
    one_path();
  }
  fprintf(stderr,
          "copies_fuzz: %llu joins, %llu candidates (%llu at another path), %llu collisions; paths: "
          "%llu own, %llu ok, %llu invalid, %llu with a NUL; compact: %llu answers, %llu spoilt "
          "in range, %llu out of range\n",
          (unsigned long long)g_joins, (unsigned long long)g_cands, (unsigned long long)g_moved,
          (unsigned long long)g_collisions, (unsigned long long)g_paths[0],
          (unsigned long long)g_paths[1], (unsigned long long)g_paths[2],
          (unsigned long long)g_paths[3], (unsigned long long)g_compact[0],
          (unsigned long long)g_compact[1], (unsigned long long)g_compact[2]);
  printf("copies_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
