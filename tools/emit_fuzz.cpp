// The emit rule (ciruela_amd/csrc/emit.hpp) under ASan + UBSan: a stand-alone
// host program, no device code.
//
//   emit_fuzz [cases] [seed]
//
// Per case a seeded random file list over a small alphabet of components (so
// that duplicates, file / directory conflicts and invalid paths occur):
//   * validity is decided independently by inserting every path into a tree of
//     std::map, and emit::build must agree;
//   * for a valid list the body is built by a plain recursive string builder
//     over that tree (directory line, files by name, subdirectories by name)
//     and compared with emit::emit_host (fill16) and, byte by byte, with
//     emit::byte_at, the zero padding up to 16 included; the pieces must tile
//     the body;
//   * then the tables are damaged (ranges outside the arrays, out_off ascending
//     still) and fill16 must agree with byte_at, yield zero bytes for the bad
//     pieces and count them exactly.
// Every table lives in a heap buffer of exactly its size, so a read past an
// array is a report.  Exit status 0 and "emit_fuzz: N cases ok" on stdout; the
// totals go to stderr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "dirsig.hpp"
#include "emit.hpp"

using namespace cir;

namespace {

struct Node {
  bool is_file = false;
  bool exe = false;
  uint64_t size = 0, first = 0;
  std::map<std::string, std::unique_ptr<Node>> kids;
};

struct Totals {
  uint64_t files = 0, dir_lines = 0, blocks = 0, body = 0, invalid = 0, bad_pieces = 0;
} tot;

[[noreturn]] void die(const char* what, uint64_t c) {
  fprintf(stderr, "emit_fuzz: case %llu: %s\n", (unsigned long long)c, what);
  exit(1);
}

// the reference walk: false when the path is invalid or conflicts
bool insert(Node* root, const std::string& path, bool exe, uint64_t size, uint64_t first) {
  if (path.size() < 2 || path[0] != '/' || path.find('\0') != std::string::npos) return false;
  std::vector<std::string> parts;
  size_t i = 1;
  while (true) {
    const size_t j = path.find('/', i);
    parts.push_back(path.substr(i, j == std::string::npos ? std::string::npos : j - i));
    if (j == std::string::npos) break;
    i = j + 1;
  }
  for (const std::string& c : parts)
    if (c.empty() || c == "." || c == "..") return false;
  Node* cur = root;
  for (size_t k = 0; k + 1 < parts.size(); ++k) {
    std::unique_ptr<Node>& n = cur->kids[parts[k]];
    if (!n) n = std::make_unique<Node>();
    if (n->is_file) return false;
    cur = n.get();
  }
  std::unique_ptr<Node>& n = cur->kids[parts.back()];
  if (n) return false;  // given twice, or a directory of that name
  n = std::make_unique<Node>();
  n->is_file = true;
  n->exe = exe;
  n->size = size;
  n->first = first;
  return true;
}

const char kHex[] = "0123456789abcdef";

void plain(const Node& d, const std::string& vpath, uint64_t bs, const uint8_t* digests,
           std::string* out) {
  *out += dirsig::escape(vpath) + "\n";
  ++tot.dir_lines;
  for (const auto& kv : d.kids) {
    const Node& f = *kv.second;
    if (!f.is_file) continue;
    *out += "  " + dirsig::escape(kv.first) + (f.exe ? " x " : " f ") + std::to_string(f.size);
    const uint64_t nb = f.size / bs + (f.size % bs != 0);
    for (uint64_t b = 0; b < nb; ++b) {
      *out += ' ';
      for (int k = 0; k < 32; ++k) {
        const uint8_t v = digests[32 * (f.first + b) + k];
        *out += kHex[v >> 4];
        *out += kHex[v & 15];
      }
    }
    *out += '\n';
  }
  for (const auto& kv : d.kids)
    if (!kv.second->is_file) plain(*kv.second, vpath == "/" ? "/" + kv.first : vpath + "/" + kv.first,
                                   bs, digests, out);
}

template <class T>
std::unique_ptr<T[]> exact(const T* src, size_t n) {  // a heap copy of exactly n elements
  std::unique_ptr<T[]> p(new T[n]);
  if (n) memcpy(p.get(), src, n * sizeof(T));
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  std::mt19937_64 rng(seed);
  auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  static const char* kComp[] = {"a", "b", "a.b", "a.c", "d", "d1", "with space", "\xff\x01",
                                "back\\slash", "Z", "zz", "e", ".x", "..."};
  static const char* kRare[] = {".", "..", "", "nul\0in"};
  for (uint64_t c = 0; c < cases; ++c) {
    const uint64_t bs = 1 + pick(5) * pick(40);
    // small lists around the conflicts, and now and then a few hundred files
    const size_t nfiles = pick(20) == 0 ? 100 + pick(300) : pick(12);
    const uint64_t alphabet = nfiles > 50 ? 14 : 3 + pick(12);
    std::string paths;
    std::vector<uint64_t> path_off{0}, sizes;
    std::vector<uint8_t> exe;
    for (size_t i = 0; i < nfiles; ++i) {
      std::string p;
      const uint64_t depth = 1 + pick(nfiles > 50 ? 5 : 4);
      for (uint64_t k = 0; k < depth; ++k) {
        p += '/';
        if (nfiles <= 50 && pick(150) == 0) {
          const uint64_t r = pick(4);
          p += r == 3 ? std::string(kRare[3], 6) : std::string(kRare[r]);
        } else {
          p += kComp[pick(alphabet)];
          if (nfiles > 50 && k + 1 == depth) p += std::to_string(pick(400));
        }
      }
      if (nfiles <= 50 && pick(200) == 0) p = p.substr(1);  // relative
      if (nfiles <= 50 && pick(200) == 0) p += '/';
      paths += p;
      path_off.push_back(paths.size());
      sizes.push_back(pick(4) == 0 ? 0 : pick(4 * bs + 2));
      exe.push_back((uint8_t)(pick(3) == 0));
    }
    // the independent verdict and tree
    const bool no_exe = pick(8) == 0;  // a null exe array: no file is executable
    Node root;
    bool valid = true;
    uint64_t nblk = 0;
    for (size_t i = 0; i < nfiles; ++i) {
      const std::string p = paths.substr(path_off[i], path_off[i + 1] - path_off[i]);
      if (!insert(&root, p, !no_exe && exe[i] != 0, sizes[i], nblk)) valid = false;
      nblk += sizes[i] / bs + (sizes[i] % bs != 0);
    }
    auto h_paths = exact((const uint8_t*)paths.data(), paths.size());
    auto h_off = exact(path_off.data(), path_off.size());
    auto h_sizes = exact(sizes.data(), sizes.size());
    auto h_exe = exact(exe.data(), exe.size());
    emit::Layout lay;
    std::string err;
    const bool ok = emit::build(emit::Files{h_paths.get(), h_off.get(), h_sizes.get(),
                                            no_exe ? nullptr : h_exe.get(), nfiles},
                                bs, 1ull << 31, &lay, &err);
    if (ok != valid) die(valid ? "a valid list was rejected" : "an invalid list was accepted", c);
    if (!ok) {
      if (err.empty()) die("a rejection without a message", c);
      ++tot.invalid;
      continue;
    }
    if (lay.nblocks != nblk) die("block count", c);
    std::unique_ptr<uint8_t[]> digests(new uint8_t[32 * nblk]);
    for (uint64_t i = 0; i < 32 * nblk; ++i) digests[i] = (uint8_t)rng();
    std::string want;
    plain(root, "/", bs, digests.get(), &want);
    if (lay.body_len != want.size()) die("body length", c);
    // the pieces tile the body
    uint64_t at = 0;
    for (uint64_t k = 0; k < lay.npieces(); ++k) {
      const uint64_t* q = lay.pieces.data() + emit::kPieceWords * k;
      if (q[0] != at || q[1] + q[2] > lay.lits.size() || q[3] + q[4] > nblk) die("piece", c);
      at += q[2] + emit::kTokenBytes * q[4] + 1;
    }
    if (at != lay.body_len) die("pieces do not tile the body", c);
    auto h_pieces = exact(lay.pieces.data(), lay.pieces.size());
    auto h_lits = exact((const uint8_t*)lay.lits.data(), lay.lits.size());
    emit::Tables t{h_pieces.get(), lay.npieces(), h_lits.get(), lay.lits.size(), digests.get(),
                   nblk, lay.body_len};
    const uint64_t cap = emit::round_up16(lay.body_len);
    std::unique_ptr<uint8_t[]> body(new uint8_t[cap]);
    memset(body.get(), 0xEE, cap);
    if (emit::emit_host(t, body.get()) != 0) die("a bad piece in a layout's own tables", c);
    if (memcmp(body.get(), want.data(), want.size()) != 0) die("fill16 differs from the builder", c);
    for (uint64_t o = 0; o < cap + 3; ++o) {
      const uint8_t w = o < want.size() ? (uint8_t)want[o] : 0;
      if (emit::byte_at(t, o) != w) die("byte_at differs from the builder", c);
      if (o < cap && body[o] != w) die("padding", c);
    }
    tot.files += nfiles;
    tot.blocks += nblk;
    tot.body += lay.body_len;

    // damaged tables: ranges outside the arrays, a shorter digest list, a
    // body_len that cuts the last piece
    std::vector<uint64_t> dmg(lay.pieces);
    uint64_t expect_bad = 0;
    const uint64_t ndig = nblk ? nblk - pick(2) : 0;
    auto h_dig = exact(digests.get(), 32 * ndig);
    const uint64_t cut = lay.body_len - pick(lay.body_len < 20 ? lay.body_len : 20);
    for (uint64_t k = 0; k < lay.npieces(); ++k) {
      uint64_t* q = dmg.data() + emit::kPieceWords * k;
      switch (pick(8)) {
        case 0: q[1] = lay.lits.size() - q[2] + 1 + pick(3); break;
        case 1: q[2] = ~0ull - pick(5); break;
        case 2: q[3] = ~0ull - pick(70); break;
        case 3: q[4] = (1ull << 63) + pick(9); break;
        case 4: q[1] = ~0ull; break;
        default: break;
      }
      const bool bad = q[2] > lay.lits.size() || q[1] > lay.lits.size() - q[2] || q[4] > ndig ||
                       q[3] > ndig - q[4];
      if (bad && q[0] < cut) ++expect_bad;
    }
    auto h_dmg = exact(dmg.data(), dmg.size());
    emit::Tables u{h_dmg.get(), lay.npieces(), h_lits.get(), lay.lits.size(), h_dig.get(), ndig,
                   cut};
    const uint64_t ucap = emit::round_up16(cut);
    std::unique_ptr<uint8_t[]> ub(new uint8_t[ucap]);
    memset(ub.get(), 0xEE, ucap);
    if (emit::emit_host(u, ub.get()) != expect_bad) die("bad-piece count", c);
    for (uint64_t o = 0; o < ucap; ++o)
      if (ub[o] != emit::byte_at(u, o)) die("fill16 differs from byte_at on damaged tables", c);
    for (uint64_t k = 0; k < lay.npieces(); ++k) {
      const uint64_t* q = dmg.data() + emit::kPieceWords * k;
      const uint64_t* g = lay.pieces.data() + emit::kPieceWords * k;
      const bool bad = emit::piece_bad(u, q[1], q[2], q[3], q[4]);
      const uint64_t end = k + 1 < lay.npieces() ? g[emit::kPieceWords] : lay.body_len;
      for (uint64_t o = q[0]; o < end && o < cut; ++o)
        if (ub[o] != (bad ? 0 : (uint8_t)want[o])) die("a damaged piece's bytes", c);
    }
    tot.bad_pieces += expect_bad;
  }
  fprintf(stderr,
          "emit_fuzz: %llu files, %llu directory lines, %llu blocks, %llu body bytes; %llu invalid "
          "lists rejected; %llu bad pieces counted\n",
          (unsigned long long)tot.files, (unsigned long long)tot.dir_lines,
          (unsigned long long)tot.blocks, (unsigned long long)tot.body,
          (unsigned long long)tot.invalid, (unsigned long long)tot.bad_pieces);
  printf("emit_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
