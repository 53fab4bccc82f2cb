// Seeded fuzz of ciruela_amd/csrc/idxscan.hpp (the rule which index lines the
// device parser of cir_index_digests_dev takes) against dirsig::parse.
// Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/index_accept_fuzz.cpp ciruela_amd/csrc/dirsig.cpp \
//       -o build/index_accept_fuzz
// and run it; tests/test_index_digests_cpu.py does.
//
// The invariant: the header's host loop (scan_host: parse_head on every body
// line, decode_token on every token) reports no declined line  =>
// dirsig::parse succeeds on the same bytes and gives the same file count, the
// same (first block, size, file ordinal) per non-empty file and the same
// digests; and dirsig::frame fails only where dirsig::parse fails.  Checked
// over seeded random indexes (dirsig::Emitter's; every one of those must be
// taken, not declined) and over one mutation of each: a flipped byte, a
// deleted or doubled space, a swapped case, a truncated line, an injected
// \x2e, \x2f or \x00, a raw tab or "\r", a size that disagrees with the token
// count, sizes near 2^64.  Every text and every output array lives in a heap
// buffer of exactly its size, so a read or write one byte outside is an
// AddressSanitizer report.
//
// usage: index_accept_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dirsig.hpp"
#include "idxscan.hpp"

using namespace cir;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

static std::string random_name() {
  static const char* kOdd[] = {"a b", "\xff" "q", "back\\slash", "...", ".x", "x.", "tab\there",
                               "nl\nname", "UPPER", "~"};
  if (rnd() % 5 == 0) return kOdd[rnd() % 10];
  std::string s;
  const int n = 1 + (int)(rnd() % 9);
  for (int i = 0; i < n; ++i) s += (char)('a' + rnd() % 26);
  if (rnd() % 40 == 0) s = std::string(1400, 'n') + s;  // (escaped below: a long head)
  return s;
}

static std::string random_index(uint64_t* bs_out) {
  static const uint64_t kBs[] = {1, 2, 64, 4096, 32768};
  dirsig::Header h;
  h.block_size = kBs[rnd() % 5];
  h.hash = rnd() % 2 ? dirsig::HashType::kBlake2b256 : dirsig::HashType::kSha512_256;
  *bs_out = h.block_size;
  dirsig::Emitter em(h);
  const int ndirs = (int)(rnd() % 4);
  for (int d = 0; d < ndirs; ++d) {
    em.start_dir(d == 0 ? "/" : "/d" + std::to_string(d) + "/" + random_name());
    const int nfiles = (int)(rnd() % 6);
    for (int f = 0; f < nfiles; ++f) {
      std::string name = random_name() + std::to_string(f);
      if (name.size() > 1000) {  // four bytes per byte once escaped: past kMaxHead
        for (char& c : name) c = c == 'n' ? '\x01' : c;
      }
      if (rnd() % 6 == 0) {
        em.add_symlink(name, rnd() % 2 ? "../t g" : "/abs/target");
        continue;
      }
      static const uint64_t kFull[] = {0, 0, 1, 2, 3, 9};
      const uint64_t nfull = kFull[rnd() % 6];
      const uint64_t tail = h.block_size > 1 && rnd() % 3 == 0 ? 1 + rnd() % (h.block_size - 1) : 0;
      const uint64_t nb = nfull + (tail != 0);
      std::vector<uint8_t> hs(32 * nb + 1);
      for (uint8_t& b : hs) b = (uint8_t)rnd();
      em.add_file(name, rnd() % 4 == 0, nfull * h.block_size + tail, hs.data(), nb);
    }
  }
  static const uint8_t footer[32] = {1};
  size_t len = 0;
  uint8_t* raw = em.finish_malloc(footer, 32, &len);
  if (!raw) abort();
  std::string s((const char*)raw, len);
  free(raw);
  return s;
}

// The digit spans of the size fields: behind " f " or " x " on an entry line.
static std::vector<std::pair<size_t, size_t>> size_fields(const std::string& s) {
  std::vector<std::pair<size_t, size_t>> out;
  for (size_t i = 0; i + 3 < s.size(); ++i)
    if (s[i] == ' ' && (s[i + 1] == 'f' || s[i + 1] == 'x') && s[i + 2] == ' ' &&
        s[i + 3] >= '0' && s[i + 3] <= '9') {
      size_t j = i + 3;
      while (j < s.size() && s[j] >= '0' && s[j] <= '9') ++j;
      out.push_back({i + 3, j - (i + 3)});
    }
  return out;
}

static std::string mutate(const std::string& in, uint64_t bs) {
  std::string s = in;
  const size_t at = rnd() % s.size();
  switch (rnd() % 10) {
    case 0:  // a flipped byte
      s[at] = (char)(s[at] ^ (1 + rnd() % 255));
      break;
    case 1: {  // a deleted space
      const size_t p = s.find(' ', at);
      if (p != std::string::npos) s.erase(p, 1);
      break;
    }
    case 2: {  // a doubled space
      const size_t p = s.find(' ', at);
      if (p != std::string::npos) s.insert(p, 1, ' ');
      break;
    }
    case 3: {  // a swapped case
      size_t p = at;
      while (p < s.size() && !((s[p] | 0x20) >= 'a' && (s[p] | 0x20) <= 'z')) ++p;
      if (p < s.size()) s[p] = (char)(s[p] ^ 0x20);
      break;
    }
    case 4: {  // a truncated line
      const size_t e = s.find('\n', at);
      if (e != std::string::npos) s.erase(at, rnd() % 2 ? e - at : (e - at) / 2);
      break;
    }
    case 5: {  // an injected escape
      static const char* kEsc[] = {"\\x2e", "\\x2f", "\\x00", "\\x2E", "\\x2", "\\y41", "\\x41"};
      s.insert(at, kEsc[rnd() % 7]);
      break;
    }
    case 6: {  // a raw byte the canonical form escapes
      static const char kRaw[] = {'\t', '\r', '\x7f', '\x00', '\x80', '\n'};
      s.insert(at, 1, kRaw[rnd() % 6]);
      break;
    }
    case 7: {  // a size that disagrees with the token count
      const auto f = size_fields(s);
      if (f.empty()) break;
      const auto sp = f[rnd() % f.size()];
      const uint64_t v = strtoull(s.substr(sp.first, sp.second).c_str(), nullptr, 10);
      static const int64_t kD[] = {1, -1, 0, 0};
      uint64_t nv = v + (uint64_t)kD[rnd() % 2] * (rnd() % 2 ? bs : 1);
      if (rnd() % 4 == 0) nv = 0;
      s.replace(sp.first, sp.second, std::to_string(nv));
      break;
    }
    case 8: {  // sizes near 2^64, too many digits, leading zeros
      const auto f = size_fields(s);
      if (f.empty()) break;
      const auto sp = f[rnd() % f.size()];
      static const char* kBig[] = {"18446744073709551615", "18446744073709551616",
                                   "18446744073709551614", "99999999999999999999",
                                   "184467440737095516150", "000000000000000000064",
                                   "00000000000000000064", "9223372036854775808"};
      s.replace(sp.first, sp.second, kBig[rnd() % 8]);
      break;
    }
    default: {  // a token cut short or grown by a digit; a "\r\n"
      const size_t e = s.find('\n', at);
      if (e == std::string::npos) break;
      if (rnd() % 3 == 0)
        s.insert(e, 1, '\r');
      else if (rnd() % 2)
        s.erase(e - 1, 1);
      else
        s.insert(e, 1, 'a');
      break;
    }
  }
  return s;
}

static int failures = 0;
static void fail_case(const char* what, const std::string& text) {
  fprintf(stderr, "index_accept_fuzz: %s\n---\n%.*s\n---\n", what, (int)text.size(), text.c_str());
  ++failures;
}

// One text through both parsers; returns true when the device rule took it.
static bool check(const std::string& text) {
  uint8_t* t = (uint8_t*)malloc(text.size() ? text.size() : 1);  // exactly its size
  memcpy(t, text.data(), text.size());
  dirsig::Index idx;
  std::string err, ferr;
  const bool host_ok = dirsig::parse(t, text.size(), &idx, &err);
  dirsig::Header h;
  size_t b0 = 0, b1 = 0;
  const bool framed = dirsig::frame(t, text.size(), &h, &b0, &b1, &ferr);
  bool taken = false;
  if (!framed) {
    if (host_ok) fail_case("frame fails where parse succeeds", text);
  } else {
    if (!(b0 <= b1 && b1 < text.size() && (b0 == b1 || t[b1 - 1] == '\n')))
      fail_case("frame gives a body that is not empty or '\\n'-terminated", text);
    if (host_ok && (h.hash != idx.header.hash || h.block_size != idx.header.block_size))
      fail_case("frame's header differs from parse's", text);
    const idxscan::Counts c = idxscan::scan_host(t, b0, b1, h.block_size, nullptr, nullptr);
    if (c.declined == idxscan::kBad) {
      taken = true;
      uint8_t* dg = (uint8_t*)malloc(c.blocks ? 32 * c.blocks : 1);
      idxscan::Run* runs = (idxscan::Run*)malloc(c.runs ? sizeof(idxscan::Run) * c.runs : 1);
      const idxscan::Counts c2 = idxscan::scan_host(t, b0, b1, h.block_size, dg, runs);
      if (c2.declined != idxscan::kBad || c2.blocks != c.blocks || c2.runs != c.runs ||
          c2.files != c.files)
        fail_case("the two passes of the host loop disagree", text);
      if (!host_ok) {
        fail_case(("taken by the device rule, rejected by parse: " + err).c_str(), text);
      } else {
        uint64_t file = 0, blk = 0, run = 0;
        bool same = true;
        for (const dirsig::Entry& e : idx.entries) {
          if (e.kind != dirsig::EntryKind::kFile) continue;
          const uint64_t nb = e.hashes.size() / 32;
          if (nb) {
            if (run >= c.runs || blk + nb > c.blocks) {
              same = false;
              break;
            }
            const idxscan::Run& r = runs[run];
            same = same && r.first == blk && r.size == e.size && r.file == file &&
                   t[r.hash_off] == ' ' && memcmp(dg + 32 * blk, e.hashes.data(), 32 * nb) == 0;
            ++run;
            blk += nb;
          }
          ++file;
        }
        if (!same || file != c.files || run != c.runs || blk != c.blocks)
          fail_case("taken by the device rule with other counts, runs or digests", text);
      }
      free(dg);
      free(runs);
    } else if (c.declined < b0 || c.declined >= b1 ||
               !(c.declined == b0 || t[c.declined - 1] == '\n')) {
      fail_case("the declined offset is not a line start of the body", text);
    }
  }
  free(t);
  return taken;
}

int main(int argc, char** argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 4000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  long n = 0, taken_mut = 0;
  while (n < cases && !failures) {
    uint64_t bs = 0;
    const std::string base = random_index(&bs);
    // every emitted index is canonical unless a head passes kMaxHead
    const bool long_head = base.find("\\x01\\x01\\x01") != std::string::npos;
    if (!check(base) && !long_head) fail_case("an emitted index was declined", base);
    ++n;
    const std::string mut = mutate(base, bs);
    taken_mut += check(mut);
    ++n;
  }
  if (failures) return 1;
  // some mutations stay canonical (upper-case hex, a changed name byte), most do not
  if (n >= 200 && (taken_mut == 0 || taken_mut * 4 > n)) {
    fprintf(stderr, "index_accept_fuzz: %ld of %ld mutations taken: the mutator lost its teeth\n",
            taken_mut, n / 2);
    return 1;
  }
  printf("index_accept_fuzz: %ld cases ok\n", n);
  return 0;
}
