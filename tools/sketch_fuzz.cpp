// Seeded fuzz of the sketch rule (ciruela_amd/csrc/sketch.hpp: key, bottom_k,
// index_keys, encode, view, overlap, rank -- the text the host path of
// cir_index_sketch and cir_sketch_rank compile) against restatements that go
// one key and one source at a time.  Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iciruela_amd/csrc tools/sketch_fuzz.cpp ciruela_amd/csrc/dirsig.cpp \
//       -o build/sketch_fuzz
// and run it; tests/test_index_sketch_cpu.py does.  Every blob sits in a heap
// buffer of exactly its size, so a read one byte outside is an
// AddressSanitizer report.
//
// Per case: an index of 0-12 files of 0-40 blocks over a small universe of
// digests (so that digests repeat, inside an image and between images), emitted
// and parsed by dirsig.cpp; a need sketch and 0-6 source sketches of random
// sizes k.
//   1. key equals a restatement byte by byte; a digest solved for a chosen key
//      (0, 2^64 - 1, random) has that key;
//   2. bottom_k over index_keys equals the first k of a std::set of the keys;
//   3. encode then view gives the fields back; view rejects a short header, a
//      foreign magic, k = 0, k > 4096, count > k, count > n_blocks, a length one
//      byte off either way, equal neighbours and descending keys;
//   4. overlap equals a loop over the need's keys with a std::set of the
//      source's;
//   5. rank equals a loop per source and an insertion by exact fractions, with
//      null, malformed and foreign (hash type, block size) sources left out and
//      counted, and ties in the caller's order.
//
// usage: sketch_fuzz [cases [seed]]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "dirsig.hpp"
#include "sketch.hpp"

using namespace cir;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

static uint64_t g_case, g_blocks, g_full, g_partial, g_ranked, g_skipped, g_rejected, g_ties;
#define CHECK(c)                                                                    \
  do {                                                                              \
    if (!(c)) {                                                                     \
      fprintf(stderr, "sketch_fuzz: %s:%d: %s (case %llu)\n", __FILE__, __LINE__, #c, \
              (unsigned long long)g_case);                                          \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

// A heap buffer of exactly n bytes (none at all for n == 0).
struct Exact {
  uint8_t* p;
  size_t n;
  explicit Exact(size_t n_) : p(n_ ? new uint8_t[n_]() : nullptr), n(n_) {}
  Exact(const uint8_t* src, size_t n_) : Exact(n_) {
    if (n_) memcpy(p, src, n_);
  }
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

struct Digest {
  uint8_t b[32];
};

// the key, one byte at a time
static uint64_t key_restated(const uint8_t* d) {
  unsigned __int128 x = 0x243F6A8885A308D3ull;
  for (int w = 0; w < 4; ++w) {
    uint64_t word = 0;
    for (int i = 0; i < 8; ++i) word |= (uint64_t)d[8 * w + i] << (8 * i);
    uint64_t y = ((uint64_t)x ^ word);
    x = ((unsigned __int128)y * 0x9E3779B97F4A7C15ull) & ~(uint64_t)0;
    x = (uint64_t)x ^ ((uint64_t)x >> 32);
  }
  return (uint64_t)x;
}

static uint64_t inverse_of_mul() {  // Newton: five steps double the correct bits from 3
  uint64_t inv = sketch::kMul;      // (odd: correct to 3 bits)
  for (int i = 0; i < 5; ++i) inv *= 2 - sketch::kMul * inv;
  return inv;
}

static Digest digest_with_key(uint64_t want) {
  Digest d;
  uint64_t x = sketch::kSeed;
  for (int w = 0; w < 3; ++w) {
    const uint64_t word = rnd();
    sketch::store_le64(d.b + 8 * w, word);
    x = sketch::mix(x, word);
  }
  const uint64_t y = want ^ (want >> 32);
  sketch::store_le64(d.b + 24, (y * inverse_of_mul()) ^ x);
  return d;
}

struct Image {
  uint32_t hash = 1;
  uint64_t bs = 64;
  std::vector<Digest> blocks;
};

// The index text of an image, through the emitter, in a buffer of its size.
static std::vector<uint8_t> emit(const Image& im) {
  dirsig::Header h;
  h.hash = im.hash == 1 ? dirsig::HashType::kBlake2b256 : dirsig::HashType::kSha512_256;
  h.block_size = im.bs;
  dirsig::Emitter e(h);
  e.start_dir("/");
  e.add_symlink("l", "t");
  size_t at = 0;
  int fi = 0;
  while (at < im.blocks.size() || fi == 0) {
    const size_t n = std::min<size_t>(rnd() % 41, im.blocks.size() - at);
    const uint64_t size = n ? (n - 1) * im.bs + 1 + rnd() % im.bs : 0;
    if (fi == 3) e.start_dir("/sub dir");
    e.add_file("f" + std::to_string(fi), fi % 3 == 0, size,
               n ? im.blocks[at].b : nullptr, n);
    at += n;
    ++fi;
  }
  const uint8_t footer[32] = {1, 2, 3};  // (the parser does not recompute it)
  size_t len = 0;
  uint8_t* buf = e.finish_malloc(footer, 32, &len);
  CHECK(buf);
  std::vector<uint8_t> out(buf, buf + len);
  free(buf);
  return out;
}

static std::vector<uint64_t> set_sketch(const std::vector<Digest>& blocks, uint32_t k) {
  std::set<uint64_t> s;
  for (const Digest& d : blocks) s.insert(key_restated(d.b));
  std::vector<uint64_t> out;
  for (uint64_t x : s) {
    if (out.size() == k) break;
    out.push_back(x);
  }
  return out;
}

// The sketch of an image through the rule's own path: text, parse, keys, bottom-k, blob.
static Exact* sketch_of(const Image& im, uint32_t k) {
  const std::vector<uint8_t> text = emit(im);
  const Exact exact_text(text.data(), text.size());
  dirsig::Index idx;
  std::string err;
  CHECK(dirsig::parse(exact_text.p, exact_text.n, &idx, &err));
  std::vector<uint64_t> all = sketch::index_keys(idx);
  CHECK(all.size() == im.blocks.size());
  for (size_t i = 0; i < all.size(); ++i) CHECK(all[i] == key_restated(im.blocks[i].b));
  const std::vector<uint64_t> keys = sketch::bottom_k(&all, k);
  CHECK(keys == set_sketch(im.blocks, k));
  Exact* blob = new Exact(sketch::blob_bytes(keys.size()));
  sketch::encode(im.hash, k, im.bs, im.blocks.size(), keys.data(), keys.size(), blob->p);
  sketch::View v;
  CHECK(sketch::view(blob->p, blob->n, &v));
  CHECK(v.hash_type == im.hash && v.k == k && v.block_size == im.bs &&
        v.n_blocks == im.blocks.size() && v.count == keys.size());
  for (size_t i = 0; i < keys.size(); ++i) CHECK(v.at(i) == keys[i]);
  g_blocks += im.blocks.size();
  (keys.size() == k ? g_full : g_partial)++;
  return blob;
}

static void expect_rejected(const uint8_t* p, size_t n) {
  const Exact e(p, n);
  sketch::View v;
  CHECK(!sketch::view(e.p, e.n, &v));
  ++g_rejected;
}

// Malformed variants of a valid blob.
static void malformed(const Exact& blob) {
  std::vector<uint8_t> b(blob.p, blob.p + blob.n);
  const uint64_t count = sketch::load_le64(b.data() + 32);
  const uint32_t k = sketch::load_le32(b.data() + 12);
  expect_rejected(b.data(), rnd() % sketch::kHeaderBytes);  // a short header
  expect_rejected(b.data(), b.size() - 1);                  // a length off by one
  {
    std::vector<uint8_t> c = b;
    c.push_back(0);
    expect_rejected(c.data(), c.size());
    if (count) {  // a whole key too many for the count
      c.resize(b.size() + 8, 0xFF);
      expect_rejected(c.data(), c.size());
    }
  }
  {
    std::vector<uint8_t> c = b;
    c[rnd() % 8] ^= 1 << (rnd() % 8);  // a foreign magic
    expect_rejected(c.data(), c.size());
  }
  for (uint32_t bad_k : {0u, 4097u, 0xFFFFFFFFu}) {
    std::vector<uint8_t> c = b;
    sketch::store_le32(c.data() + 12, bad_k);
    expect_rejected(c.data(), c.size());
  }
  if (count) {
    std::vector<uint8_t> c = b;  // count > k
    sketch::store_le32(c.data() + 12, (uint32_t)count - 1);
    expect_rejected(c.data(), c.size());
    c = b;  // count > n_blocks
    sketch::store_le64(c.data() + 24, count - 1);
    expect_rejected(c.data(), c.size());
    c = b;  // the count says more keys than the blob holds
    sketch::store_le64(c.data() + 32, count + 1);
    sketch::store_le32(c.data() + 12, std::max<uint32_t>(k, (uint32_t)count + 1));
    sketch::store_le64(c.data() + 24, ~0ull);
    expect_rejected(c.data(), c.size());
    c = b;  // a count whose 8 x count wraps
    sketch::store_le64(c.data() + 32, (1ull << 61) + count);
    expect_rejected(c.data(), c.size());
  }
  if (count >= 2) {
    const size_t i = 1 + rnd() % (count - 1);
    std::vector<uint8_t> c = b;  // equal neighbours
    memcpy(c.data() + 40 + 8 * i, c.data() + 40 + 8 * (i - 1), 8);
    expect_rejected(c.data(), c.size());
    c = b;  // descending keys
    uint8_t t[8];
    memcpy(t, c.data() + 40 + 8 * i, 8);
    memcpy(c.data() + 40 + 8 * i, c.data() + 40 + 8 * (i - 1), 8);
    memcpy(c.data() + 40 + 8 * (i - 1), t, 8);
    expect_rejected(c.data(), c.size());
  }
}

struct Row {
  uint64_t ordinal, shared, examined;
};

static void overlap_restated(const std::vector<uint64_t>& need, uint32_t nk,
                             const std::vector<uint64_t>& src, uint32_t sk, uint64_t* shared,
                             uint64_t* examined) {
  const uint64_t tn = need.size() == nk ? need.back() : ~0ull;
  const uint64_t ts = src.size() == sk ? src.back() : ~0ull;
  const uint64_t tau = tn < ts ? tn : ts;
  const std::set<uint64_t> held(src.begin(), src.end());
  *shared = *examined = 0;
  for (uint64_t x : need) {
    if (x > tau) continue;
    ++*examined;
    if (held.count(x)) ++*shared;
  }
}

// a's fraction against b's, in 128 bits: > 0 when a's is larger
static int cmp_fraction(const Row& a, const Row& b) {
  // (0 / 0 counts as 0 / 1)
  const unsigned __int128 l = (unsigned __int128)a.shared * (b.examined ? b.examined : 1);
  const unsigned __int128 r = (unsigned __int128)b.shared * (a.examined ? a.examined : 1);
  return l > r ? 1 : l < r ? -1 : 0;
}

static void one_case() {
  // a small universe of digests, a few with crafted keys
  std::vector<Digest> universe;
  const size_t nu = 1 + rnd() % 200;
  for (size_t i = 0; i < nu; ++i) {
    const uint64_t r = rnd() % 50;
    const uint64_t want = r == 0 ? 0 : r == 1 ? ~0ull : r == 2 ? 1 : r == 3 ? ~0ull - 1 : rnd();
    universe.push_back(digest_with_key(want));
    CHECK(sketch::key(universe.back().b) == want && key_restated(universe.back().b) == want);
  }
  auto image = [&](uint32_t hash, uint64_t bs) {
    Image im;
    im.hash = hash;
    im.bs = bs;
    const size_t n = rnd() % 4 == 0 ? 0 : rnd() % 300;
    const size_t span = 1 + rnd() % nu;  // (a narrow span repeats digests often)
    for (size_t i = 0; i < n; ++i) im.blocks.push_back(universe[rnd() % span]);
    return im;
  };
  auto pick_k = [&]() -> uint32_t {
    const uint64_t r = rnd() % 6;
    return r == 0 ? 1 : r == 1 ? 4096 : r == 2 ? 1 + rnd() % 8 : 1 + rnd() % 200;
  };
  const uint64_t bs = 1 + rnd() % 100;
  const Image need_im = image(1 + rnd() % 2, bs);
  const uint32_t nk = pick_k();
  Exact* need = sketch_of(need_im, nk);
  malformed(*need);
  const std::vector<uint64_t> need_keys = set_sketch(need_im.blocks, nk);

  const size_t nsrc = rnd() % 7;
  std::vector<Exact*> blobs(nsrc, nullptr);
  std::vector<const uint8_t*> sp(nsrc, nullptr);
  std::vector<size_t> sl(nsrc, 0);
  std::vector<Row> want;
  size_t want_skipped = 0;
  for (size_t s = 0; s < nsrc; ++s) {
    const uint64_t kind = rnd() % 10;
    if (kind == 0) {  // null
      ++want_skipped;
      continue;
    }
    Image im = image(need_im.hash, bs);
    if (kind == 1) im.hash = 3 - need_im.hash;
    if (kind == 2) im.bs = bs + 1;
    if (kind == 3) im.blocks = need_im.blocks;  // (ties with another copy: the caller's order)
    const uint32_t k = pick_k();
    blobs[s] = sketch_of(im, k);
    if (kind == 4 && blobs[s]->n > 40) {  // malformed: the last key dropped, the count kept
      Exact* cut = new Exact(blobs[s]->p, blobs[s]->n - 8);
      delete blobs[s];
      blobs[s] = cut;
    }
    sp[s] = blobs[s]->p;
    sl[s] = blobs[s]->n;
    if (kind == 1 || kind == 2 || (kind == 4 && !im.blocks.empty())) {
      ++want_skipped;
      continue;
    }
    Row r{s, 0, 0};
    overlap_restated(need_keys, nk, set_sketch(im.blocks, k), k, &r.shared, &r.examined);
    // insertion: behind every row that is not worse
    size_t at = want.size();
    while (at > 0 && cmp_fraction(r, want[at - 1]) > 0) --at;
    want.insert(want.begin() + at, r);
  }
  sketch::View nv;
  CHECK(sketch::view(need->p, need->n, &nv));
  size_t skipped = 99;
  const std::vector<sketch::Ranked> got =
      sketch::rank(nv, nsrc ? sp.data() : nullptr, nsrc ? sl.data() : nullptr, nsrc, &skipped);
  CHECK(skipped == want_skipped && got.size() == want.size());
  for (size_t i = 0; i < got.size(); ++i) {
    CHECK(got[i].ordinal == want[i].ordinal && got[i].shared == want[i].shared &&
          got[i].examined == want[i].examined);
    CHECK(got[i].shared <= got[i].examined && got[i].examined <= nv.count);
    if (i && cmp_fraction(want[i - 1], want[i]) == 0) ++g_ties;
  }
  g_ranked += got.size();
  g_skipped += skipped;
  for (Exact* b : blobs) delete b;
  delete need;
}

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  CHECK(sketch::kMul * inverse_of_mul() == 1);
  for (g_case = 0; g_case < cases; ++g_case) one_case();
  fprintf(stderr,
          "sketch_fuzz: %llu blocks; %llu full and %llu partial sketches; %llu ranked, %llu left "
          "out, %llu ties; %llu malformed blobs rejected\n",
          (unsigned long long)g_blocks, (unsigned long long)g_full, (unsigned long long)g_partial,
          (unsigned long long)g_ranked, (unsigned long long)g_skipped, (unsigned long long)g_ties,
          (unsigned long long)g_rejected);
  printf("sketch_fuzz: %llu cases ok\n", (unsigned long long)cases);
  return 0;
}
