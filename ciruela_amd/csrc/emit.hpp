// The rule of the index emitter over a flat file list (cir_index_emit,
// cir_index_emit_dev, cir_index_memory_dev), written once for the host and the
// device: the inverse of idxscan.hpp, from digests to DIRSIGNATURE.v1 text.  No
// HIP runtime call; compiled by emit.hip (the kernels), memindex.cpp (the host
// form and the call) and, with dirsig.cpp alone under the sanitizers, by
// tools/emit_fuzz.cpp.
//
// Input: regular files in the caller's order {raw path bytes, size, exe flag}
// and one flat digest list, file i's digests behind file i-1's in that same
// order: size / bs + (size % bs != 0) digests of 32 bytes per file.
//
// Tree (the checks of cir_index_rewrite's tree, scan.cpp: InvalidPath and
// PathConflict): a path is '/' followed by components separated by single '/';
// no component is empty, "." or ".."; no NUL byte; no path twice; no path that is
// both a file and a directory.  The directories are those the paths imply,
// plus "/".
//
// Order and bytes: what cir_scan_v1 emits for a directory holding these files
// (dirsig::Emitter behind the scan's walk): per directory its line
// (dirsig::escape of the path), its files in bytewise name order ("  " name
// " f " or " x " size, one ' ' + 64 lower-case hex digits per block, '\n'),
// then its subdirectories in bytewise name order, recursively.  A size-0 file
// carries no token.
//
// Layout: the body is a sequence of pieces, one per file in emission order (one
// piece with the literal "/" and no block when there is no file at all).  A
// piece is kPieceWords u64 {out_off, lit_off, lit_len, first_block, nblk}: at
// body offset out_off stand lit_len bytes of the literal arena from lit_off
// (the directory lines since the previous file and the file line's head
// through the size digits), then nblk tokens of the digests first_block ..
// first_block + nblk - 1, then '\n'.  The host knows every size, so every
// out_off is computed there; byte_at() defines each body byte from the tables
// alone, and fill16() is the same function over 16 bytes at once: the host
// emitter and k_emit_text both are fill16().
//
// Untrusted tables: a piece whose literal range lies outside the arena or whose
// block range lies outside the digests is a bad piece: every byte of it is 0 and
// nothing is read through it.  Bytes before the first piece, between pieces
// (where out_off leaves a gap) and at or past body_len are 0 too.  The count of
// bad pieces is exact for tables whose out_off strictly ascends.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CIR_EMIT_HD __host__ __device__
#else
#define CIR_EMIT_HD
#endif

namespace cir {
namespace emit {

constexpr int kPieceWords = 5;        // {out_off, lit_off, lit_len, first_block, nblk}
constexpr uint64_t kTokenBytes = 65;  // ' ' + 64 hex digits
constexpr uint64_t kLaneBytes = 16;   // body bytes per lane of k_emit_text
constexpr uint64_t kMaxPieces = 0xFFFFFFFFull;  // the bisection's 32 steps
constexpr int kFileWords = 3;         // k_mem_desc's table: {first_block, base offset, size}
constexpr uint64_t kNoPiece = ~0ull;

struct Tables {
  const uint64_t* pieces;
  uint64_t npieces;
  const uint8_t* lits;
  uint64_t lits_len;
  const uint8_t* digests;
  uint64_t ndigests;
  uint64_t body_len;
};

CIR_EMIT_HD inline uint64_t round_up16(uint64_t n) { return (n + 15) & ~15ull; }

// The last piece whose out_off is at or below off; kNoPiece when there is none.
// At most 32 steps: npieces <= kMaxPieces.
CIR_EMIT_HD inline uint64_t piece_at(const uint64_t* pieces, uint64_t npieces, uint64_t off) {
  uint64_t lo = 0, hi = npieces;  // pieces[< lo].out_off <= off < pieces[>= hi].out_off
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (pieces[kPieceWords * mid] <= off)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : kNoPiece;
}

// One piece in registers.  bad: a range outside the arrays (or no piece at all:
// the bytes before the first one).
struct Cur {
  uint64_t out_off, lit_off, lit_len, first, nblk;
  uint64_t next_off;  // out_off of the piece behind it, ~0 behind the last one
  bool bad;
};

CIR_EMIT_HD inline bool piece_bad(const Tables& t, uint64_t lit_off, uint64_t lit_len,
                                  uint64_t first, uint64_t nblk) {
  return lit_len > t.lits_len || lit_off > t.lits_len - lit_len || nblk > t.ndigests ||
         first > t.ndigests - nblk;
}

CIR_EMIT_HD inline Cur load_piece(const Tables& t, uint64_t p) {
  Cur c;
  if (p == kNoPiece) {
    c.out_off = c.lit_off = c.lit_len = c.first = c.nblk = 0;
    c.next_off = t.npieces ? t.pieces[0] : ~0ull;
    c.bad = true;
    return c;
  }
  const uint64_t* q = t.pieces + kPieceWords * p;
  c.out_off = q[0];
  c.lit_off = q[1];
  c.lit_len = q[2];
  c.first = q[3];
  c.nblk = q[4];
  c.next_off = p + 1 < t.npieces ? q[kPieceWords] : ~0ull;
  c.bad = piece_bad(t, c.lit_off, c.lit_len, c.first, c.nblk);
  return c;
}

CIR_EMIT_HD inline uint8_t hex_digit(uint32_t v) { return (uint8_t)(v < 10 ? '0' + v : 'a' + v - 10); }

// The body byte at off inside the piece c (c.out_off <= off < c.next_off).
CIR_EMIT_HD inline uint8_t piece_byte(const Tables& t, const Cur& c, uint64_t off) {
  if (c.bad) return 0;
  uint64_t r = off - c.out_off;
  if (r < c.lit_len) return t.lits[c.lit_off + r];
  r -= c.lit_len;
  // (nblk <= ndigests, and the callers keep ndigests below 2^57: no overflow)
  if (r < kTokenBytes * c.nblk) {
    const uint64_t k = r % kTokenBytes;
    if (k == 0) return ' ';
    const uint8_t b = t.digests[32 * (c.first + r / kTokenBytes) + (k - 1) / 2];
    return hex_digit((k - 1) & 1 ? b & 15u : b >> 4);
  }
  return r == kTokenBytes * c.nblk ? '\n' : 0;
}

// The definition: the body byte at off.
CIR_EMIT_HD inline uint8_t byte_at(const Tables& t, uint64_t off) {
  if (off >= t.body_len) return 0;
  const Cur c = load_piece(t, piece_at(t.pieces, t.npieces, off));
  return piece_byte(t, c, off);
}

// The 16 body bytes at off (a multiple of 16) as four little-endian words,
// walking forward from *p = piece_at(off) (a host caller may hand in any piece
// at or before it); leaves *p at the piece of the last byte.  *nbad += the bad
// pieces that start inside [off, off + 16) and before body_len.
CIR_EMIT_HD inline void fill16(const Tables& t, uint64_t off, uint64_t* p, uint32_t w[4],
                               uint32_t* nbad) {
  Cur c = load_piece(t, *p);
  if (*p != kNoPiece && c.bad && c.out_off >= off && c.out_off < t.body_len) ++*nbad;
  w[0] = w[1] = w[2] = w[3] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 16; ++j) {
    const uint64_t o = off + (uint64_t)j;
    if (o >= t.body_len) break;
    if (o >= c.next_off) {  // (a strictly ascending table advances at most once per byte)
      *p = *p == kNoPiece ? 0 : *p + 1;
      c = load_piece(t, *p);
      if (c.bad) ++*nbad;
    }
    w[j >> 2] |= (uint32_t)piece_byte(t, c, o) << (8 * (j & 3));
  }
}

// k_mem_desc's rule: the descriptor of global block g from the table of
// non-empty files {first_block, base offset, size} (first_block ascending).  A
// block the table does not cover gets the empty descriptor.
CIR_EMIT_HD inline void desc_of(const uint64_t* files, uint64_t nfiles, uint64_t bs, uint64_t g,
                                uint64_t* off, uint32_t* len) {
  *off = 0;
  *len = 0;
  uint64_t lo = 0, hi = nfiles;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (files[kFileWords * mid] <= g)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (!lo) return;
  const uint64_t* f = files + kFileWords * (lo - 1);
  const uint64_t j = g - f[0], size = f[2];
  if (j >= size / bs + (size % bs != 0)) return;
  const uint64_t rest = size - j * bs;
  *off = f[1] + j * bs;
  *len = (uint32_t)(rest < bs ? rest : bs);
}

}  // namespace emit
}  // namespace cir

// ---- the host side: tree, order, pieces and literals -----------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dirsig.hpp"

namespace cir {
namespace emit {

struct Files {
  const uint8_t* paths;      // raw bytes, no terminators
  const uint64_t* path_off;  // nfiles + 1 offsets
  const uint64_t* sizes;
  const uint8_t* exe;  // nullable: no file is executable
  uint64_t nfiles;
};

struct Layout {
  std::vector<uint64_t> pieces;       // kPieceWords per piece, emission order
  std::string lits;                   // the literal arena
  std::vector<uint64_t> first_block;  // per file, the caller's order
  uint64_t nblocks = 0, body_len = 0;
  uint64_t npieces() const { return pieces.size() / kPieceWords; }
  Tables tables(const uint8_t* digests) const {
    return Tables{pieces.data(), npieces(), (const uint8_t*)lits.data(), lits.size(), digests,
                  nblocks, body_len};
  }
};

struct PathRef {
  const uint8_t* p;
  size_t n;
};

// The sort key of a valid path: every '/' becomes a 0 byte and a letter, 'F' in
// front of the file name (the last component) and 'S' in front of a directory
// name.  No path holds a 0 byte, so under plain bytewise order of the keys a
// name that ends sorts before every longer one, and where two paths part inside
// one directory the letter puts a file before a subdirectory, whatever their
// names: the emission order.  Equal keys are equal paths.
inline void append_key(const PathRef& r, size_t name0, std::string* keys) {
  for (size_t i = 0; i < r.n; ++i) {
    if (r.p[i] == '/') {
      *keys += '\0';
      *keys += i + 1 == name0 ? 'F' : 'S';
    } else {
      *keys += (char)r.p[i];
    }
  }
}

inline bool path_valid(const PathRef& r, std::string* err) {
  auto bad = [&](const char* what) {
    *err = std::string("Invalid path: ") + what + ": " +
           dirsig::escape(std::string((const char*)r.p, r.n));
    return false;
  };
  if (r.n < 2 || r.p[0] != '/') return bad("not absolute");
  if (memchr(r.p, 0, r.n)) return bad("NUL byte");
  size_t c0 = 1;
  for (size_t i = 1; i <= r.n; ++i) {
    if (i == r.n || r.p[i] == '/') {
      const size_t n = i - c0;
      if (n == 0) return bad("empty component");
      if ((n == 1 && r.p[c0] == '.') || (n == 2 && r.p[c0] == '.' && r.p[c0 + 1] == '.'))
        return bad("\".\" or \"..\" component");
      c0 = i + 1;
    }
  }
  return true;
}

// dirsig::escape of n raw bytes appended to *out; bytes that need no escape
// (the common case) are appended as they are, without a temporary.
inline void append_escaped(std::string* out, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i] <= 0x20 || p[i] >= 0x7f || p[i] == '\\') {
      *out += dirsig::escape(std::string((const char*)p, n));
      return;
    }
  out->append((const char*)p, n);
}

inline uint64_t blocks_of(uint64_t size, uint64_t bs) { return size / bs + (size % bs != 0); }

// Validates the list and lays the body out.  false with *err set: an invalid
// path, a duplicate, a file / directory conflict, more than max_blocks blocks
// or more than kMaxPieces files.  Allocates host memory only.
inline bool build(const Files& f, uint64_t bs, uint64_t max_blocks, Layout* out,
                  std::string* err) {
  const size_t n = (size_t)f.nfiles;
  if (f.nfiles >= kMaxPieces) {
    *err = "more than 2^32-2 files";
    return false;
  }
  std::vector<PathRef> ref(n);
  out->first_block.assign(n, 0);
  uint64_t nblk = 0;
  for (size_t i = 0; i < n; ++i) {
    if (f.path_off[i + 1] < f.path_off[i]) {
      *err = "path_off decreases";
      return false;
    }
    ref[i] = PathRef{f.paths + f.path_off[i], (size_t)(f.path_off[i + 1] - f.path_off[i])};
    if (!path_valid(ref[i], err)) return false;
    out->first_block[i] = nblk;
    const uint64_t nb = blocks_of(f.sizes[i], bs);
    if (nb > max_blocks - nblk) {
      *err = "more blocks than one call takes";
      return false;
    }
    nblk += nb;
  }
  out->nblocks = nblk;
  if (n == 0) {  // (path_off may be null then) the body is "/\n"
    out->lits = "/";
    const uint64_t one[kPieceWords] = {0, 0, 1, 0, 0};
    out->pieces.assign(one, one + kPieceWords);
    out->body_len = 2;
    return true;
  }
  // the emission order: one sort of the keys
  std::string keys;
  std::vector<size_t> key_off(n + 1, 0), name_at(n);
  keys.reserve((size_t)(f.path_off[n] - f.path_off[0]) + 2 * n);
  for (size_t i = 0; i < n; ++i) {
    size_t name0 = ref[i].n;
    while (ref[i].p[name0 - 1] != '/') --name0;  // the file name is [name0, n)
    name_at[i] = name0;
    append_key(ref[i], name0, &keys);
    key_off[i + 1] = keys.size();
  }
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const size_t la = key_off[a + 1] - key_off[a], lb = key_off[b + 1] - key_off[b];
    const int c = memcmp(keys.data() + key_off[a], keys.data() + key_off[b], la < lb ? la : lb);
    return c < 0 || (c == 0 && la < lb);
  });

  auto path_str = [](const PathRef& r) { return dirsig::escape(std::string((const char*)r.p, r.n)); };
  out->pieces.clear();
  out->pieces.reserve((n ? n : 1) * kPieceWords);
  out->lits.clear();
  uint64_t body = 0;
  out->lits = "/\n";
  // The directories on the way to the current file: level d's path is the
  // current path's first `end` bytes (level 0 is "/", end 0), and [lo, hi) are
  // the positions in `order` of the files directly in it.  A directory's own
  // files all come before its first subdirectory, so when a subdirectory is
  // entered its parent's range is final: a file of the subdirectory's name in it
  // is the conflict.
  struct Level {
    size_t end;
    size_t lo, hi;
  };
  std::vector<Level> lv{Level{0, 0, 0}};
  PathRef prev{nullptr, 0};
  for (size_t k = 0; k < n; ++k) {
    const PathRef& r = ref[order[k]];
    const size_t name0 = name_at[order[k]];
    if (k && prev.n == r.n && memcmp(prev.p, r.p, r.n) == 0) {
      *err = "Path given twice: " + path_str(r);
      return false;
    }
    const size_t lit0 = out->lits.size();
    // the directory levels shared with the previous file: equal text, level by level
    size_t keep = 1;
    while (keep < lv.size() && lv[keep].end < name0 && r.p[lv[keep].end] == '/' &&
           memcmp(prev.p + lv[keep - 1].end, r.p + lv[keep - 1].end,
                  lv[keep].end - lv[keep - 1].end) == 0)
      ++keep;
    lv.resize(keep);
    // enter the levels below: one directory line each
    while (lv.back().end + 1 < name0) {
      const size_t c0 = lv.back().end + 1;
      size_t ce = c0;
      while (r.p[ce] != '/') ++ce;
      // a file of this name directly in the parent?
      size_t lo = lv.back().lo, hi = lv.back().hi;
      const size_t cn = ce - c0;
      while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        const PathRef& q = ref[order[mid]];
        const size_t qn = q.n - c0;
        const int c = memcmp(q.p + c0, r.p + c0, qn < cn ? qn : cn);
        if (c == 0 && qn == cn) {
          *err = "The following path conflicts with others: " + path_str(q);
          return false;
        }
        if (c < 0 || (c == 0 && qn < cn))
          lo = mid + 1;
        else
          hi = mid;
      }
      lv.push_back(Level{ce, k, k});
      append_escaped(&out->lits, r.p, ce);
      out->lits += '\n';
    }
    lv.back().hi = k + 1;
    out->lits += "  ";
    append_escaped(&out->lits, r.p + name0, r.n - name0);
    out->lits += f.exe && f.exe[order[k]] ? " x " : " f ";
    out->lits += std::to_string(f.sizes[order[k]]);
    const uint64_t l0 = k == 0 ? 0 : lit0;
    const uint64_t lit_len = out->lits.size() - l0;
    const uint64_t nb = blocks_of(f.sizes[order[k]], bs);
    const uint64_t piece[kPieceWords] = {body, l0, lit_len, out->first_block[order[k]], nb};
    out->pieces.insert(out->pieces.end(), piece, piece + kPieceWords);
    body += lit_len + kTokenBytes * nb + 1;
    prev = r;
  }
  out->body_len = body;
  return true;
}

// The body from the tables, 16 bytes at a time: dst holds round_up16(body_len)
// bytes.  Returns the number of bad pieces (0 for a Layout's own tables).
inline uint64_t emit_host(const Tables& t, uint8_t* dst) {
  uint64_t p = piece_at(t.pieces, t.npieces, 0), bad = 0;
  for (uint64_t off = 0; off < t.body_len; off += kLaneBytes) {
    uint32_t w[4], nb = 0;
    fill16(t, off, &p, w, &nb);
    bad += nb;
    memcpy(dst + off, w, 16);
  }
  return bad;
}

}  // namespace emit
}  // namespace cir
#endif
