// The acceptance rule of the device index parser (cir_index_digests_dev),
// written once for the host and the device.  No HIP runtime call; compiled by
// idxscan.hip (the kernels), idxscan.cpp (the host form) and, with dirsig.cpp
// alone under the sanitizers, by tools/index_accept_fuzz.cpp.
//
// The device path accepts a canonical subset of what dirsig::parse accepts and
// declines the rest; it never guesses.  The invariant everything rests on:
//
//   status OK  =>  dirsig::parse succeeds on the same bytes, and the file
//   count, the non-empty files' (first block, size, file ordinal) and every
//   digest are identical.
//
// A declined index goes to the host parser, which alone decides between
// success, CIR_EPARSE and CIR_EHASHSIZE and produces the error text.
//
// The subset, over the body [body_off, body_end) (after the header line, before
// the footer line; empty, or ending in '\n'):
//   * the first line starts with '/' (the parser's have_dir);
//   * a directory line starts with '/'; every byte up to its '\n' is in
//     0x21..0x7e; a backslash is followed by 'x' and two hex digits and the
//     decoded byte is not 0x00, 0x2e or 0x2f (so no escape can form a ".",
//     ".." or "/" component); no literal component is "." or ".."; at most
//     kMaxHead bytes;
//   * an entry line is "  " name ' ' type ' ' ...: the name non-empty, bytes
//     and escapes as in a directory line, no literal '/', not literally "." or
//     ".."; type one of f x s;
//   * f / x: 1-20 decimal digits without u64 overflow (parse_u64), n = size /
//     bs + (size % bs != 0) tokens of exactly ' ' + 64 hex digits (upper case
//     decodes as on the host), then '\n' -- '\n' right after the digits when
//     n == 0;
//   * s: one non-empty token of bytes 0x21..0x7e with valid escapes (any
//     decoded value), then '\n';
//   * the head of an entry line (through the size digits, or through the
//     symlink target) is at most kMaxHead bytes; a longer one is declined;
//   * anything else is declined: two spaces in a row, a trailing space, a raw
//     byte outside 0x21..0x7e, an unknown type, a wrong token count, a bad hex
//     digit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CIR_HD __host__ __device__
#else
#define CIR_HD
#endif

namespace cir {
namespace idxscan {

constexpr uint64_t kMaxHead = 4096;   // longest directory line / entry head, without its '\n'
constexpr uint64_t kTokenBytes = 65;  // ' ' + 64 hex digits
constexpr uint64_t kMinRunLine = 73;  // "  a f 1" + one token + '\n': the shortest line with a block
constexpr uint64_t kBad = ~0ull;

enum Kind : uint32_t { kDecline = 0, kDir = 1, kLink = 2, kFile = 3 };

struct Head {
  uint32_t kind;      // Kind
  uint64_t size;      // kFile: the entry's size
  uint64_t nblk;      // kFile: its number of tokens
  uint64_t hash_off;  // kFile: offset of the byte behind the size digits (the first token's ' ')
};

CIR_HD inline int hexval(uint8_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

// The token that starts at i: the offset of the ' ' or '\n' that ends it, which
// lies before lim; kBad when a byte is outside 0x21..0x7e, an escape is
// malformed, (path_rules) an escape decodes to 0x00, '.' or '/', (no_slash)
// a literal '/' occurs, or no terminator comes before lim.
CIR_HD inline uint64_t token_end(const uint8_t* t, uint64_t i, uint64_t lim, bool path_rules,
                                 bool no_slash) {
  while (i < lim) {
    const uint8_t c = t[i];
    if (c == ' ' || c == '\n') return i;
    if (c < 0x21 || c > 0x7e) return kBad;
    if (c == '\\') {
      if (lim - i < 4 || t[i + 1] != 'x') return kBad;
      const int a = hexval(t[i + 2]), b = hexval(t[i + 3]);
      if (a < 0 || b < 0) return kBad;
      const int v = a * 16 + b;
      if (path_rules && (v == 0x00 || v == 0x2e || v == 0x2f)) return kBad;
      i += 4;
      continue;
    }
    if (no_slash && c == '/') return kBad;
    ++i;
  }
  return kBad;
}

// Classify the body line that starts at p (p < end; end = body_end) and parse
// its head.  Reads only [p, end).  A kFile head promises: hash_off + 65 nblk <
// end, the byte there is '\n', and (nblk > 0) the byte at hash_off is ' ';
// the tokens themselves are decode_token's to check.
CIR_HD inline Head parse_head(const uint8_t* t, uint64_t p, uint64_t end, uint64_t bs) {
  Head h = {kDecline, 0, 0, 0};
  const uint64_t lim = end - p > kMaxHead + 1 ? p + kMaxHead + 1 : end;
  if (t[p] == '/') {
    const uint64_t e = token_end(t, p, lim, true, false);
    if (e == kBad || t[e] != '\n') return h;
    // literal components between the slashes: none is "." or ".." (a component
    // with an escape in it is neither: no escape decodes to '.')
    uint64_t c0 = p + 1;
    for (uint64_t i = p + 1; i <= e; ++i) {
      if (i == e || t[i] == '/') {
        const uint64_t n = i - c0;
        if ((n == 1 && t[c0] == '.') || (n == 2 && t[c0] == '.' && t[c0 + 1] == '.')) return h;
        c0 = i + 1;
      }
    }
    h.kind = kDir;
    return h;
  }
  if (end - p < 3 || t[p] != ' ' || t[p + 1] != ' ') return h;
  const uint64_t n0 = p + 2;
  const uint64_t ne = token_end(t, n0, lim, true, true);
  if (ne == kBad || ne == n0 || t[ne] != ' ') return h;
  if ((ne - n0 == 1 && t[n0] == '.') || (ne - n0 == 2 && t[n0] == '.' && t[n0 + 1] == '.'))
    return h;
  if (lim - ne < 4) return h;  // ' ', the type, ' ' and one byte more
  const uint8_t type = t[ne + 1];
  if (t[ne + 2] != ' ') return h;
  uint64_t q = ne + 3;
  if (type == 's') {
    const uint64_t te = token_end(t, q, lim, false, false);
    if (te == kBad || te == q || t[te] != '\n') return h;
    h.kind = kLink;
    return h;
  }
  if (type != 'f' && type != 'x') return h;
  // the size, as dirsig.cpp's parse_u64
  uint64_t x = 0;
  unsigned nd = 0;
  while (q < lim && t[q] >= '0' && t[q] <= '9') {
    if (++nd > 20) return h;
    const uint64_t nx = x * 10 + (uint64_t)(t[q] - '0');
    if (nx / 10 != x) return h;
    x = nx;
    ++q;
  }
  if (nd == 0 || q >= lim) return h;
  const uint64_t n = x / bs + (x % bs != 0);
  if (n == 0) {
    if (t[q] != '\n') return h;
  } else {
    if (t[q] != ' ') return h;
    if (n > (end - q) / kTokenBytes) return h;
    const uint64_t e = q + kTokenBytes * n;
    if (e >= end || t[e] != '\n') return h;
  }
  h.kind = kFile;
  h.size = x;
  h.nblk = n;
  h.hash_off = q;
  return h;
}

// Four hex digits in a little-endian word (the first digit in the low byte) to
// two bytes (the first in the low byte); *bad goes negative at a byte that is
// no hex digit.
CIR_HD inline uint32_t hex4(uint32_t w, int* bad) {
  const int a = hexval((uint8_t)w), b = hexval((uint8_t)(w >> 8));
  const int c = hexval((uint8_t)(w >> 16)), d = hexval((uint8_t)(w >> 24));
  *bad |= a | b | c | d;
  return ((((unsigned)a & 15u) << 4) | ((unsigned)b & 15u)) |
         (((((unsigned)c & 15u) << 4) | ((unsigned)d & 15u)) << 8);
}

// 16 hex digits in four such words to 8 bytes in two; false at a bad digit.
CIR_HD inline bool hex16(const uint32_t w[4], uint32_t out[2]) {
  int bad = 0;
  out[0] = hex4(w[0], &bad) | (hex4(w[1], &bad) << 16);
  out[1] = hex4(w[2], &bad) | (hex4(w[3], &bad) << 16);
  return bad >= 0;
}

// One hash token, ' ' + 64 hex digits at p (65 readable bytes), to 32 bytes
// (the host's form: the device decodes a quarter of a token per lane with
// hex16).  Little-endian hosts only, like the rest of the library.
inline bool decode_token(const uint8_t* p, uint8_t* out) {
  bool ok = p[0] == ' ';
  for (int j = 0; j < 4; ++j) {
    uint32_t w[4], o[2];
    __builtin_memcpy(w, p + 1 + 16 * j, 16);
    ok = hex16(w, o) && ok;
    __builtin_memcpy(out + 8 * j, o, 8);
  }
  return ok;
}

// A run record: one non-empty file of the index.
struct Run {
  uint64_t first;     // global block number of its block 0 (cir_check_blocks' numbering)
  uint64_t size;      // the entry's size
  uint64_t file;      // file ordinal, file entries only (cir_link_candidates')
  uint64_t hash_off;  // offset in the text of the first token's leading ' '
};

struct Counts {
  uint64_t files = 0, runs = 0, blocks = 0;
  uint64_t declined = kBad;  // start of the first declined line
};

// The host loop over the same rule: every body line through parse_head, every
// token through decode_token, in text order.  digests (32 B per block) and
// runs may be null (count only).  Stops at the first declined line.
inline Counts scan_host(const uint8_t* t, uint64_t body_off, uint64_t body_end, uint64_t bs,
                        uint8_t* digests, Run* runs) {
  Counts c;
  uint64_t p = body_off;
  if (p < body_end && t[p] != '/') {
    c.declined = p;
    return c;
  }
  while (p < body_end) {
    const Head h = parse_head(t, p, body_end, bs);
    if (h.kind == kDecline) {
      c.declined = p;
      return c;
    }
    if (h.kind == kFile) {
      uint8_t tmp[32];
      for (uint64_t k = 0; k < h.nblk; ++k)
        if (!decode_token(t + h.hash_off + kTokenBytes * k,
                          digests ? digests + 32 * (c.blocks + k) : tmp)) {
          c.declined = p;
          return c;
        }
      if (h.nblk) {
        if (runs) runs[c.runs] = Run{c.blocks, h.size, c.files, h.hash_off};
        ++c.runs;
        c.blocks += h.nblk;
      }
      ++c.files;
      p = h.hash_off + kTokenBytes * h.nblk + 1;
    } else {
      while (t[p] != '\n') ++p;  // (parse_head saw the '\n' before body_end)
      ++p;
    }
  }
  return c;
}

}  // namespace idxscan
}  // namespace cir
