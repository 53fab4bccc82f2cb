// A candidate's path decoded from the index text that holds it, in the form
// the index parser gives an entry's path ("/dir/name", raw bytes): what
// cir_file_copies and cir_fetch_plan report beside a content candidate
// (copies.cpp, plan.cpp).  The bytes are files.hpp's next_byte, which is the rule.
#pragma once
#include <stdint.h>

#include <string>

#include "files.hpp"

namespace cir {

// Appends the decoded token at t[off ..): the stretch before its first escape in
// one piece, the rest byte by byte (files::next_byte, which is the rule).
inline void append_token(const uint8_t* t, uint64_t len, uint64_t off, std::string* p) {
  const uint64_t lim = files::walk_lim(off, len);
  uint64_t i = off;
  while (i < lim && t[i] != ' ' && t[i] != '\n' && t[i] != '\\') ++i;
  p->append(reinterpret_cast<const char*>(t) + off, i - off);
  for (int c; (c = files::next_byte(t, &i, lim)) >= 0;) p->push_back((char)c);
}

// Appends the decoded path of the entry whose record holds (name_off, dir_off) in text t.
inline void decode_path(const uint8_t* t, uint64_t len, uint64_t dir_off, uint64_t name_off,
                        std::string* p) {
  const size_t at = p->size();
  append_token(t, len, dir_off, p);
  if (p->size() != at + 1) p->push_back('/');  // (every directory but "/" gets its separator)
  append_token(t, len, name_off, p);
}

}  // namespace cir
