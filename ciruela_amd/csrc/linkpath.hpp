// The paths cir_check_links_at takes from its caller (which took them from
// another party's index, through cir_file_copies): split into components and
// validated before any I/O.  No HIP, no I/O; compiled by check.cpp and, under
// the sanitizers, by tools/copies_fuzz.cpp.
//
// A path is split at '/'; a leading '/' is allowed and empty components are
// dropped.  The empty path means "the entry's own path" (kOwn).  A "." or ".."
// component, or a non-empty path without any component (slashes only), makes
// the whole call invalid (kInvalid): nothing below a source root is reached
// through either, and every component is then opened with O_DIRECTORY |
// O_NOFOLLOW below the root fd.  A component that holds a NUL byte cannot be
// handed to openat(2) whole (kNul): that candidate alone is unreadable.
// kInvalid wins over kNul.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace cir {
namespace linkpath {

enum Verdict { kOwn = 0, kOk = 1, kInvalid = 2, kNul = 3 };

// comps (cleared first): the components of p[0 .. n), the last one the name.
// Filled for kOk only; unspecified otherwise.
inline Verdict split(const uint8_t* p, size_t n, std::vector<std::string>* comps) {
  comps->clear();
  if (n == 0) return kOwn;
  bool nul = false;
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && p[j] != '/') ++j;
    if (j > i) {
      const size_t len = j - i;
      if ((len == 1 && p[i] == '.') || (len == 2 && p[i] == '.' && p[i + 1] == '.')) return kInvalid;
      for (size_t k = i; k < j; ++k) nul = nul || p[k] == 0;
      comps->emplace_back(reinterpret_cast<const char*>(p + i), len);
    }
    i = j + 1;
  }
  if (comps->empty()) return kInvalid;
  return nul ? kNul : kOk;
}

}  // namespace linkpath
}  // namespace cir
