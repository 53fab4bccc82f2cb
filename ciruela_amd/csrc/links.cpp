// cir_link_candidates: which files of a new image may be hardlinked from
// older images of the same base directory (host only).
//
// Reference: scan_links (src/daemon/metadata/hardlink_sources.rs:107-153)
// walks the new index's entries in order and, for every file entry, the
// entries the older images' indexes hold at the same path, in the order
// files_to_hardlink ranked the images (newest first, :66-72): the first one
// that is a file with the same exe flag, size and hashes (:131-133) makes a
// Hardlink and ends the search (the break at :143).  An older index that
// cannot be read is left out with a warning (:95-101).  The walk itself is
// MergedSignatures of the external dir-signature crate, which the reference
// tree does not hold: what is restated here is what :121-146 show of it.
#include <stdlib.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "dirsig.hpp"
#include "links.hpp"
#include "runtime.hpp"

namespace cir {

int candidates_impl(const uint8_t* index, size_t len, const uint8_t* const* src_index,
                    const size_t* src_len, size_t nsrc, uint64_t** file_out, uint32_t** src_out,
                    size_t* n_out, size_t* nskipped_out, uint64_t* counts) {
  if (!index || !file_out || !src_out || !n_out || (nsrc && (!src_index || !src_len)))
    return fail(CIR_EINVAL, "null pointer");
  *file_out = nullptr;
  *src_out = nullptr;
  *n_out = 0;
  if (nskipped_out) *nskipped_out = 0;
  dirsig::Index idx;
  std::string err;
  if (!dirsig::parse(index, len, &idx, &err))
    return idx.bad_hash_size ? fail(CIR_EHASHSIZE, "hash size is unsupported: " + err)
                             : fail(CIR_EPARSE, "error parsing index: " + err);
  // the sources that take part, each with its file entries by path
  struct Source {
    uint32_t ordinal;
    dirsig::Index idx;
    std::unordered_map<std::string, const dirsig::Entry*> files;
  };
  std::vector<Source> sources;
  sources.reserve(nsrc);
  size_t skipped = 0;
  for (size_t j = 0; j < nsrc; ++j) {
    Source s;
    s.ordinal = (uint32_t)j;
    std::string serr;
    if (!src_index[j] || !dirsig::parse(src_index[j], src_len[j], &s.idx, &serr) ||
        s.idx.header.hash != idx.header.hash ||
        s.idx.header.block_size != idx.header.block_size) {
      ++skipped;
      continue;
    }
    sources.push_back(std::move(s));
  }
  // (the maps point into the indexes: filled once `sources` no longer moves)
  for (Source& s : sources)
    for (const dirsig::Entry& en : s.idx.entries)
      if (en.kind == dirsig::EntryKind::kFile) s.files.emplace(en.path, &en);
  std::vector<uint64_t> files;
  std::vector<uint32_t> srcs;
  uint64_t ordinal = 0, bytes = 0, pool_files = 0;
  for (const Source& s : sources)
    for (const dirsig::Entry& en : s.idx.entries) pool_files += en.kind == dirsig::EntryKind::kFile;
  for (const dirsig::Entry& en : idx.entries) {
    if (en.kind != dirsig::EntryKind::kFile) continue;
    for (const Source& s : sources) {
      const auto hit = s.files.find(en.path);
      if (hit == s.files.end()) continue;
      const dirsig::Entry& t = *hit->second;
      if (t.exe == en.exe && t.size == en.size && t.hashes == en.hashes) {
        files.push_back(ordinal);
        srcs.push_back(s.ordinal);
        bytes += en.size;
        break;
      }
    }
    ++ordinal;
  }
  if (nskipped_out) *nskipped_out = skipped;
  if (counts) {
    counts[0] = ordinal;
    counts[1] = files.size();
    counts[2] = bytes;
    counts[3] = pool_files;
    counts[4] = sources.size();
  }
  if (files.empty()) return CIR_OK;
  uint64_t* f = (uint64_t*)malloc(files.size() * sizeof(uint64_t));
  uint32_t* s = (uint32_t*)malloc(srcs.size() * sizeof(uint32_t));
  if (!f || !s) {
    free(f);
    free(s);
    return fail(CIR_ENOMEM, "malloc");
  }
  memcpy(f, files.data(), files.size() * sizeof(uint64_t));
  memcpy(s, srcs.data(), srcs.size() * sizeof(uint32_t));
  *file_out = f;
  *src_out = s;
  *n_out = files.size();
  return CIR_OK;
}

}  // namespace cir

extern "C" int cir_link_candidates(const uint8_t* index, size_t len,
                                   const uint8_t* const* src_index, const size_t* src_len,
                                   size_t nsrc, uint64_t** file_out, uint32_t** src_out,
                                   size_t* n_out, size_t* nskipped_out) try {
  return cir::candidates_impl(index, len, src_index, src_len, nsrc, file_out, src_out, n_out,
                              nskipped_out, nullptr);
} CIR_CATCH_BOUNDARY
