// The host rule of cir_link_candidates (links.cpp), for cir_file_sources'
// host path and fallback (files.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cir {

// cir_link_candidates' arguments and outputs.  counts (nullable, written on
// CIR_OK): {file entries of the index, candidates, their bytes, file entries
// of the sources that take part, sources that take part}.
int candidates_impl(const uint8_t* index, size_t len, const uint8_t* const* src_index,
                    const size_t* src_len, size_t nsrc, uint64_t** file_out, uint32_t** src_out,
                    size_t* n_out, size_t* nskipped_out, uint64_t* counts);

}  // namespace cir
