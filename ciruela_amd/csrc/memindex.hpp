// What cir_index_emit, cir_index_memory_dev (memindex.cpp) and cir_store_blocks
// (store.cpp) share of the index over a flat file list: the checks of the
// list's arrays, the header of a hash type and block size, and the host emit
// of a laid-out list (emit.hpp) with its footer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dirsig.hpp"
#include "emit.hpp"

namespace cir {

// CIR_EINVAL ("null pointer") when an array of a non-empty list is missing.
int check_files(const uint8_t* paths, const uint64_t* path_off, const uint64_t* sizes,
                size_t nfiles);
// false: bs is not in 1 .. 2^32-1.
bool header_of(int hash_type, uint64_t bs, dirsig::Header* h);
// The index of `lay` over `digests` (lay.nblocks of 32 bytes, the caller's
// file order), emitted on the host: header, body, footer.  *index_out is the
// caller's to cir_free; image_id may be null.  CIR_ENOMEM.
int emit_index_host(const emit::Layout& lay, const dirsig::Header& h, const uint8_t* digests,
                    uint8_t** index_out, size_t* len_out, uint8_t* image_id);

}  // namespace cir
