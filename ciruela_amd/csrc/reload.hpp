// What check.cpp's load pipeline and reload.cpp share: cir_load_blocks with a
// step between the index's parse and the first look at the image directory.
#pragma once
#include <functional>
#include <vector>

#include "runtime.hpp"
#include "stage.hpp"

namespace cir {

// Called once the index is parsed and the destinations are accepted, before any
// I/O: fills what it can of the destinations from memory on device `d` (the
// stream's) and leaves in *mem one bit per global block that now stands there
// (ceil(nblk_total / 64) words, the bits past the last block 0), or leaves *mem
// empty when it filled nothing.  A code other than CIR_OK ends the call.
using ResidentFn = std::function<int(const stage::Layout& image, Device& d, std::vector<uint64_t>* mem)>;

// cir_load_blocks (resident == nullptr), or the same with `resident` run first
// and the blocks it filled neither looked at nor read: they count as "have", a
// non-empty file made of them alone is CIR_FILE_COMPLETE | CIR_FILE_RESIDENT.
int load_blocks_resident(cir_ctx* ctx, int dirfd, const char* dir, const uint8_t* index, size_t len,
                         uint32_t threads, void* const* d_data, size_t ndata, void* stream,
                         const ResidentFn* resident, uint64_t** have_out, uint64_t* nblk_out,
                         uint8_t** state_out, int32_t** errno_out, size_t* nfiles_out,
                         uint64_t* stats);

}  // namespace cir
