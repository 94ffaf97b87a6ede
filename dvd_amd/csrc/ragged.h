// Per-document table of the ragged (one size per document) batch kernels: dvd_unwarp_u8_ragged (warp.hip) and
// dvd_ingest_u8_ragged (ingest.hip).  It travels BY VALUE as a kernel argument (structure of arrays, so one document's
// field is one scalar load at a wave-uniform index): nothing is allocated or copied for it, and the host array the caller
// passed is not read after the entry point returns.
#pragma once
#include "common.h"

namespace dvd {

// Documents per launch (DVD_RAGGED_CAP of include/dvd_hip.h): 64 x 28 B = 1792 B of kernel argument here, plus
// 64 x 20 B = 1280 B of up-sampling scales for the tail - 3.1 KiB of the 4 KiB a HIP kernel may take.
constexpr int kRaggedCap = DVD_RAGGED_CAP;

struct RaggedTab {
  const uint8_t* src[kRaggedCap];
  uint8_t* out[kRaggedCap];
  int h[kRaggedCap], w[kRaggedCap];
  unsigned tile_end[kRaggedCap];   // inclusive prefix sum of the documents' tile counts: document d owns the blocks
                                   // [tile_end[d-1], tile_end[d]) of the flat 1-D grid (a document may own none)
  int n;
};

// The document of a block: the first d with tile < tile_end[d] (tile < tile_end[n-1] by the launch).  blockIdx and the
// table are wave-uniform, so the search runs on the scalar unit; readfirstlane states it for what is indexed with d.
__device__ __forceinline__ int ragged_doc_of(const RaggedTab& tab, unsigned tile) {
  int lo = 0, hi = tab.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tile >= tab.tile_end[mid]) lo = mid + 1;
    else hi = mid;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

}  // namespace dvd
