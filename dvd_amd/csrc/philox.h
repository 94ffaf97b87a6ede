// Philox4x32-10 (Salmon et al. 2011), shared by the corruptions (corrupt_core.h) and the keyed sampler noise (noise_core.h) and by
// their stand-alone CPU restatements (plain C++, no HIP).  Who owns which counters: corrupt_core.h uses c3 in {0, 1},
// noise_core.h c3 = 2.
#pragma once
#include <stdint.h>

#include "hd.h"

namespace dvd {

// counter (c0..c3), key (k0, k1) -> four 32-bit words
DVD_HD void philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* out) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

}  // namespace dvd
