// Four neighbouring pixels of an [H,W,3] uint8 picture as three dwords, to and from an address that may begin anywhere (a row
// begins anywhere when 3 W is no multiple of 4).  Device only; used by sized.hip and clean.hip.
#pragma once
#include <stdint.h>

namespace dvd {

// Twelve bytes d0 | d1 | d2 (little endian) to dst, which may begin anywhere: whole dwords where dst is on one, else
// head = 4 - (dst & 3) single bytes, the two dwords between, and the 4 - head bytes left.  Only shifts: no indexed registers.
__device__ __forceinline__ void store12(uint8_t* __restrict__ dst, uint32_t d0, uint32_t d1, uint32_t d2) {
  const unsigned m = (unsigned)((uintptr_t)dst & 3);
  if (m == 0) {
    uint32_t* p = reinterpret_cast<uint32_t*>(dst);
    p[0] = d0;
    p[1] = d1;
    p[2] = d2;
    return;
  }
  const unsigned head = 4 - m, sh = 8 * head;             // 1..3 bytes, 8..24 bits
  for (unsigned k = 0; k < head; ++k) dst[k] = (uint8_t)(d0 >> (8 * k));
  uint32_t* p = reinterpret_cast<uint32_t*>(dst + head);
  p[0] = d0 >> sh | d1 << (32 - sh);
  p[1] = d1 >> sh | d2 << (32 - sh);
  for (unsigned k = 0; k < m; ++k) dst[head + 8 + k] = (uint8_t)(d2 >> (sh + 8 * k));
}

// The twelve bytes at src as d0 | d1 | d2: whole dwords where src is on one, else the same head bytes, two dwords and tail
// bytes - no byte outside src[0..11] is read.
__device__ __forceinline__ void load12(const uint8_t* __restrict__ src, uint32_t& d0, uint32_t& d1, uint32_t& d2) {
  const unsigned m = (unsigned)((uintptr_t)src & 3);
  if (m == 0) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src);
    d0 = p[0];
    d1 = p[1];
    d2 = p[2];
    return;
  }
  const unsigned head = 4 - m, sh = 8 * head;
  uint32_t lo = 0, hi = 0;
  for (unsigned k = 0; k < head; ++k) lo |= (uint32_t)src[k] << (8 * k);
  const uint32_t* p = reinterpret_cast<const uint32_t*>(src + head);
  const uint32_t a = p[0], b = p[1];
  for (unsigned k = 0; k < m; ++k) hi |= (uint32_t)src[head + 8 + k] << (8 * k);
  d0 = lo | a << sh;
  d1 = a >> (32 - sh) | b << sh;
  d2 = b >> (32 - sh) | hi << sh;
}

// byte k (0..11, a constant after unrolling) of d0 | d1 | d2
__device__ __forceinline__ uint32_t byte12(uint32_t d0, uint32_t d1, uint32_t d2, int k) {
  return ((k < 4 ? d0 : (k < 8 ? d1 : d2)) >> (8 * (k & 3))) & 255u;
}

}  // namespace dvd
