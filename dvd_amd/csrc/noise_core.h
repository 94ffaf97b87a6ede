// The arithmetic of the keyed sampler noise and of the map deviation, shared by the kernels of noise.hip
// and by the stand-alone CPU restatement noise_host_check.cpp (plain C++, no HIP).  tests/noise_model.py is its NumPy statement
// and the definition.  Every f32 operation below is one that IEEE 754 rounds exactly (add, subtract, multiply, divide, sqrt,
// conversions, bit casts) and each is rounded on its own - no fused multiply-add, no library logarithm or sine - so NumPy
// float32 gives the same bits as the kernel.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dvd_hip.h"

#include "hd.h"
#include "philox.h"

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")     // the host restatement: g++ contracts across statements where the target has an FMA
#endif

namespace dvd {
namespace nz {

constexpr int kMinGrid = 2, kMaxGrid = 8192;   // g of [.,2,g,g]
constexpr int kMaxDocs = 65535, kMaxHyp = 65535;
constexpr uint32_t kStream = 2;                // c3 of every counter of this file (the corruptions own 0 and 1)
constexpr int kDevBlock = 256, kDevPer = 4;    // map deviation: threads per workgroup, grid points per thread
constexpr double kPx = 0.987 * 511;            // pixels of the 512 x 512 network input per unit of flow

// ---- separately rounded f32 operations, host and device -----------------------------------------------------------------
// (clang contracts only inside one expression, so a product returned from its own function is never fused; g++ is told above)
DVD_HD float fmul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}
DVD_HD float fadd(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}
DVD_HD float fsub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(a, b);
#else
  return a - b;
#endif
}
DVD_HD float fdiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
DVD_HD float fsqrt(float a) { return sqrtf(a); }
DVD_HD uint32_t bits_of(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
#endif
}
DVD_HD float float_of(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  memcpy(&f, &u, 4);
  return f;
#endif
}

// ---- -2 ln u for u = k 2^-24, k = 1 .. 2^24 -------------------------------------------------------------------------------
// u = 2^e m with m in (sqrt(1/2), sqrt 2]; ln m = 2 atanh s, s = f / (2 + f), f = m - 1 (exact), as the odd series
// 2 s + s z (2/3 + z (2/5 + z (2/7 + z (2/9 + z 2/11)))), z = s^2 <= 0.0295 (the first dropped term is below 2^-34 of the sum);
// ln u = e ln2_hi + (e ln2_lo + ln m), with ln2_hi of nine significant bits so that e ln2_hi is exact.  Working on f keeps
// the result relatively accurate near u = 1, where it is -f (1 + O(f)).
DVD_HD float neg2ln(uint32_t k) {
  const float u = fmul((float)k, 5.9604644775390625e-8f);          // exact: k <= 2^24
  const uint32_t b = bits_of(u);
  int e = (int)(b >> 23) - 127;
  float m = float_of((b & 0x7fffffu) | 0x3f800000u);               // [1, 2)
  if (m > 1.41421354f) {
    m = fmul(m, 0.5f);
    e += 1;
  }
  const float f = fsub(m, 1.f);
  const float s = fdiv(f, fadd(2.f, f));
  const float z = fmul(s, s);
  float p = (float)(2.0 / 11.0);
  p = fadd(fmul(p, z), (float)(2.0 / 9.0));
  p = fadd(fmul(p, z), (float)(2.0 / 7.0));
  p = fadd(fmul(p, z), (float)(2.0 / 5.0));
  p = fadd(fmul(p, z), (float)(2.0 / 3.0));
  const float lnm = fadd(fadd(s, s), fmul(fmul(s, z), p));
  const float fe = (float)e;
  const float ln = fadd(fmul(fe, 0.693359375f), fadd(fmul(fe, -2.12194440e-4f), lnm));
  return fmul(-2.f, ln);
}

// ---- cos and sin of 2 pi k 2^-24, k = 0 .. 2^24 - 1 -----------------------------------------------------------------------
// The reduction is exact, in integers: k = n 2^22 + r with r in [-2^21, 2^21), so the angle is n pi/2 + x, |x| <= pi/4, and
// x = r (2 pi 2^-24) is one rounded product.  sin x and cos x are their Taylor polynomials to x^9 and x^10 (remainders below
// 2^-28 and 2^-30); the quadrant swaps and negates them.
DVD_HD void cossin(uint32_t k, float* c, float* s) {
  const uint32_t n = (k + (1u << 21)) >> 22;                       // 0 .. 4
  const int r = (int)k - (int)(n << 22);
  const float x = fmul((float)r, (float)(6.283185307179586 / 16777216.0));
  const float x2 = fmul(x, x);
  float ps = (float)(1.0 / 362880.0);
  ps = fadd(fmul(ps, x2), (float)(-1.0 / 5040.0));
  ps = fadd(fmul(ps, x2), (float)(1.0 / 120.0));
  ps = fadd(fmul(ps, x2), (float)(-1.0 / 6.0));
  const float sn = fadd(x, fmul(fmul(x, x2), ps));
  float pc = (float)(-1.0 / 3628800.0);
  pc = fadd(fmul(pc, x2), (float)(1.0 / 40320.0));
  pc = fadd(fmul(pc, x2), (float)(-1.0 / 720.0));
  pc = fadd(fmul(pc, x2), (float)(1.0 / 24.0));
  const float cs = fadd(fsub(1.f, fmul(0.5f, x2)), fmul(fmul(x2, x2), pc));
  const uint32_t quad = n & 3;
  *c = quad == 0 ? cs : (quad == 1 ? -sn : (quad == 2 ? -cs : sn));
  *s = quad == 0 ? sn : (quad == 1 ? cs : (quad == 2 ? -sn : -cs));
}

// two normals from two words: u_a = ((wa >> 8) + 1) 2^-24 in (0, 1], u_b = (wb >> 8) 2^-24 in [0, 1)
DVD_HD void box_muller(uint32_t wa, uint32_t wb, float* z0, float* z1) {
  const float rad = fsqrt(neg2ln((wa >> 8) + 1));
  float c, s;
  cossin(wb >> 8, &c, &s);
  *z0 = fmul(rad, c);
  *z1 = fmul(rad, s);
}

// elements 4 q .. 4 q + 3 of hypothesis h of the document with key (k0, k1), draw `slot`
DVD_HD void quad_normals(uint32_t k0, uint32_t k1, uint32_t q, uint32_t slot, uint32_t h, float* z) {
  uint32_t w[4];
  philox(k0, k1, q, slot, h, kStream, w);
  box_muller(w[0], w[1], z, z + 1);
  box_muller(w[2], w[3], z + 2, z + 3);
}

// ---- map deviation: the distance of one grid point between two maps ---------------------------------------------------------
DVD_HD float point_distance(float ax, float ay, float bx, float by) {
  const float dx = fsub(ax, bx), dy = fsub(ay, by);
  return fsqrt(fadd(fmul(dx, dx), fmul(dy, dy)));
}

inline long deviation_blocks(int g) { return ((long)g * g + kDevBlock * kDevPer - 1) / (kDevBlock * kDevPer); }

// ---- the argument checks of the two entry points (no pointers), shared with the restatement ---------------------------------
inline int check_randn(int docs, int n_hyp, int g) {
  if (docs < 0 || docs > kMaxDocs || n_hyp < 0 || n_hyp > kMaxHyp || g < kMinGrid || g > kMaxGrid) return DVD_E_ARG;
  const unsigned long long quads = ((unsigned long long)2 * g * g + 3) / 4;
  return (unsigned long long)docs * n_hyp * quads > (1ull << 38) ? DVD_E_ARG : DVD_OK;
}
inline int check_deviation(int docs, int g) {
  return docs < 0 || docs > kMaxDocs || g < kMinGrid || g > kMaxGrid ? DVD_E_ARG : DVD_OK;
}

}  // namespace nz
}  // namespace dvd
