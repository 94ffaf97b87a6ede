// The arithmetic of the scan-like page, shared by the kernels of clean.hip and by the stand-alone CPU
// restatement clean_host_check.cpp (plain C++, no HIP).  tests/clean_model.py is its NumPy statement and the definition.
// Everything is integer: the paper estimate (cell maxima, a closing, a tent rounded once), the flatten (a bilinear sample of the
// estimate in units of 1 / 4 s^2 and one 32-bit division per sample) and Sauvola's rule (window sums, an exact floor square
// root, one signed 64-bit comparison).  Sums and maxima may be taken in any order.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dvd_hip.h"

#include "hd.h"

namespace dvd {
namespace cl {

constexpr int kMaxSide = 16384;                // sides of the page: 1..kMaxSide
constexpr int kMaxClose = 8, kMaxSmooth = 8;   // the closing's and the tent's half-widths in cells: 0..8
constexpr int kMaxRadius = 63, kMaxKq = 256;   // Sauvola's window half-width 1..63 and round(256 k) 0..256
constexpr int kR = 128;                        // Sauvola's dynamic range of the standard deviation
constexpr int kBlock = 256, kPer = 4;          // threads of a workgroup, pixels of a thread (along x)
constexpr int kTileW = 64, kTileH = 16;        // page pixels of a flatten workgroup, and of one pass of a binarise workgroup

DVD_HD uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b) { return (r + 2 * g + b + 2) >> 2; }

// ---- the paper estimate ----------------------------------------------------------------------------------------------------
DVD_HD int clip_lo(int x, int r) { return x - r < 0 ? 0 : x - r; }
DVD_HD int clip_hi(int x, int r, int n) { return x + r > n - 1 ? n - 1 : x + r; }
// the cells of a window of half-width r around x that lie in 0..n-1
DVD_HD int win_count(int x, int n, int r) { return clip_hi(x, r, n) - clip_lo(x, r) + 1; }

// the tent's weight at distance d, |d| <= b
DVD_HD uint32_t tent_w(int d, int b) { return (uint32_t)(b + 1 - (d < 0 ? -d : d)); }
// the sum of the weights over the clipped window around x: at most (b + 1)^2 = 81
DVD_HD uint32_t tent_den(int x, int n, int b) {
  uint32_t den = 0;
  for (int i = clip_lo(x, b), hi = clip_hi(x, b, n); i <= hi; ++i) den += tent_w(i - x, b);
  return den;
}
// num <= 255 * 81 * 81 < 2^21, den <= 81 * 81: one rounding
DVD_HD uint32_t bg_round(uint32_t num, uint32_t den) { return (2 * num + den) / (2 * den); }

// ---- flatten ---------------------------------------------------------------------------------------------------------------
// A pixel between two cell centres: the cells i0 and i1, clamped to 0..n-1, and the weight f of i1 in units of 1 / 2s, 0..2s-1.
struct Axis {
  short i0, i1, f;
};

DVD_HD int log2_of(int s) { return s == 4 ? 2 : s == 8 ? 3 : s == 16 ? 4 : s == 32 ? 5 : 6; }

// u = 2x + 1 - s >= 1 - s, so u + 2s > 0 and floor(u / 2s) = ((u + 2s) >> log2(2s)) - 1
DVD_HD Axis flat_axis(int x, int s, int n) {
  const int u = 2 * x + 1 - s;
  const int i0 = ((u + 2 * s) >> (log2_of(s) + 1)) - 1;
  Axis a;
  a.f = (short)(u - 2 * s * i0);
  a.i0 = (short)(i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0));
  a.i1 = (short)(i0 + 1 > n - 1 ? n - 1 : i0 + 1);
  return a;
}

// 4 s^2 times the bilinear sample: at most 255 * 4 * 64^2 < 2^22
DVD_HD uint32_t bgq_of(uint32_t b00, uint32_t b01, uint32_t b10, uint32_t b11, int fx, int fy, int s) {
  const uint32_t ux = (uint32_t)fx, uy = (uint32_t)fy, s2 = (uint32_t)(2 * s);
  return (s2 - uy) * ((s2 - ux) * b00 + ux * b01) + uy * ((s2 - ux) * b10 + ux * b11);
}

// what a flatten counts, and what a binarise counts
struct Counts {
  unsigned saturated, floored, ink;
};

// one channel sample: v white 4 s^2 <= 255 * 255 * 16384 < 2^30, so numerator and quotient are 32-bit
DVD_HD uint32_t flatten_sample(uint32_t v, uint32_t white, int s, uint32_t bgq, Counts& n) {
  const uint32_t one = (uint32_t)(4 * s * s);
  if (bgq < one) {
    bgq = one;
    n.floored += 1;
  }
  const uint32_t q = (v * white * one + bgq / 2) / bgq;
  if (q > 255) {
    n.saturated += 1;
    return 255;
  }
  return q;
}

// ---- Sauvola ---------------------------------------------------------------------------------------------------------------
// floor(sqrt(d)) of d < 2^45, exactly: an f32 seed is less than 1 off, the two loops take it home
DVD_HD uint64_t isqrt_floor(uint64_t d) {
  uint64_t s = (uint64_t)sqrtf((float)d);
  while ((s + 1) * (s + 1) <= d) ++s;
  while (s * s > d) --s;
  return s;
}

// g of the pixel; n <= 127^2 pixels of the clipped window, s1 = sum g <= 255 n, s2 = sum g^2 <= 65025 n < 2^31.
// n s2 >= s1^2 (Cauchy-Schwarz); every product below stays under 2^52 in magnitude.
DVD_HD bool sauvola_ink(uint32_t g, uint32_t n, uint32_t s1, uint32_t s2, int kq) {
  const int64_t N = (int64_t)n, S1 = (int64_t)s1;
  const uint64_t d = (uint64_t)n * s2 - (uint64_t)s1 * s1;
  const int64_t sn = (int64_t)isqrt_floor(d);
  const int64_t a = 256 * (int64_t)kR * N;
  return (int64_t)g * N * a <= S1 * a + (int64_t)kq * S1 * (sn - kR * N);
}

// ---- the argument checks of the entry points, shared with the restatement: all before any HIP call ------------------------
inline bool cell_ok(int s) { return s == 4 || s == 8 || s == 16 || s == 32 || s == 64; }
inline int check_page(int h, int w) { return h >= 1 && h <= kMaxSide && w >= 1 && w <= kMaxSide ? DVD_OK : DVD_E_CLEAN_SHAPE; }
inline int check_background(int cell, int close, int smooth) {
  return cell_ok(cell) && close >= 0 && close <= kMaxClose && smooth >= 0 && smooth <= kMaxSmooth ? DVD_OK : DVD_E_CLEAN_PARAM;
}
inline int check_flatten(int cell, int white) { return cell_ok(cell) && white >= 1 && white <= 255 ? DVD_OK : DVD_E_CLEAN_PARAM; }
inline int check_binarize(int radius, int kq) {
  return radius >= 1 && radius <= kMaxRadius && kq >= 0 && kq <= kMaxKq ? DVD_OK : DVD_E_CLEAN_PARAM;
}
inline bool bytes_overlap(const void* a, size_t an, const void* b, size_t bn) {
  return a && b && (uintptr_t)a < (uintptr_t)b + bn && (uintptr_t)b < (uintptr_t)a + an;
}
inline int coarse(int n, int s) { return (n + s - 1) / s; }

}  // namespace cl
}  // namespace dvd
