// The arithmetic of the page at a chosen size, shared by the kernels of sized.hip and by the
// stand-alone CPU restatement sized_host_check.cpp (plain C++, no HIP).  tests/sized_model.py is its NumPy statement and the
// definition.  The unwarp tail's sampling grid at the PAGE's size (flowgrid_core.h) gives every page pixel a signed Q8 position
// on the photograph; the first differences of those positions give the radii of synth_core.h's integer tent, which here
// filters the photograph: a tap outside it contributes zero (padding_mode='zeros'), its weight still counts, and the result is
// rounded once.  Every f32 operation is one of noise_core.h's separately rounded ones; everything behind the Q8 position is
// integer.
#pragma once
#include "flowgrid_core.h"
#include "synth_core.h"

namespace dvd {
namespace sz {

using nz::bits_of;
using nz::fadd;
using nz::fmul;

constexpr int kMaxSide = 16384;                // sides of the photograph and of the page: 1..kMaxSide
constexpr int kMaxRadius = 16;                 // the tent's half-width in photograph pixels: 1..max_radius <= kMaxRadius
constexpr int kPad = kMaxRadius + 1;           // a position further outside the photograph is moved here: no tap reaches back
constexpr int kBlock = 256, kPer = 4;          // threads of a workgroup, pixels of a thread (along x: twelve bytes)
constexpr int kTileW = 64, kTileH = 16;        // page pixels of a workgroup
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;
constexpr int kNone = -2147483647 - 1;         // Pos::x of a pixel that is off the page or whose grid value is not finite

// the signed Q8 position of a page pixel on the photograph
struct Pos {
  int x, y;
};

struct Foot {
  int rx, ry;                                  // the tent's radii, 1..max_radius
  int capped;                                  // 1: a radius would have been larger
};

// what a call counts (DVD_SIZED_STATS words, in this order)
struct Counts {
  unsigned capped, outside, invalid;
};

DVD_HD bool finite_f32(float f) { return (bits_of(f) & 0x7f800000u) != 0x7f800000u; }

// floor(256 x + 1/2) of x = (g + 1) ((n - 1) / 2), clamped to [-256 kPad, 256 (n - 1 + kPad)]: both ends are exact in f32 and
// far below 2^31.  g is finite, so the value is never a NaN; an overflow to infinity takes the clamp.
DVD_HD int q8_of(float g, int n) {
  const float x = fmul(fadd(g, 1.f), fmul((float)(n - 1), 0.5f));
  const float t = floorf(fadd(fmul(x, 256.f), 0.5f));
  const float lo = (float)(-256 * kPad), hi = (float)(256 * (n - 1 + kPad));
  return !(t >= lo) ? (int)lo : (t > hi ? (int)hi : (int)t);
}

DVD_HD Pos pos_of(float gx, float gy, int hs, int ws) {
  Pos p;
  p.x = kNone;
  p.y = 0;
  if (finite_f32(gx) && finite_f32(gy)) {
    p.x = q8_of(gx, ws);
    p.y = q8_of(gy, hs);
  }
  return p;
}

// sy::radius_of without its cap: at least 1.  |a|, |b| <= 2 * 256 * (kMaxSide + 2 kPad) < 2^24.
DVD_HD int radius_raw(int a, int b) {
  a = a < 0 ? -a : a;
  b = b < 0 ? -b : b;
  const int r = ((a > b ? a : b) + 255) >> 9;
  return r < 1 ? 1 : r;
}

// At: Pos operator()(int dy, int dx), the neighbourhood of a valid page pixel; off the page, and where the grid is not finite,
// it answers kNone and the difference goes without that neighbour (sy::diff2)
template <class At>
DVD_HD Foot foot_at(const At& at, int max_radius) {
  const Pos c = at(0, 0), l = at(0, -1), r = at(0, 1), u = at(-1, 0), d = at(1, 0);
  const bool hl = l.x != kNone, hr = r.x != kNone, hu = u.x != kNone, hd = d.x != kNone;
  const int ux = radius_raw(sy::diff2(c.x, hl, l.x, hr, r.x), sy::diff2(c.x, hu, u.x, hd, d.x));
  const int uy = radius_raw(sy::diff2(c.y, hl, l.y, hr, r.y), sy::diff2(c.y, hu, u.y, hd, d.y));
  Foot f;
  f.rx = ux < max_radius ? ux : max_radius;
  f.ry = uy < max_radius ? uy : max_radius;
  f.capped = ux > max_radius || uy > max_radius ? 1 : 0;
  return f;
}

DVD_HD bool centre_outside(const Pos& c, int hs, int ws) { return c.x < 0 || c.x > 256 * (ws - 1) || c.y < 0 || c.y > 256 * (hs - 1); }

// radii 1 x 1: Q8 bilinear sampling with zeros outside - the tent below with its four taps written out (s & 255 is the
// fraction above floor(s / 256) for a negative s too).  The sum is at most 65536 * 255: 32 bits.
DVD_HD void bilinear_at(const uint8_t* __restrict__ src, int hs, int ws, int sx, int sy, uint32_t* rgb) {
  const int x0 = sx >> 8, y0 = sy >> 8;
  const uint32_t fx = (uint32_t)(sx & 255), fy = (uint32_t)(sy & 255);
  const bool l = x0 >= 0 && x0 < ws, r = x0 + 1 >= 0 && x0 + 1 < ws;
  uint32_t top[3] = {0, 0, 0}, bot[3] = {0, 0, 0};
  if (y0 >= 0 && y0 < hs) {
    const uint8_t* row = src + 3 * ((size_t)y0 * ws + (l ? x0 : 0));
    for (int q = 0; q < 3; ++q) top[q] = (l ? (256 - fx) * row[q] : 0u) + (r ? fx * row[(l ? 3 : 3 * (x0 + 1)) + q] : 0u);
  }
  if (y0 + 1 >= 0 && y0 + 1 < hs) {
    const uint8_t* row = src + 3 * ((size_t)(y0 + 1) * ws + (l ? x0 : 0));
    for (int q = 0; q < 3; ++q) bot[q] = (l ? (256 - fx) * row[q] : 0u) + (r ? fx * row[(l ? 3 : 3 * (x0 + 1)) + q] : 0u);
  }
  for (int q = 0; q < 3; ++q) rgb[q] = ((256 - fy) * top[q] + fy * bot[q] + 32768) >> 16;
}

// The separable tent of half-width rx x ry photograph pixels: 2 rx columns and 2 ry rows from floor(s / 256) - r + 1 on, weight
// 256 r - |256 c - s| >= 0; a tap outside the photograph is left out of the sum and stays in the divisor.  With r <= 16 a
// row's sum is at most 256 rx^2 * 255 <= 2^16 * 255 < 2^24 (32 bits); the rows add up to at most W * 255 < 2^40 with
// W = 65536 rx^2 ry^2 <= 2^32 (64 bits).  (acc + W / 2) / W = ((acc + 2^15 q) >> 16) / q with q = rx^2 ry^2 <= 65536 - a floor
// of a floor is the floor - and (acc + 2^15 q) >> 16 <= 255 q + q / 2 < 2^24, so the division is one of 32 bits.
DVD_HD void tent_at(const uint8_t* __restrict__ src, int hs, int ws, int sx, int sy, int rx, int ry, uint32_t* rgb) {
  unsigned long long acc[3] = {0, 0, 0};
  const int c0 = (sx >> 8) - rx + 1, r0 = (sy >> 8) - ry + 1;
  const int i0 = c0 < 0 ? -c0 : 0, i1 = c0 + 2 * rx > ws ? ws - c0 : 2 * rx;        // the columns c0 + i0 .. c0 + i1 - 1 exist
  const int j0 = r0 < 0 ? -r0 : 0, j1 = r0 + 2 * ry > hs ? hs - r0 : 2 * ry;
  for (int j = j0; j < j1; ++j) {
    const int r = r0 + j, dy = 256 * r - sy;
    const uint32_t wy = (uint32_t)(256 * ry - (dy < 0 ? -dy : dy));
    const uint8_t* row = src + 3 * (size_t)r * ws;
    uint32_t sum[3] = {0, 0, 0};
    for (int i = i0; i < i1; ++i) {
      const int c = c0 + i, dx = 256 * c - sx;
      const uint32_t wx = (uint32_t)(256 * rx - (dx < 0 ? -dx : dx));
      const uint8_t* t = row + 3 * c;
      for (int q = 0; q < 3; ++q) sum[q] += wx * t[q];
    }
    for (int q = 0; q < 3; ++q) acc[q] += (unsigned long long)wy * sum[q];
  }
  const uint32_t q2 = (uint32_t)(rx * rx * ry * ry);
  for (int q = 0; q < 3; ++q) rgb[q] = (uint32_t)((acc[q] + ((unsigned long long)q2 << 15)) >> 16) / q2;
}

// One page pixel: black where the grid is not finite.
template <class At>
DVD_HD void pixel_at(const uint8_t* __restrict__ src, int hs, int ws, const At& at, int max_radius, uint32_t* rgb, Counts& n) {
  const Pos c = at(0, 0);
  if (c.x == kNone) {
    rgb[0] = rgb[1] = rgb[2] = 0;
    n.invalid += 1;
    return;
  }
  const Foot f = foot_at(at, max_radius);
  n.capped += (unsigned)f.capped;
  n.outside += centre_outside(c, hs, ws) ? 1u : 0u;
  if (f.rx == 1 && f.ry == 1)
    bilinear_at(src, hs, ws, c.x, c.y, rgb);
  else
    tent_at(src, hs, ws, c.x, c.y, f.rx, f.ry, rgb);
}

// rx | ry << 8 of a page pixel, 0 where the grid is not finite
template <class At>
DVD_HD uint16_t radii_at(const At& at, int max_radius) {
  if (at(0, 0).x == kNone) return 0;
  const Foot f = foot_at(at, max_radius);
  return (uint16_t)(f.rx | f.ry << 8);
}

// ---- the argument checks of the entry points, shared with the restatement: all before any HIP call ------------------------
inline int check_shape(int g, int hs, int ws, int hp, int wp) {
  const bool sides = hs >= 1 && hs <= kMaxSide && ws >= 1 && ws <= kMaxSide && hp >= 1 && hp <= kMaxSide && wp >= 1 && wp <= kMaxSide;
  return sides && g >= nz::kMinGrid && g <= nz::kMaxGrid ? DVD_OK : DVD_E_SIZED_SHAPE;
}
inline int check_params(float scale, int max_radius) {
  return finite_f32(scale) && max_radius >= 1 && max_radius <= kMaxRadius ? DVD_OK : DVD_E_SIZED_PARAM;
}
// null pointers, and a page that shares bytes with its photograph (out may be null where an entry point writes no page)
inline bool bytes_overlap(const void* a, size_t an, const void* b, size_t bn) {
  return (uintptr_t)a < (uintptr_t)b + bn && (uintptr_t)b < (uintptr_t)a + an;
}
inline size_t image_bytes(int h, int w) { return 3 * (size_t)h * (size_t)w; }
inline int check_pointers(const void* flow, const void* src, const void* out, int hs, int ws, int hp, int wp) {
  if (!flow || !src || !out) return DVD_E_ARG;
  return bytes_overlap(src, image_bytes(hs, ws), out, image_bytes(hp, wp)) ? DVD_E_ARG : DVD_OK;
}

}  // namespace sz
}  // namespace dvd
