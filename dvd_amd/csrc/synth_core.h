// The arithmetic of the synthetic-document render, shared by the kernels of synth.hip and by the
// stand-alone CPU restatement synth_host_check.cpp (plain C++, no HIP).  tests/synth_model.py is its NumPy statement and the
// definition.  A flat scan is drawn on the photograph through fwd, the forward field dvd_map_invert writes (photograph pixel ->
// page position): Q8 scan positions, an integer tent filter whose radii follow the field's first differences, optional
// shading in Q16 and a 3 x 3 coverage blend at the page's edge.  Every f32 operation is one of noise_core.h's separately rounded
// ones; everything behind the Q8 position is integer.
#pragma once
#include "noise_core.h"

namespace dvd {
namespace sy {

using nz::bits_of;
using nz::fadd;
using nz::fdiv;
using nz::fmul;
using nz::fsub;

constexpr int kMaxSide = 16384;                // sides of the scan and of the photograph: 1..kMaxSide
constexpr int kMaxRadius = 8;                  // the tent's half-width in scan pixels: 1..kMaxRadius
constexpr uint32_t kInvalid = 0xffffffffu;     // fwd's bit pattern at a pixel the page does not cover
constexpr int kBlock = 256, kPer = 4;          // threads of a workgroup, pixels of a thread (along x: twelve bytes, three dwords)
constexpr int kTileW = 64, kTileH = 16;        // photograph pixels of a workgroup
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;

typedef dvd_synth_params Params;

// the Q8 scan position of a photograph pixel; x < 0: the page does not cover it
struct Pos {
  int x, y;
};
constexpr int kUncovered = -1;

// what the first differences of a pixel's neighbourhood give: twice the derivatives (integers: the central difference is not
// halved) and the tent's radii
struct Foot {
  int xx, xy, yx, yy;                          // 2 d(sx)/d(px), 2 d(sx)/d(py), 2 d(sy)/d(px), 2 d(sy)/d(py)
  int rx, ry;
};

DVD_HD float axis_scale(int ns, int n) { return n > 1 ? fdiv((float)(ns - 1), (float)(n - 1)) : 0.f; }

// floor(u k 256 + 1/2) clamped to [0, 256 (ns - 1)]; a NaN gives 0
DVD_HD int scan_q8(float u, float k, int ns) {
  const float f = floorf(fadd(fmul(fmul(u, k), 256.f), 0.5f));
  const int cap = 256 * (ns - 1);              // at most 2^22: exact in f32
  return !(f >= 0.f) ? 0 : (f > (float)cap ? cap : (int)f);
}

DVD_HD Pos pos_of(float u, float v, float kx, float ky, int hs, int ws) {
  Pos p;
  p.x = kUncovered;
  p.y = 0;
  if (bits_of(u) != kInvalid) {
    p.x = scan_q8(u, kx, ws);
    p.y = scan_q8(v, ky, hs);
  }
  return p;
}

// twice the derivative from the covered neighbours: the central difference, a doubled one-sided difference, or 0
DVD_HD int diff2(int c, bool has_l, int l, bool has_r, int r) {
  return has_l && has_r ? r - l : (has_r ? 2 * (r - c) : (has_l ? 2 * (c - l) : 0));
}

// The larger of two derivatives, in scan pixels, to the nearest integer (a half rounds down) in 1..kMaxRadius: a and b are doubled
// Q8 derivatives, 512 per scan pixel.  A scan minified by up to 1.5 is still sampled bilinearly.
DVD_HD int radius_of(int a, int b) {
  a = a < 0 ? -a : a;
  b = b < 0 ? -b : b;
  const int r = ((a > b ? a : b) + 255) >> 9;
  return r < 1 ? 1 : (r > kMaxRadius ? kMaxRadius : r);
}

// At: Pos operator()(int dy, int dx), the neighbourhood of a covered pixel; off the image it answers "uncovered"
template <class At>
DVD_HD Foot foot_at(const At& at) {
  const Pos c = at(0, 0), l = at(0, -1), r = at(0, 1), u = at(-1, 0), d = at(1, 0);
  const bool hl = l.x >= 0, hr = r.x >= 0, hu = u.x >= 0, hd = d.x >= 0;
  Foot f;
  f.xx = diff2(c.x, hl, l.x, hr, r.x);
  f.yx = diff2(c.y, hl, l.y, hr, r.y);
  f.xy = diff2(c.x, hu, u.x, hd, d.x);
  f.yy = diff2(c.y, hu, u.y, hd, d.y);
  f.rx = radius_of(f.xx, f.xy);
  f.ry = radius_of(f.yx, f.yy);
  return f;
}

// the covered pixels of the 3 x 3 window, the centre among them
template <class At>
DVD_HD int covered9(const At& at) {
  int n = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) n += at(dy, dx).x >= 0;
  return n;
}

// radii 1 x 1: Q8 bilinear sampling.  The sum is at most 65536 * 255: 32 bits.
DVD_HD void bilinear_at(const uint8_t* __restrict__ scan, int hs, int ws, int sx, int sy, uint32_t* rgb) {
  const int x0 = sx >> 8, y0 = sy >> 8;
  const int x1 = x0 + 1 < ws ? x0 + 1 : ws - 1, y1 = y0 + 1 < hs ? y0 + 1 : hs - 1;
  const uint32_t fx = (uint32_t)(sx & 255), fy = (uint32_t)(sy & 255);
  const uint8_t* r0 = scan + 3 * (size_t)y0 * ws;
  const uint8_t* r1 = scan + 3 * (size_t)y1 * ws;
  for (int q = 0; q < 3; ++q) {
    const uint32_t top = (256 - fx) * r0[3 * x0 + q] + fx * r0[3 * x1 + q];
    const uint32_t bot = (256 - fx) * r1[3 * x0 + q] + fx * r1[3 * x1 + q];
    rgb[q] = ((256 - fy) * top + fy * bot + 32768) >> 16;
  }
}

// The separable tent of half-width rx x ry scan pixels: 2 rx columns and 2 ry rows from floor(s / 256) - r + 1 on, weight
// 256 r - |256 c - s| >= 0, the taps clamped to the scan.  A row's sum is at most 256 rx^2 * 255 < 2^23 (32 bits); the rows add
// up to at most W * 255 < 2^37 with W = 65536 rx^2 ry^2 (64 bits).  (acc + W / 2) / W = ((acc + 2^15 q) >> 16) / q with
// q = rx^2 ry^2 <= 4096 - a floor of a floor is the floor - so the division is one of 32 bits.
DVD_HD void tent_at(const uint8_t* __restrict__ scan, int hs, int ws, int sx, int sy, int rx, int ry, uint32_t* rgb) {
  unsigned long long acc[3] = {0, 0, 0};
  const int c0 = (sx >> 8) - rx + 1, r0 = (sy >> 8) - ry + 1;
  for (int j = 0; j < 2 * ry; ++j) {
    const int r = r0 + j, dy = 256 * r - sy;
    const uint32_t wy = (uint32_t)(256 * ry - (dy < 0 ? -dy : dy));
    const uint8_t* row = scan + 3 * (size_t)(r < 0 ? 0 : (r > hs - 1 ? hs - 1 : r)) * ws;
    uint32_t sum[3] = {0, 0, 0};
    for (int i = 0; i < 2 * rx; ++i) {
      const int c = c0 + i, dx = 256 * c - sx;
      const uint32_t wx = (uint32_t)(256 * rx - (dx < 0 ? -dx : dx));
      const uint8_t* t = row + 3 * (c < 0 ? 0 : (c > ws - 1 ? ws - 1 : c));
      for (int q = 0; q < 3; ++q) sum[q] += wx * t[q];
    }
    for (int q = 0; q < 3; ++q) acc[q] += (unsigned long long)wy * sum[q];
  }
  const uint32_t q2 = (uint32_t)(rx * rx * ry * ry);
  for (int q = 0; q < 3; ++q) rgb[q] = (uint32_t)((acc[q] + ((unsigned long long)q2 << 15)) >> 16) / q2;
}

// all-zero parameters: no shading (a_ref is not looked at)
DVD_HD bool shading_on(const Params& p) { return p.l0 != 0.f || p.lgx != 0.f || p.lgy != 0.f || p.k != 0.f; }

// Lq = clamp(rint(65536 L), 0, 131072), L = l0 + lgx (px / (w - 1) - 1/2) + lgy (py / (h - 1) - 1/2) + k (A / a_ref - 1); A = the
// scan area of the photograph pixel, |xx yy - xy yx| / 4 in Q8 x Q8 units (through f64, where the integer is exact, so that the
// conversion to f32 rounds once).  A NaN gives 0.
DVD_HD uint32_t shade_q16(const Params& p, int px, int py, int h, int w, const Foot& f) {
  const float tx = fsub(w > 1 ? fdiv((float)px, (float)(w - 1)) : 0.f, 0.5f);
  const float ty = fsub(h > 1 ? fdiv((float)py, (float)(h - 1)) : 0.f, 0.5f);
  long long det = (long long)f.xx * f.yy - (long long)f.xy * f.yx;
  det = det < 0 ? -det : det;
  const float area = fmul((float)(double)det, 3.814697265625e-6f);          // 2^-18
  float L = fadd(p.l0, fmul(p.lgx, tx));
  L = fadd(L, fmul(p.lgy, ty));
  L = fadd(L, fmul(p.k, fsub(fdiv(area, p.a_ref), 1.f)));
  const float t = fmul(L, 65536.f);
  return !(t >= 0.f) ? 0u : (t >= 131072.f ? 131072u : (uint32_t)rintf(t));
}

DVD_HD uint32_t shade(uint32_t c, uint32_t lq) {
  const uint32_t v = (c * lq + 32768) >> 16;
  return v > 255 ? 255 : v;
}

// the soft edge: n of the window's nine pixels show the page, the others the background
DVD_HD uint32_t edge_blend(uint32_t page, uint32_t bg, int n) { return (page * (uint32_t)n + bg * (uint32_t)(9 - n) + 4) / 9; }

// One photograph pixel.  bg: its background colour; shade_on = shading_on(prm), hoisted.
template <class At>
DVD_HD void pixel_at(const uint8_t* __restrict__ scan, int hs, int ws, const At& at, int px, int py, int h, int w, const uint32_t* bg,
                     const Params& prm, bool shade_on, uint32_t* rgb) {
  const Pos c = at(0, 0);
  if (c.x < 0) {
    rgb[0] = bg[0];
    rgb[1] = bg[1];
    rgb[2] = bg[2];
    return;
  }
  const Foot f = foot_at(at);
  if (f.rx == 1 && f.ry == 1)
    bilinear_at(scan, hs, ws, c.x, c.y, rgb);
  else
    tent_at(scan, hs, ws, c.x, c.y, f.rx, f.ry, rgb);
  if (shade_on) {
    const uint32_t lq = shade_q16(prm, px, py, h, w, f);
    for (int q = 0; q < 3; ++q) rgb[q] = shade(rgb[q], lq);
  }
  const int n = covered9(at);
  if (n < 9)
    for (int q = 0; q < 3; ++q) rgb[q] = edge_blend(rgb[q], bg[q], n);
}

// ---- the argument checks of the entry points (no pointers), shared with the restatement ------------------------------------
inline int check_size(int hs, int ws, int h, int w) {
  return hs < 1 || hs > kMaxSide || ws < 1 || ws > kMaxSide || h < 1 || h > kMaxSide || w < 1 || w > kMaxSide ? DVD_E_SYNTH_SHAPE : DVD_OK;
}
inline int check_params(const Params& p) {
  if (!isfinite(p.l0) || !isfinite(p.lgx) || !isfinite(p.lgy) || !isfinite(p.k) || !isfinite(p.a_ref)) return DVD_E_SYNTH_PARAM;
  return shading_on(p) && !(p.a_ref > 0.f) ? DVD_E_SYNTH_PARAM : DVD_OK;
}

}  // namespace sy
}  // namespace dvd
