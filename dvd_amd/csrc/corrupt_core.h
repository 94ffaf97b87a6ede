// The integer arithmetic of the common corruptions, shared by the kernels of corrupt.hip and by the
// stand-alone CPU restatement corrupt_host_check.cpp (plain C++, no HIP).  tests/corrupt_model.py is its NumPy statement and
// the definition.  Everything marked DVD_HD is a pure function of its arguments; the table builders at the end are host code
// (double, libm) that the library runs once and hands out through dvd_corrupt_table.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/dvd_hip.h"

#include "hd.h"
#include "philox.h"

namespace dvd {
namespace cr {

constexpr int kKinds = 19;
constexpr int kMinSide = 32;          // one reflection suffices for 24 taps either way
constexpr int kMaxSide = 16384;       // the zoom's Q8 coordinates stay below 2^31
constexpr int kMaxTaps = 49;          // largest FIR side (gaussian_blur, severity 5)
constexpr int kMaxRadius = kMaxTaps / 2;
constexpr int kMotionSide = 41;       // largest motion_blur side (r = 20)
constexpr int kAngles = 91;           // motion_blur: -45 .. 45 degrees
constexpr int kShotMax = 60;          // largest photon count c of shot_noise = entries per row of its CDF table
constexpr int kIrwinMean = 6 * 65535; // mean of twelve 16-bit uniforms

enum Kind {
  kGaussianNoise = 0, kShotNoise = 1, kImpulseNoise = 2, kDefocusBlur = 3, kGlassBlur = 4, kMotionBlur = 5, kZoomBlur = 6,
  kSnow = 7, kFrost = 8, kFog = 9, kBrightness = 10, kContrast = 11, kElastic = 12, kPixelate = 13, kJpeg = 14,
  kSpeckleNoise = 15, kGaussianBlur = 16, kSpatter = 17, kSaturate = 18
};

// 1: a kernel of corrupt.hip; 2: delivered by the JPEG codec's entry points; 0: refused
inline int supported(int kind) {
  switch (kind) {
    case kGaussianNoise: case kShotNoise: case kImpulseNoise: case kDefocusBlur: case kMotionBlur: case kZoomBlur:
    case kBrightness: case kContrast: case kPixelate: case kSpeckleNoise: case kGaussianBlur: return 1;
    case kJpeg: return 2;
    default: return 0;
  }
}
inline bool is_fir(int kind) { return kind == kDefocusBlur || kind == kMotionBlur || kind == kGaussianBlur; }

// What a launch needs of (kind, severity): every constant of the issue's table as the integer the arithmetic uses.
struct Params {
  int kind, severity;
  int64_t gain;        // kind 0: rint(255 sigma 2^16); kind 15: rint(c 2^16)
  uint32_t t_hi, t_lo; // kind 2: u < t_hi -> 255, u < t_lo -> 0 (floor(p/2 2^32), floor(p 2^32))
  int photons;         // kind 1: c
  int side;            // FIR kinds: taps per side
  int zooms, zstep;    // kind 6: zoom k is (100 + k zstep) / 100, k = 0 .. zooms - 1
  int lift;            // kind 10: rint(255 c), ties to even
  int keep;            // kind 11: rint(c 2^16)
  int cells;           // kind 13: c in hundredths
};

inline Params params_for(int kind, int severity) {
  static const int sigma_milli[5] = {80, 120, 180, 260, 380}, speckle[5] = {15, 20, 35, 45, 60};
  static const int impulse[5] = {3, 6, 9, 17, 27}, photons[5] = {60, 25, 12, 5, 3};
  static const int defocus_r[5] = {3, 4, 6, 8, 10}, motion_r[5] = {10, 15, 15, 15, 20}, gauss_sigma[5] = {1, 2, 3, 4, 6};
  static const int zstep[5] = {1, 1, 2, 2, 3}, zend[5] = {111, 116, 121, 126, 133};
  static const int lift[5] = {26, 51, 76, 102, 128};      // rint(255 c) for c = .1 .. .5 (25.5 -> 26, 76.5 -> 76, 127.5 -> 128)
  static const int keep[5] = {40, 30, 20, 10, 5}, cells[5] = {60, 50, 40, 30, 25};
  const int s = severity - 1;
  Params p = {};
  p.kind = kind;
  p.severity = severity;
  if (kind == kGaussianNoise) p.gain = (255ll * sigma_milli[s] * 65536 + 500) / 1000;
  if (kind == kSpeckleNoise) p.gain = (speckle[s] * 65536ll + 50) / 100;
  p.t_lo = (uint32_t)(((uint64_t)impulse[s] << 32) / 100);
  p.t_hi = (uint32_t)(((uint64_t)impulse[s] << 32) / 200);
  p.photons = photons[s];
  if (kind == kDefocusBlur) p.side = 2 * (defocus_r[s] + (defocus_r[s] > 8 ? 2 : 1)) + 1;
  if (kind == kMotionBlur) p.side = 2 * motion_r[s] + 1;
  if (kind == kGaussianBlur) p.side = 2 * 4 * gauss_sigma[s] + 1;
  p.zstep = zstep[s];
  p.zooms = (zend[s] - 100 + zstep[s] - 1) / zstep[s];
  p.lift = lift[s];
  p.keep = (keep[s] * 65536 + 50) / 100;
  p.cells = cells[s];
  return p;
}

// ---- Philox4x32-10 (philox.h): counter (c0..c3), key (k0, k1) -> four 32-bit words ---------------------------------------
// The counter of the corruptions: c0 = the element's index in its image, c1 = the draw, c2 = the kind, c3 = 0 for an element's
// noise and 1 for a parameter of the whole image.
using dvd::philox;

DVD_HD int clamp255(int64_t v) { return v < 0 ? 0 : (v > 255 ? 255 : (int)v); }

// z 2^16: twelve 16-bit uniforms (draws 0 and 1 of kind 0: four words, then two) minus their mean; variance 2^32 - 1
DVD_HD int irwin_hall(uint32_t k0, uint32_t k1, uint32_t elem) {
  uint32_t a[4], b[4];
  philox(k0, k1, elem, 0, kGaussianNoise, 0, a);
  philox(k0, k1, elem, 1, kGaussianNoise, 0, b);
  int s = 0;
  for (int i = 0; i < 4; ++i) s += (int)(a[i] & 0xffff) + (int)(a[i] >> 16);
  for (int i = 0; i < 2; ++i) s += (int)(b[i] & 0xffff) + (int)(b[i] >> 16);
  return s - kIrwinMean;
}

// kinds 0 and 15: x + round(gain t / 2^32) and x + round(x gain t / 2^32); the shift of a negative value floors
DVD_HD int gaussian_px(int x, int64_t gain, int t) { return clamp255(x + ((gain * t + ((int64_t)1 << 31)) >> 32)); }
DVD_HD int speckle_px(int x, int64_t gain, int t) { return clamp255(x + ((x * gain * t + ((int64_t)1 << 31)) >> 32)); }

DVD_HD int impulse_px(int x, uint32_t u, uint32_t t_hi, uint32_t t_lo) { return u < t_hi ? 255 : (u < t_lo ? 0 : x); }

// kind 1: row = the c thresholds floor(CDF(j) 2^32) of Poisson(x c / 255), j = 0 .. c - 1 (saturated to 2^32 - 1);
// k = how many lie below u, then round(255 k / c)
DVD_HD int shot_px(uint32_t u, const uint32_t* row, int c) {
  int k = 0;
  while (k < c && row[k] < u) ++k;
  return (2 * 255 * k + c) / (2 * c);
}

// reflect-101 for an index at most n - 1 beyond either border; further out (lanes of a tile that lie outside the image) it
// saturates, so that the result always names a pixel
DVD_HD int reflect101(int i, int n) {
  i = i < 0 ? -i : (i > n - 1 ? 2 * (n - 1) - i : i);
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// kind 6: the source coordinate of output x under a centre-anchored zoom of zc / 100, Q8: (n-1)/2 + (x - (n-1)/2) 100 / zc
DVD_HD uint32_t zoom_coord(int x, int n, int zc) { return ((uint32_t)((n - 1) * (zc - 100) + 200 * x) << 7) / (uint32_t)zc; }

// one bilinear sample in Q16 (weights 256 - a and a per axis); p(y, x) reads a channel of the image
template <typename Px>
DVD_HD int bilinear_q16(Px p, int h, int w, uint32_t cy, uint32_t cx) {
  const int y0 = (int)(cy >> 8), x0 = (int)(cx >> 8), ay = (int)(cy & 255), ax = (int)(cx & 255);
  const int y1 = y0 + 1 < h ? y0 + 1 : h - 1, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
  return (256 - ay) * ((256 - ax) * p(y0, x0) + ax * p(y0, x1)) + ay * ((256 - ax) * p(y1, x0) + ax * p(y1, x1));
}

// the image itself plus its `zooms` zooms (zoom 0 is the identity), one rounding
template <typename Px>
DVD_HD int zoom_px(Px p, int h, int w, int y, int x, int zooms, int zstep) {
  int acc = p(y, x) << 16;
  for (int k = 0; k < zooms; ++k) {
    const int zc = 100 + k * zstep;
    acc += bilinear_q16(p, h, w, zoom_coord(y, h, zc), zoom_coord(x, w, zc));
  }
  const int den = (zooms + 1) << 16;
  return (acc + den / 2) / den;
}

// kind 10: HSV value + lift, hue and saturation kept
DVD_HD void brightness_px(int r, int g, int b, int lift, int* out) {
  const int v = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int v2 = v + lift < 255 ? v + lift : 255;
  if (v == 0) {
    out[0] = out[1] = out[2] = v2;
    return;
  }
  out[0] = (2 * r * v2 + v) / (2 * v);
  out[1] = (2 * g * v2 + v) / (2 * v);
  out[2] = (2 * b * v2 + v) / (2 * v);
}

// kind 11: the channel's mean in Q8 from its exact sum, then mean (1 - c) + c x
DVD_HD uint32_t mean_q8(uint64_t sum, uint64_t pixels) { return (uint32_t)((sum * 256 + pixels / 2) / pixels); }
DVD_HD int contrast_px(int x, uint32_t mean8, int keep) {
  return clamp255((int64_t)(((uint64_t)mean8 * (uint32_t)(65536 - keep) + (uint64_t)(x * 256) * (uint32_t)keep + (1u << 23)) >> 24));
}

// kind 13: n -> m = floor(n c / 100) cells; output x lies in cell floor((2x + 1) m / (2n)); cell i overlaps source pixel s by
// min((s+1) m, (i+1) n) - max(s m, i n) of n units
DVD_HD int cells_of(int n, int c100) { return n * c100 / 100; }
DVD_HD int cell_of(int x, int n, int m) { return (int)(((int64_t)(2 * x + 1) * m) / (2 * n)); }
DVD_HD int overlap(int s, int i, int n, int m) {
  const int64_t lo = (int64_t)s * m > (int64_t)i * n ? (int64_t)s * m : (int64_t)i * n;
  const int64_t hi = (int64_t)(s + 1) * m < (int64_t)(i + 1) * n ? (int64_t)(s + 1) * m : (int64_t)(i + 1) * n;
  return hi > lo ? (int)(hi - lo) : 0;
}
template <typename Px>
DVD_HD int pixelate_px(Px p, int h, int w, int y, int x, int c100) {
  const int mh = cells_of(h, c100), mw = cells_of(w, c100);
  const int iy = cell_of(y, h, mh), ix = cell_of(x, w, mw);
  const int y0 = (int)((int64_t)iy * h / mh), x0 = (int)((int64_t)ix * w / mw);
  uint64_t acc = 0;
  for (int sy = y0; sy < h; ++sy) {
    const int oy = overlap(sy, iy, h, mh);
    if (!oy) break;
    uint64_t row = 0;
    for (int sx = x0; sx < w; ++sx) {
      const int ox = overlap(sx, ix, w, mw);
      if (!ox) break;
      row += (uint64_t)ox * p(sy, sx);
    }
    acc += row * oy;
  }
  const uint64_t area = (uint64_t)h * w;
  return (int)((acc + area / 2) / area);
}

// ---- host: the real-valued tables, built in double and quantised once ----------------------------------------------------
// kind 1: thresholds [256][c]
inline std::vector<uint32_t> shot_table(int severity) {
  const int c = params_for(kShotNoise, severity).photons;
  std::vector<uint32_t> t((size_t)256 * c);
  for (int x = 0; x < 256; ++x) {
    const double lam = (double)x * c / 255.0;
    double p = exp(-lam), cdf = 0.0;
    for (int j = 0; j < c; ++j) {
      if (j) p = p * lam / j;
      cdf += p;
      const double q = floor(cdf * 4294967296.0);
      t[(size_t)x * c + j] = q >= 4294967295.0 ? 0xffffffffu : (uint32_t)q;
    }
  }
  return t;
}

// non-negative weights -> Q16 that sum to exactly 65536: each rint(w / sum 2^16), the first largest takes the remainder
inline std::vector<uint32_t> quantise_q16(const std::vector<double>& wt) {
  double sum = 0.0;
  for (double v : wt) sum += v;
  std::vector<uint32_t> q(wt.size());
  int64_t total = 0;
  size_t top = 0;
  for (size_t i = 0; i < wt.size(); ++i) {
    q[i] = (uint32_t)rint(wt[i] / sum * 65536.0);
    total += q[i];
    if (q[i] > q[top]) top = i;
  }
  q[top] = (uint32_t)((int64_t)q[top] + 65536 - total);
  return q;
}

// FIR weights [side][side] of kinds 3, 5 (angle in degrees, -45 .. 45) and 16
inline std::vector<uint32_t> fir_table(int kind, int severity, int angle) {
  static const double alias[5] = {0.1, 0.5, 0.5, 0.5, 0.5}, motion_sigma[5] = {3, 5, 8, 12, 15}, gauss_sigma[5] = {1, 2, 3, 4, 6};
  const int side = params_for(kind, severity).side, r = side / 2, s = severity - 1;
  std::vector<double> wt((size_t)side * side, 0.0);
  if (kind == kGaussianBlur) {
    for (int y = -r; y <= r; ++y)
      for (int x = -r; x <= r; ++x) wt[(size_t)(y + r) * side + x + r] = exp(-(double)(x * x + y * y) / (2.0 * gauss_sigma[s] * gauss_sigma[s]));
  } else if (kind == kDefocusBlur) {
    const int g = r > 10 ? 2 : 1, rd = r - g;             // r = rd + g: the disk's radius rd (g = 2 above 8), the alias Gaussian's 2 g + 1 taps
    double gw[5], gsum = 0.0;
    for (int i = -g; i <= g; ++i) gsum += gw[i + g] = exp(-(double)(i * i) / (2.0 * alias[s] * alias[s]));
    for (int i = 0; i <= 2 * g; ++i) gw[i] /= gsum;
    for (int dy = -rd; dy <= rd; ++dy)
      for (int dx = -rd; dx <= rd; ++dx) {
        if (dx * dx + dy * dy > rd * rd) continue;
        for (int j = -g; j <= g; ++j)
          for (int i = -g; i <= g; ++i) wt[(size_t)(dy + j + r) * side + dx + i + r] += gw[j + g] * gw[i + g];
      }
  } else {
    const double th = (double)angle * 3.14159265358979323846 / 180.0, cs = cos(th), sn = sin(th);
    for (int i = -r; i <= r; ++i) {
      const double gi = exp(-(double)(i * i) / (2.0 * motion_sigma[s] * motion_sigma[s]));
      const double fx = i * cs, fy = i * sn, x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0;
      const double w4[4] = {(1 - ay) * (1 - ax), (1 - ay) * ax, ay * (1 - ax), ay * ax};
      for (int k = 0; k < 4; ++k) {
        const int x = (int)x0 + (k & 1), y = (int)y0 + (k >> 1);
        if (w4[k] > 0.0 && x >= -r && x <= r && y >= -r && y <= r) wt[(size_t)(y + r) * side + x + r] += gi * w4[k];
      }
    }
  }
  return quantise_q16(wt);
}

// motion_blur's angle of an image: word 0 of the image's parameter draw, mod 91, minus 45
DVD_HD int motion_angle(uint32_t k0, uint32_t k1) {
  uint32_t o[4];
  philox(k0, k1, 0, 0, kMotionBlur, 1, o);
  return (int)(o[0] % kAngles) - 45;
}

}  // namespace cr
}  // namespace dvd
