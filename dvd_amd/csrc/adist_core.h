// The arithmetic of the aligned-distortion chain (the fit of a translation and a scale to a flow field, the fixed-point
// resampling through that fit, and the gradient weight of the final mean), shared by the kernels of sflow.hip and by the
// stand-alone CPU restatement adist_host_check.cpp (plain C++, no HIP).  DESIGN.md section 4.8 holds the definition;
// tests/adist_model.py is its NumPy statement.  Everything here is a pure function of its arguments.
#pragma once
#include "hd.h"
#include "sflow_core.h"

namespace dvd {
namespace ad {

// The partial sums of the fit and of the weighted mean are cut like the LD sum: sf::kSelBlock consecutive pixels per partial,
// sf::kFinThreads lanes in the finalize.

// ---- fit ------------------------------------------------------------------------------------------------------------------
// centred coordinate, doubled so that it stays an integer: X = 2x - (w - 1)
DVD_HD int centred(int x, int w) { return 2 * x - (w - 1); }

// the closed form of sum over the plane of X^2: lines * n (n^2 - 1) / 3 (n (n^2 - 1) is a multiple of 3)
DVD_HD int64_t sum_sq(int lines, int n) { return (int64_t)lines * ((int64_t)n * ((int64_t)n * n - 1) / 3); }

// one Q16 coefficient: rint(num / den * 65536), one correctly rounded f64 division, ties to even; 0 for a zero denominator;
// saturated to +-(2^31 - 1) (out of reach of any flow the chain can produce, within reach of an arbitrary int16 field)
DVD_HD int32_t coef_q16(int64_t num, int64_t den) {
  if (den == 0) return 0;
  const double q = rint((double)num / (double)den * 65536.0);
  const double lim = 2147483647.0;
  return (int32_t)(q > lim ? lim : (q < -lim ? -lim : q));
}

// sums = (Su, Sxu, Sv, Syv) -> coef = (ax, bx, ay, by)
DVD_HD void fit_coefs(const int64_t* sums, int h, int w, int32_t* coef) {
  const int64_t n = (int64_t)h * w;
  coef[0] = coef_q16(sums[0], n);
  coef[1] = coef_q16(2 * sums[1], sum_sq(h, w));
  coef[2] = coef_q16(sums[2], n);
  coef[3] = coef_q16(2 * sums[3], sum_sq(w, h));
}

// ---- align ----------------------------------------------------------------------------------------------------------------
// the fitted position of coordinate x along an axis of n pixels, Q16, clamped into the plane
DVD_HD int64_t fitted_q16(int x, int n, int32_t a, int32_t b) {
  const int64_t c = ((int64_t)x << 16) + (int64_t)a + (((int64_t)b * (int64_t)centred(x, n)) >> 1);
  const int64_t hi = (int64_t)(n - 1) << 16;
  return c < 0 ? 0 : (c > hi ? hi : c);
}

DVD_HD int byte_at(const float* img, size_t i) {
  const int v = (int)img[i];
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
DVD_HD int byte_at(const uint8_t* img, size_t i) { return (int)img[i]; }

// B'(y, x): B at the fitted position, bilinear with 8-bit fractions
template <typename T>
DVD_HD int aligned_at(const T* img, int h, int w, int y, int x, const int32_t* coef) {
  const int64_t cx = fitted_q16(x, w, coef[0], coef[1]), cy = fitted_q16(y, h, coef[2], coef[3]);
  const int x0 = (int)(cx >> 16), y0 = (int)(cy >> 16);
  const int fx = (int)((cx >> 8) & 255), fy = (int)((cy >> 8) & 255);
  const int x1 = sf::mini(x0 + 1, w - 1), y1 = sf::mini(y0 + 1, h - 1);
  const int b00 = byte_at(img, (size_t)y0 * w + x0), b01 = byte_at(img, (size_t)y0 * w + x1);
  const int b10 = byte_at(img, (size_t)y1 * w + x0), b11 = byte_at(img, (size_t)y1 * w + x1);
  return ((256 - fx) * (256 - fy) * b00 + fx * (256 - fy) * b01 + (256 - fx) * fy * b10 + fx * fy * b11 + 32768) >> 16;
}

// ---- weights --------------------------------------------------------------------------------------------------------------
// g = floor(sqrt(gx^2 + gy^2)) of the scan's clamped central differences; at most floor(sqrt(2) 255) = 360
template <typename T>
DVD_HD int weight_at(const T* img, int h, int w, int y, int x) {
  int gx, gy;
  sf::gradient(img, h, w, y, x, &gx, &gy);
  return (int)sf::isqrt64((uint64_t)(gx * gx + gy * gy));
}

// |f| of an int16 field (64-bit under the root: -32768 squared twice leaves 32 bits), and one term of the numerator: two
// roundings, the root, then the product
DVD_HD double flow_len(int fu, int fv) { return sqrt((double)((int64_t)fu * fu + (int64_t)fv * fv)); }
DVD_HD double weighted_term(int g, double len) { return (double)g * len; }

// AD from the three sums: the weighted mean, or the plain mean for a scan without a gradient
DVD_HD double ad_value(double wsum, double lsum, int64_t gsum, int64_t count) {
  return gsum > 0 ? wsum / (double)gsum : lsum / (double)count;
}

}  // namespace ad
}  // namespace dvd
