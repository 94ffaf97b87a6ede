// The integer arithmetic of the local-distortion chain (dense SIFT, the cost volume, min-sum BP, the argmin and the LD sum),
// shared by the kernels of sflow.hip and by the stand-alone CPU restatement sflow_host_check.cpp (plain C++, no HIP).
// DESIGN.md section 4.7 holds the definition; tests/sflow_model.py is its NumPy statement.
// Everything here is a pure function of its arguments.  How the work is spread over lanes is the caller's business: the
// kernels call these per pixel, per label or per tap, the CPU program calls them in plain loops.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dvd_hip.h"

#include "hd.h"

namespace dvd {
namespace sf {

constexpr int kMaxLevels = 6;
constexpr int kMaxWin = 10;
constexpr int kMaxLabels = (2 * kMaxWin + 1) * (2 * kMaxWin + 1);   // 441
constexpr int kMinTop = DVD_SFLOW_MIN_TOP;
constexpr int kMaxSide = 8192;
constexpr int kMaxIters = 1000;
constexpr int kDesc = 128;            // bytes of a descriptor: 4 x 4 cells x 8 orientations
constexpr int kSelBlock = 256;        // pixels per partial of the LD sum (row-major pixel index / 256)
constexpr int kFinThreads = 256;      // lanes of the finalize: lane t adds partials t, t + 256, ... in order, then a tree

DVD_HD int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
DVD_HD int absi(int v) { return v < 0 ? -v : v; }
DVD_HD int mini(int a, int b) { return a < b ? a : b; }

// ---- dense descriptor -----------------------------------------------------------------------------------------------------
// gx, gy: central differences with clamped indices
template <typename T>
DVD_HD void gradient(const T* img, int h, int w, int y, int x, int* gx, int* gy) {
  const T* row = img + (size_t)y * w;
  *gx = (int)row[clampi(x + 1, w)] - (int)row[clampi(x - 1, w)];
  *gy = (int)img[(size_t)clampi(y + 1, h) * w + x] - (int)img[(size_t)clampi(y - 1, h) * w + x];
}

// r_o = max(0, gx C[o] + gy S[o]): 1024 (cos, sin) of o * 45 degrees; at most 510 * 724 = 369 240
DVD_HD int response(int gx, int gy, int o) {
  const int C[8] = {1024, 724, 0, -724, -1024, -724, 0, 724};
  const int S[8] = {0, 724, 1024, 724, 0, -724, -1024, -724};
  const int v = gx * C[o] + gy * S[o];
  return v > 0 ? v : 0;
}

// floor(sqrt(s)) exactly: the f64 root (s < 2^53 converts exactly), then a correction of one either way
DVD_HD uint32_t isqrt64(uint64_t s) {
  uint64_t r = (uint64_t)sqrt((double)s);
  if (r * r > s) --r;
  if ((r + 1) * (r + 1) <= s) ++r;
  return (uint32_t)r;
}

// one byte: min(255, 512 h / (n + eps)).  h <= 9 * 369 240, so 512 h < 2^31; n < 2^26 and eps <= 2^30
DVD_HD uint32_t quantise(int hk, uint32_t norm, int eps) {
  const uint32_t q = ((uint32_t)hk * 512u) / (norm + (uint32_t)eps);
  return q > 255u ? 255u : q;
}

// the cell centre of histogram row / column i = 0..3 of pixel coordinate y
DVD_HD int cell_at(int y, int i, int n) { return clampi(y + 3 * i - 5, n); }

// ---- pyramid --------------------------------------------------------------------------------------------------------------
// out(i, j) = (sum_k sum_l w_k w_l I(clamp(2i + k - 2), clamp(2j + l - 2)) + 128) >> 8, w = [1,4,6,4,1]
DVD_HD int reduce2_at(const uint8_t* img, int h, int w, int i, int j) {
  const int wt[5] = {1, 4, 6, 4, 1};
  int acc = 0;
  for (int k = 0; k < 5; ++k) {
    const uint8_t* row = img + (size_t)clampi(2 * i + k - 2, h) * w;
    int r = 0;
    for (int l = 0; l < 5; ++l) r += wt[l] * (int)row[clampi(2 * j + l - 2, w)];
    acc += wt[k] * r;
  }
  return (acc + 128) >> 8;
}

// ---- cost -----------------------------------------------------------------------------------------------------------------
// four bytes of the L1 distance, accumulating: v_sad_u8 on the device
DVD_HD uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sad_u8(a, b, acc);
#else
  for (int k = 0; k < 4; ++k) {
    const int x = (int)((a >> (8 * k)) & 255u), y = (int)((b >> (8 * k)) & 255u);
    acc += (uint32_t)(x > y ? x - y : y - x);
  }
  return acc;
#endif
}

// a, b: 32 words each (128 bytes)
DVD_HD uint32_t sad128(const uint32_t* a, const uint32_t* b) {
  uint32_t s = 0;
  for (int k = 0; k < 32; ++k) s = sad4(a[k], b[k], s);
  return s;
}

// Dc(p, l) from the distance (or `outside`) and the absolute flow
DVD_HD int data_cost(bool inside, uint32_t dist, int fu, int fv, int gamma, int T) {
  const int c = inside ? mini(T, (int)dist) : T;
  return c + gamma * (absi(fu) + absi(fv));
}

// ---- smoothness -----------------------------------------------------------------------------------------------------------
// one component of V: min(alpha |delta|, d)
DVD_HD int penalty(int alpha, int d, int delta) { return mini(alpha * absi(delta), d); }

// The message of sender q to receiver p from hq[l_q] = Dc(q, l_q) + the three other messages into q, as two passes over an
// n x n label grid (label index v * n + u), before the subtraction of its minimum.  du0 = o_u(p) - o_u(q), dv0 likewise:
//   t[v'][u] = min_u' hq[v'][u'] + pen(du0 + u - u')        out[v][u] = min_v' t[v'][u] + pen(dv0 + v - v')
// One element of each pass, so that a kernel can give one element to a lane:
template <typename A>
DVD_HD int minconv_u(const A& hq, int n, int vq, int u, int du0, int alpha, int d) {
  int best = 0x7fffffff;
  for (int uq = 0; uq < n; ++uq) best = mini(best, (int)hq[vq * n + uq] + penalty(alpha, d, du0 + u - uq));
  return best;
}
template <typename A>
DVD_HD int minconv_v(const A& t, int n, int v, int u, int dv0, int alpha, int d) {
  int best = 0x7fffffff;
  for (int vq = 0; vq < n; ++vq) best = mini(best, (int)t[vq * n + u] + penalty(alpha, d, dv0 + v - vq));
  return best;
}

// The four directions of the 4-connected grid.  Sender q = (y, x) writes slot `slot` of receiver p = (y + dy, x + dx) and
// leaves out the message it got from p, which lies in its own slot `excl`.  Slot k of a pixel holds the message from its
// left (0), right (1), upper (2) and lower (3) neighbour; the slot of an absent neighbour is never written and stays 0.
DVD_HD void direction(int k, int* dy, int* dx, int* slot, int* excl) {
  *dy = k == 2 ? 1 : (k == 3 ? -1 : 0);
  *dx = k == 0 ? 1 : (k == 1 ? -1 : 0);
  *slot = k;
  *excl = k ^ 1;
}

// ---- LD -------------------------------------------------------------------------------------------------------------------
DVD_HD double flow_length(int fu, int fv) { return sqrt((double)(fu * fu + fv * fv)); }

// ---- parameters and sizes (host) ------------------------------------------------------------------------------------------
struct LevelDims { int h[kMaxLevels], w[kMaxLevels]; };

inline LevelDims level_dims(int h, int w, int levels) {
  LevelDims dm;
  for (int l = 0; l < kMaxLevels; ++l) {
    dm.h[l] = h;
    dm.w[l] = w;
    if (l + 1 < levels) { h = (h + 1) / 2; w = (w + 1) / 2; }
  }
  return dm;
}

// the largest |f_u| (or |f_v|) level `l` can reach: the top window, doubled per level, plus each lower level's own window
inline long flow_bound(const dvd_sflow_params& p, int l) {
  long b = p.w_top;
  for (int k = p.levels - 2; k >= l; --k) b = 2 * b + p.w;
  return b;
}

// nullptr, or why the parameters are refused
inline const char* check_params(const dvd_sflow_params& p) {
  if (p.levels < 1 || p.levels > kMaxLevels) return "levels outside 1..6";
  if (p.w_top < 1 || p.w_top > kMaxWin || p.w < 1 || p.w > kMaxWin) return "a window outside 1..10";
  if (p.iters_top < 1 || p.iters_top > kMaxIters || p.iters < 1 || p.iters > kMaxIters) return "iterations outside 1..1000";
  if (p.alpha < 0 || p.alpha > 65535) return "alpha outside 0..65535";
  if (p.d < 0 || 2L * p.d > 65535) return "d breaks the 16-bit bound of a message (2 d <= 65535)";
  if (p.gamma < 0 || p.gamma > 65535 || p.T < 0 || p.T > 65535) return "gamma or T outside 0..65535";
  if ((long)p.T + (long)p.gamma * 2 * flow_bound(p, 0) > 65535) return "T breaks the 16-bit bound of a cost (T + gamma |f|_1 <= 65535)";
  if (p.eps < 1 || p.eps > (1 << 30)) return "eps outside 1..2^30";
  return nullptr;
}

inline const char* check_shape(int h, int w, const dvd_sflow_params& p) {
  if (h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return "a side outside 1..8192";
  const LevelDims dm = level_dims(h, w, p.levels);
  if (dm.h[p.levels - 1] < kMinTop || dm.w[p.levels - 1] < kMinTop) return "a side of the top level below 12";
  return nullptr;
}

// one level's window and iterations
inline int level_win(const dvd_sflow_params& p, int l) { return l == p.levels - 1 ? p.w_top : p.w; }
inline int level_iters(const dvd_sflow_params& p, int l) { return l == p.levels - 1 ? p.iters_top : p.iters; }

}  // namespace sf
}  // namespace dvd
