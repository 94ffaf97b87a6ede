// The arithmetic of the map score: a predicted map against a ground-truth map - end-point error,
// PCK, Fl and the sparsification curves.  Shared by the kernels of mapscore.hip and by the stand-alone CPU restatement
// mapscore_host_check.cpp (plain C++, no HIP); tests/mapscore_model.py is its NumPy statement and the definition.  Every f32
// operation is rounded on its own (noise_core.h's helpers), the up-sampling is flowviz_core.h's full_uv_at, counts and the
// fixed-point sums are integers: NumPy gives the same bits as the kernels.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dvd_hip.h"

#include "flowviz_core.h"
#include "hd.h"
#include "noise_core.h"

namespace dvd {
namespace ms {

using fv::full_uv_at;
using fv::Up;
using nz::bits_of;
using nz::fadd;
using nz::fdiv;
using nz::float_of;
using nz::fmul;
using nz::fsqrt;
using nz::fsub;

constexpr int kMaxSide = 16384, kMinGrid = 2, kMaxGrid = 8192, kMaxHyp = 64;
constexpr int kBlock = 256, kPer = 4;                  // map_errors: threads of a workgroup, pixels of a thread
constexpr int kPartial = 7;                            // 8-byte words of a block partial: n_valid, n1, n3, n5, n_fl, sum e, sum e^2
constexpr int kMaxRanks = 50;                          // order statistics selected at once = slots of the LDS histogram
constexpr int kGridCap = 256;                          // workgroups of the selection and of the bins (they stride over the plane)
constexpr int kBinWords = 4;                           // count, #(e <= 1), #(e <= 5), sum of e in fixed point
constexpr uint32_t kInvalid = 0xffffffffu;             // the planes' value at a pixel that enters nothing (a NaN pattern)
constexpr float kUnknown = 1e9f;                       // the Middlebury unknown-flow rule: |component| above it
constexpr float kFixCap = 32768.f, kFixScale = 1048576.f;   // e saturates at 2^15 px in the fixed-point sum: 2^28 px * 2^35 <= 2^63

// the device state of a selection between its levels, per rank; level L reads half L & 1 and writes the other
struct SelState {
  uint32_t prefix[2][kMaxRanks];      // the digits found so far (non-decreasing in the rank, as the ranks are)
  uint32_t rem[2][kMaxRanks];         // the rank among the keys that share the prefix
};
struct Ranks {
  uint32_t r[kMaxRanks];
};

DVD_HD bool finite1(float x) { return (bits_of(x) & 0x7f800000u) != 0x7f800000u; }
// a ground-truth component that counts: finite and at most 1e9 in magnitude
DVD_HD bool known(float x) { return finite1(x) && fabsf(x) <= kUnknown; }

DVD_HD float length2(float x, float y) { return fsqrt(fadd(fmul(x, x), fmul(y, y))); }

// Fl-KITTI-2015 of one pixel as the reference writes it: e > 3 and e / m > 0.05; m = 0 gives e / m = inf, an outlier
DVD_HD bool fl_outlier(float e, float m) { return e > 3.f && fdiv(e, m) > 0.05f; }

// rint(min(e, 2^15) 2^20): the scaling is exact, so the only rounding is rint's
DVD_HD unsigned long long fixed_of(float e) { return (unsigned long long)rintf(fmul(e < kFixCap ? e : kFixCap, kFixScale)); }

// The spread of n_hyp hypotheses [n_hyp,2,g,g] at pixel (i, j): sqrt((1/H) sum_h |d_h - mean|^2), sums over h = 0, 1, .. in f32.
// *ok = every up-sampled component is finite.  n_hyp >= 2.
DVD_HD float spread_at(const float* hyps, int n_hyp, const Up& up, int i, int j, bool* ok) {
  const size_t per = (size_t)2 * up.g * up.g;
  float su = 0.f, sv = 0.f, u, v;
  for (int h = 0; h < n_hyp; ++h) {
    full_uv_at(hyps + h * per, up, i, j, &u, &v);
    su = fadd(su, u);
    sv = fadd(sv, v);
  }
  *ok = finite1(su) && finite1(sv);
  const float mu = fdiv(su, (float)n_hyp), mv = fdiv(sv, (float)n_hyp);
  float s = 0.f;
  for (int h = 0; h < n_hyp; ++h) {
    full_uv_at(hyps + h * per, up, i, j, &u, &v);
    const float du = fsub(u, mu), dv = fsub(v, mv);
    s = fadd(s, fadd(fmul(du, du), fmul(dv, dv)));
  }
  *ok = *ok && finite1(s);
  return fsqrt(fdiv(s, (float)n_hyp));
}

// One pixel: prediction (pu, pv), ground truth (gu, gv), spread sigma with its flag.  Returns whether the pixel is valid; then
// *e and *m are the end-point error and the ground truth's length.
DVD_HD bool pixel_error(float pu, float pv, float gu, float gv, bool sigma_ok, float* e, float* m) {
  if (!known(gu) || !known(gv) || !finite1(pu) || !finite1(pv) || !sigma_ok) return false;
  *e = length2(fsub(gu, pu), fsub(gv, pv));
  *m = length2(gu, gv);
  return finite1(*e);
}

// ---- selection: the digit and the prefix of a key at a level (0 .. 3, most significant byte first) -------------------------------
DVD_HD uint32_t sel_prefix(uint32_t key, int level) { return level ? key >> (32 - 8 * level) : 0u; }
DVD_HD uint32_t sel_digit(uint32_t key, int level) { return (key >> (24 - 8 * level)) & 255u; }
// the slot whose prefix is p, or -1: binary search of an ascending table
DVD_HD int sel_slot(const uint32_t* table, int nslots, uint32_t p) {
  int lo = 0, hi = nslots;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (table[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo < nslots && table[lo] == p ? lo : -1;
}
// The live slots of a level: the distinct prefixes of the k ranks, ascending (equal ones are neighbours).  Returns their number and
// writes them to table[]; *slot_of = the slot of rank `which`.
DVD_HD int sel_slots(const uint32_t* prefix, int k, int which, uint32_t* table, int* slot_of) {
  int n = 0;
  for (int r = 0; r < k; ++r) {
    if (r == 0 || prefix[r] != prefix[r - 1]) table[n++] = prefix[r];
    if (r == which) *slot_of = n - 1;
  }
  return n;
}
// the digit of a rank from its slot's histogram: the first bin that holds it; *rem becomes its rank inside that bin
DVD_HD uint32_t sel_walk(const uint32_t* hist, uint32_t* rem) {
  for (uint32_t d = 0; d < 256; ++d) {
    if (*rem < hist[d]) return d;
    *rem -= hist[d];
  }
  return 255;
}
// the bin of a key among k thresholds in non-increasing order: how many of them are >= key (0 .. k)
DVD_HD int bin_of(const uint32_t* thr, int k, uint32_t key) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] >= key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

inline long pixels(int h, int w) { return (long)h * w; }
inline long error_blocks(long n) { return (n + kBlock * kPer - 1) / (kBlock * kPer); }
inline int strided_blocks(long n) {
  const long b = (n + kBlock - 1) / kBlock;
  return (int)(b < kGridCap ? b : kGridCap);
}

// ---- the workspace: byte offsets of its parts for a plane of n pixels (every part 256-byte aligned) ----------------------------
// The head (selection state, block histograms, block bins) has one size for every n: the selection and the bins need no more.
struct Layout {
  long state, hist, bins, partials, e, sigma, total;
};
inline long up256(long x) { return (x + 255) & ~255l; }
inline Layout layout(long n) {
  Layout l;
  l.state = 0;
  l.hist = up256(l.state + (long)sizeof(SelState));
  l.bins = up256(l.hist + (long)kGridCap * kMaxRanks * 256 * 4);
  l.partials = up256(l.bins + (long)kGridCap * (kMaxRanks + 1) * kBinWords * 8);
  l.e = up256(l.partials + error_blocks(n) * kPartial * 8);
  l.sigma = up256(l.e + 4 * n);
  l.total = up256(l.sigma + 4 * n);
  return l;
}

// ---- the argument checks of the entry points (no pointers), shared with the restatement ----------------------------------------
inline int check_size(int h, int w) { return h < 1 || w < 1 || h > kMaxSide || w > kMaxSide ? DVD_E_MAP_SHAPE : DVD_OK; }
inline int check_grid(int g) { return g < kMinGrid || g > kMaxGrid ? DVD_E_MAP_SHAPE : DVD_OK; }
inline int check_errors(int g, int gt_g, int n_hyp, int h, int w) {
  if (check_size(h, w) != DVD_OK || (g != 0 && check_grid(g) != DVD_OK) || (gt_g != 0 && check_grid(gt_g) != DVD_OK)) return DVD_E_MAP_SHAPE;
  return n_hyp < 1 || n_hyp > (g ? kMaxHyp : 1) ? DVD_E_MAP_SHAPE : DVD_OK;      // g = 0, a field: no hypotheses
}
inline int check_plane(long n) { return n < 1 || n > (long)kMaxSide * kMaxSide ? DVD_E_MAP_SHAPE : DVD_OK; }
// k ranks 1 .. 50, non-decreasing, each below n
inline int check_ranks(const uint32_t* ranks, int k, long n) {
  if (k < 1 || k > kMaxRanks || !ranks) return DVD_E_MAP_RANKS;
  for (int i = 0; i < k; ++i)
    if ((long)ranks[i] >= n || (i && ranks[i] < ranks[i - 1])) return DVD_E_MAP_RANKS;
  return DVD_OK;
}

}  // namespace ms
}  // namespace dvd
