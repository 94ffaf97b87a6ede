// The arithmetic of the flow pictures, shared by the kernels of flowviz.hip and by the stand-alone CPU
// restatement flowviz_host_check.cpp (plain C++, no HIP).  tests/flowviz_model.py is its NumPy statement and the definition.
// The colour wheel is integers; everything else is f32 with every operation rounded on its own (noise_core.h's fmul, fadd, fsub,
// fdiv, fsqrt) - the angle is written out here, no library atan2 - and the up-sampling is interp_core.h's, whose only fused
// operations are explicit fmaf calls: NumPy float32 gives the same bits as the kernel.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dvd_hip.h"

#include "hd.h"
#include "interp_core.h"
#include "noise_core.h"

namespace dvd {
namespace fv {

using nz::bits_of;
using nz::fadd;
using nz::fdiv;
using nz::fmul;
using nz::fsqrt;
using nz::fsub;

constexpr int kMaxSide = 16384, kMaxImages = 65535;
constexpr int kMinGrid = 2, kMaxGrid = 8192;          // g of the coarse map [.,2,g,g]
constexpr int kGroup = 4;                             // pixels per lane of the picture kernels: 12 bytes, three whole dwords
constexpr int kBlock = 256;
constexpr int kRadPer = 16;                           // radius maximum: pixels per lane (stride kBlock inside a workgroup's run)
constexpr int kWheel = 55;                            // RY 15, YG 6, GC 4, CB 11, BM 13, MR 6
constexpr float kEps = 1e-5f;

// ---- the Middlebury colour wheel (Baker et al., ICCV 2007), entry k = 0 .. 54 ------------------------------------------------
// Six segments between the primaries; inside one a channel ramps by floor(255 i / n) while the other two stay at 0 or 255.
DVD_HD void wheel(int k, int* rgb) {
  int r, g, b;
  if (k < 15) {                       // red -> yellow
    r = 255; g = 255 * k / 15; b = 0;
  } else if (k < 21) {                // yellow -> green
    r = 255 - 255 * (k - 15) / 6; g = 255; b = 0;
  } else if (k < 25) {                // green -> cyan
    r = 0; g = 255; b = 255 * (k - 21) / 4;
  } else if (k < 36) {                // cyan -> blue
    r = 0; g = 255 - 255 * (k - 25) / 11; b = 255;
  } else if (k < 49) {                // blue -> magenta
    r = 255 * (k - 36) / 13; g = 0; b = 255;
  } else {                            // magenta -> red
    r = 255; g = 0; b = 255 - 255 * (k - 49) / 6;
  }
  rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// ---- atan2(y, x) / pi in [-1, 1] ----------------------------------------------------------------------------------------------
// q = min(|x|, |y|) / max(|x|, |y|) in [0, 1] (0 for x = y = 0).  Above sqrt 2 - 1 the argument is reduced by
// atan q = pi/4 + atan((q - 1) / (q + 1)), so |r| <= sqrt 2 - 1 and atan(r) / pi = r P(r^2), P of degree 5 (a least-squares fit
// on Chebyshev nodes; its error is below 6e-9, less than half an ulp of 1/4).  The octant, the sign bit of x and the sign bit
// of y then place it: the axes and the diagonals give k / 4 exactly, and a signed zero counts as numpy's arctan2 counts it.
DVD_HD float turn_of(float y, float x) {
  const float ay = fabsf(y), ax = fabsf(x);
  const float mn = ay < ax ? ay : ax, mx = ay < ax ? ax : ay;
  const float q = mx == 0.f ? 0.f : (mn == mx ? 1.f : fdiv(mn, mx));       // mn == mx: also inf / inf
  const bool upper = q > 0.41421357f;
  const float r = upper ? fdiv(fsub(q, 1.f), fadd(q, 1.f)) : q;
  const float z = fmul(r, r);
  float p = -0.019203662872314453f;
  p = fadd(fmul(p, z), 0.03365402668714523f);
  p = fadd(fmul(p, z), -0.045327235013246536f);
  p = fadd(fmul(p, z), 0.0636562779545784f);
  p = fadd(fmul(p, z), -0.10610321164131165f);
  p = fadd(fmul(p, z), 0.31830987334251404f);
  float t = fmul(r, p);
  if (upper) t = fadd(0.25f, t);
  if (ay > ax) t = fsub(0.5f, t);
  if (bits_of(x) >> 31) t = fsub(1.f, t);
  return (bits_of(y) >> 31) ? -t : t;
}

DVD_HD bool finite2(float u, float v) { return ((bits_of(u) & 0x7f800000u) != 0x7f800000u) && ((bits_of(v) & 0x7f800000u) != 0x7f800000u); }

// the reference's clip_flow: np.clip(flow, 0, clip) - negative components become 0.  clip < 0: no clip.
DVD_HD float clipped(float x, float clip) { return clip < 0.f ? x : (x < 0.f ? 0.f : (x > clip ? clip : x)); }

// sqrt(u^2 + v^2) of a clipped pixel; -1 for a pixel with a non-finite component (it takes no part in the maximum)
DVD_HD float radius_of(float u, float v, float clip) {
  if (!finite2(u, v)) return -1.f;
  u = clipped(u, clip);
  v = clipped(v, clip);
  return fsqrt(fadd(fmul(u, u), fmul(v, v)));
}

// rad_max of norm 'diag' (the reference's) and of norm 'max' from the largest radius of the image
inline float diag_rad_max(int h, int w) {
  const long hh = h / 2, ww = w / 2;
  return fadd(fsqrt((float)(ww * ww + hh * hh)), kEps);
}
DVD_HD float max_rad_max(float largest) { return fadd(largest, kEps); }

// One channel: the blend g c0 + f c1 of two wheel entries over 255, pulled towards white inside the unit radius and dimmed
// outside it, then floor(255 col).
DVD_HD int channel_byte(float g, float f, int c0, int c1, float rad) {
  float col = fdiv(fadd(fmul(g, (float)c0), fmul(f, (float)c1)), 255.f);
  col = rad <= 1.f ? fsub(1.f, fmul(rad, fsub(1.f, col))) : fmul(col, 0.75f);
  const int byte = (int)fmul(255.f, col);
  return byte < 0 ? 0 : (byte > 255 ? 255 : byte);
}

// One pixel: displacement (u, v) in pixels -> rgb bytes.  rad_max: diag_rad_max or max_rad_max.
DVD_HD void pixel_rgb(float u, float v, float rad_max, float clip, int* rgb) {
  if (!finite2(u, v)) {
    rgb[0] = rgb[1] = rgb[2] = 0;
    return;
  }
  u = clipped(u, clip);
  v = clipped(v, clip);
  const float rad = fdiv(fsqrt(fadd(fmul(u, u), fmul(v, v))), rad_max);
  const float a = turn_of(-v, -u);
  const float fk = fmul(fmul(fadd(a, 1.f), 0.5f), (float)(kWheel - 1));
  int k0 = (int)fk;                                   // 0 .. 54
  k0 = k0 > kWheel - 1 ? kWheel - 1 : k0;
  const int k1 = k0 + 1 == kWheel ? 0 : k0 + 1;
  const float f = fsub(fk, (float)k0), g = fsub(1.f, f);
  int c0[3], c1[3];
  wheel(k0, c0);
  wheel(k1, c1);
  rgb[0] = channel_byte(g, f, c0[0], c1[0], rad);
  rgb[1] = channel_byte(g, f, c0[1], c1[1], rad);
  rgb[2] = channel_byte(g, f, c0[2], c1[2], rad);
}

// ---- the full-resolution displacement of a coarse map -------------------------------------------------------------------------
// s = F.interpolate(flow [2,g,g] -> h x w, bilinear, align_corners=True) by interp_core.h, as the unwarp tail does it;
// u = s_x (w - 1), v = s_y (h - 1).
struct Up {
  int g, h, w, small;
  float sy, sx;       // (g-1)/(h-1), (g-1)/(w-1)
  float hm1, wm1;     // h - 1, w - 1
};
inline Up make_up(int g, int h, int w) {
  Up p;
  p.g = g;
  p.h = h;
  p.w = w;
  p.small = (h + w <= 128) ? 1 : 0;
  p.sy = interp_scale(g, h);
  p.sx = interp_scale(g, w);
  p.hm1 = (float)(h - 1);
  p.wm1 = (float)(w - 1);
  return p;
}
DVD_HD void full_uv_at(const float* flow, const Up& p, int i, int j, float* u, float* v) {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  interp_axis(p.sy, i, p.g, y0, y1, ly0, ly1);
  interp_axis(p.sx, j, p.g, x0, x1, lx0, lx1);
  const float* fx = flow;
  const float* fy = flow + p.g * p.g;
  const int a = y0 * p.g + x0, b = y0 * p.g + x1, c = y1 * p.g + x0, d = y1 * p.g + x1;
  *u = fmul(interp_sum(fx[a], fx[b], fx[c], fx[d], lx0, lx1, ly0, ly1, p.small), p.wm1);
  *v = fmul(interp_sum(fy[a], fy[b], fy[c], fy[d], lx0, lx1, ly0, ly1, p.small), p.hm1);
}

inline long radius_blocks(int h, int w) { return ((long)h * w + kBlock * kRadPer - 1) / (kBlock * kRadPer); }

// ---- the argument checks of the entry points (no pointers), shared with the restatement -----------------------------------------
inline int check_shape(int n, int h, int w) {
  return n < 0 || n > kMaxImages || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide ? DVD_E_FLOW_SHAPE : DVD_OK;
}
inline int check_grid(int g) { return g < kMinGrid || g > kMaxGrid ? DVD_E_FLOW_SHAPE : DVD_OK; }
inline int check_norm(int norm) { return norm == DVD_FLOW_NORM_DIAG || norm == DVD_FLOW_NORM_MAX ? DVD_OK : DVD_E_ARG; }
// clip: negative = none; NaN is refused
inline int check_clip(float clip) { return clip == clip ? DVD_OK : DVD_E_ARG; }

}  // namespace fv
}  // namespace dvd
