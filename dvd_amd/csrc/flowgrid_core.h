// The sampling grid of the unwarp tail at one page pixel: where on the photograph the tail samples for page pixel (i, j).
// Shared by the unwarp kernels (warp.hip), by the map inverse (mapinv.hip) and by the stand-alone CPU restatement
// mapinv_host_check.cpp (plain C++, no HIP).  The up-sampling is interp_core.h's; every other f32 operation is rounded on its
// own (noise_core.h's helpers), so the host gives the device's bits.
#pragma once
#include "hd.h"
#include "interp_core.h"
#include "noise_core.h"

namespace dvd {

struct UpParams {
  int g, h, w;
  float sy, sx;     // (g-1)/(h-1), (g-1)/(w-1): ATen area_pixel_compute_scale, align_corners=True
  float sby, sbx;   // 511/(h-1), 511/(w-1): the same for the 512 x 512 base grid (train_settings/dvd/evaluation.py:304)
  float scale;
  int small;        // h + w <= 128: torch's CPU dispatch takes its channels-last kernel, whose sum has another order (below)
};

inline UpParams make_up(int g, int h, int w, float scale) {
  UpParams p;
  p.g = g;
  p.h = h;
  p.w = w;
  p.sy = h > 1 ? (float)(g - 1) / (float)(h - 1) : 0.f;
  p.sx = w > 1 ? (float)(g - 1) / (float)(w - 1) : 0.f;
  p.sby = h > 1 ? 511.f / (float)(h - 1) : 0.f;
  p.sbx = w > 1 ? 511.f / (float)(w - 1) : 0.f;
  p.scale = scale;
  p.small = (h + w <= 128) ? 1 : 0;
  return p;
}

// interp_axis and interp_sum, one axis of F.interpolate(bilinear, align_corners=True) and its four-value sum in the order of
// ATen's CPU kernels, are interp_core.h's: the flow pictures (flowviz.hip) upsample the same map with the same arithmetic.

// The per-AXIS terms of one output coordinate: the flow's and the 512-grid base's source indices and lambdas, and the base
// grid's two values k / 511 (an IEEE division each).  They depend on the column (or the row) alone, so a kernel that walks
// down a column block computes its x terms ONCE (unwarp_u8_band_kernel); flow_grid_at composes them per pixel.
struct AxisTerm {
  int f0, f1;            // flow rows / columns
  float l0, l1;          // ... and their lambdas
  float bl0, bl1;        // lambdas of the 512-grid base
  float c0, c1;          // its two values: index / 511
};
DVD_HD AxisTerm axis_term(float scale, float bscale, int dst, int g) {
  AxisTerm t;
  interp_axis(scale, dst, g, t.f0, t.f1, t.l0, t.l1);
  int b0, b1;
  interp_axis(bscale, dst, 512, b0, b1, t.bl0, t.bl1);
  t.c0 = nz::fdiv((float)b0, 511.f);
  t.c1 = nz::fdiv((float)b1, 511.f);
  return t;
}
DVD_HD void flow_grid_from(const float* __restrict__ flow, const UpParams& p, const AxisTerm& y, const AxisTerm& x, float& gx,
                           float& gy) {
  // sample = F.interpolate(flow, (H, W), bilinear, align_corners=True)                       (evaluation.py:301)
  const int gg = p.g * p.g;
  float v[2];
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const float* f = flow + ch * gg;
    v[ch] = interp_sum(f[y.f0 * p.g + x.f0], f[y.f0 * p.g + x.f1], f[y.f1 * p.g + x.f0], f[y.f1 * p.g + x.f1], x.l0, x.l1, y.l0,
                       y.l1, p.small);
  }
  // base = F.interpolate(coords_grid_tensor((512, 512)) / 511., (H, W), bilinear, align_corners=True)   (evaluation.py:304):
  // channel 0 holds column / 511, channel 1 row / 511 of the 512 x 512 grid - interpolated like any other image, so the
  // value is NOT j / (W - 1) to the last bit
  const float bx = interp_sum(x.c0, x.c1, x.c0, x.c1, x.bl0, x.bl1, y.bl0, y.bl1, p.small);
  const float by = interp_sum(y.c0, y.c0, y.c1, y.c1, x.bl0, x.bl1, y.bl0, y.bl1, p.small);
  // sample = (((sample + base) * 1) * 2 - 1) * 0.987                                         (evaluation.py:306)
  gx = nz::fmul(nz::fsub(nz::fmul(nz::fmul(nz::fadd(v[0], bx), 1.f), 2.f), 1.f), p.scale);
  gy = nz::fmul(nz::fsub(nz::fmul(nz::fmul(nz::fadd(v[1], by), 1.f), 2.f), 1.f), p.scale);
}
DVD_HD void flow_grid_at(const float* __restrict__ flow, const UpParams& p, int i, int j, float& gx, float& gy) {
  flow_grid_from(flow, p, axis_term(p.sy, p.sby, i, p.g), axis_term(p.sx, p.sbx, j, p.g), gx, gy);
}

}  // namespace dvd
