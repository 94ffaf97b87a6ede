// F.interpolate(bilinear, align_corners=True) of the coarse flow as ATen's CPU kernels compute it: the per-axis source index and
// lambdas and the four-value sum.  Shared by the unwarp tail (warp.hip), by the flow pictures (flowviz.hip) and by the stand-alone
// CPU restatement flowviz_host_check.cpp (plain C++, no HIP); oracle/aten_order.py and tests/flowviz_model.py restate it.
#pragma once
#include <math.h>

#include "hd.h"

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")     // the host restatement: only the fmaf calls below are fused
#endif

namespace dvd {

DVD_HD float interp_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}
DVD_HD float interp_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(a, b);
#else
  return a - b;
#endif
}

// (g-1)/(n-1): ATen area_pixel_compute_scale, align_corners=True
inline float interp_scale(int g, int n) { return n > 1 ? (float)(g - 1) / (float)(n - 1) : 0.f; }

// One axis of F.interpolate(bilinear, align_corners=True) as ATen's CPU kernel computes it (UpSampleKernel.cpp,
// compute_source_index_and_lambda): src = scale * dst; i0 = min(floor(src), in - 1); l1 = clamp(src - i0, 0, 1); l0 = 1 - l1.
DVD_HD void interp_axis(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
  const float s = interp_mul(scale, (float)dst);
#if defined(__HIP_DEVICE_COMPILE__)
  i0 = min((int)s, in - 1);
  i1 = min(i0 + 1, in - 1);
#else
  const int f = (int)s;
  i0 = f < in - 1 ? f : in - 1;
  i1 = i0 + 1 < in - 1 ? i0 + 1 : in - 1;
#endif
  l1 = fminf(fmaxf(interp_sub(s, (float)i0), 0.f), 1.f);
  l0 = interp_sub(1.f, l1);
}
// ... and its four-value sum.  torch picks one of two CPU kernels by the OUTPUT size (UpSampleKernel.cpp,
// _use_vectorized_kernel_cond_2d; both orders found by bit-exact probing, oracle/aten_order.py restates them):
//   h + w > 128   separable: t = fma(left, lx0, right * lx1) per row, then fma(t_upper, ly0, t_lower * ly1)
//   h + w <= 128  channels-last kernel: weights w_rc = l_y(r) * l_x(c), sum fma(d, w11, fma(c, w10, fma(a, w00, b * w01)))
DVD_HD float interp_sum(float a, float b, float c, float d, float lx0, float lx1, float ly0, float ly1, int small) {
  if (small) {
    const float w00 = interp_mul(ly0, lx0), w01 = interp_mul(ly0, lx1), w10 = interp_mul(ly1, lx0), w11 = interp_mul(ly1, lx1);
    return fmaf(d, w11, fmaf(c, w10, fmaf(a, w00, interp_mul(b, w01))));
  }
  const float t0 = fmaf(a, lx0, interp_mul(b, lx1)), t1 = fmaf(c, lx0, interp_mul(d, lx1));
  return fmaf(t0, ly0, interp_mul(t1, ly1));
}

}  // namespace dvd
