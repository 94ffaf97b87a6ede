// Synthetic documents: a flat scan drawn on the photograph through the forward field of
// dvd_map_invert.  The arithmetic is synth_core.h's; tests/synth_model.py restates it.
//   render_kernel<kDwords>   a workgroup owns a tile of 64 x 16 photograph pixels.  It turns the tile's fwd values and their
//                            one-pixel halo into Q8 scan positions in LDS once (66 x 18 x 8 bytes); then a lane draws four
//                            neighbouring pixels of a row - footprint, filter, shading, edge blend, all from the LDS tile - and
//                            stores their twelve bytes as three dwords (kDwords: w is a multiple of 4, so every row begins on a
//                            dword and no group straddles the image's edge) or byte by byte.  The filter's branch is per pixel:
//                            in a wave whose lanes all have radii 1 x 1 no lane enters the general tent loop.
//   footprint_kernel         the same tile; the radii as two bytes per pixel
// No atomics, no scratch memory; which kernel runs depends on w alone.
#include "common.h"
#include "synth_core.h"

namespace dvd {
namespace sy {

struct Args {
  const uint8_t* scan;
  const float* fwd;
  const uint8_t* bg;
  uint8_t* out;
  int hs, ws, h, w;
  float kx, ky;
  uint32_t bg_color;
  int shade_on;
  Params prm;
};

// a pixel's neighbourhood in the LDS tile
struct TileAt {
  const Pos* at0;
  __device__ __forceinline__ Pos operator()(int dy, int dx) const { return at0[dy * kHaloW + dx]; }
};

struct Dwords3 {
  uint32_t a, b, c;
};

// the Q8 positions of the tile at (x0, y0) and of its halo; off the image: uncovered
__device__ __forceinline__ void stage_tile(const float* __restrict__ fwd, int h, int w, int hs, int ws, float kx, float ky, int x0, int y0,
                                           Pos* __restrict__ tile) {
  for (int i = threadIdx.x; i < kHaloW * kHaloH; i += kBlock) {
    const int ty = i / kHaloW, tx = i - ty * kHaloW;
    const int y = y0 - 1 + ty, x = x0 - 1 + tx;
    Pos p;
    p.x = kUncovered;
    p.y = 0;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const float2 uv = reinterpret_cast<const float2*>(fwd)[(size_t)y * w + x];
      p = pos_of(uv.x, uv.y, kx, ky, hs, ws);
    }
    tile[i] = p;
  }
  __syncthreads();
}

template <bool kDwords>
__global__ __launch_bounds__(kBlock) void render_kernel(Args a) {
  __shared__ Pos tile[kHaloW * kHaloH];
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  stage_tile(a.fwd, a.h, a.w, a.hs, a.ws, a.kx, a.ky, x0, y0, tile);
  const int ly = threadIdx.x / (kTileW / kPer), lx = (threadIdx.x % (kTileW / kPer)) * kPer;
  const int y = y0 + ly, xa = x0 + lx;
  if (y >= a.h || xa >= a.w) return;
  uint32_t bytes[3 * kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int x = xa + k;
    uint32_t rgb[3] = {0, 0, 0};
    if (kDwords || x < a.w) {
      const size_t p = (size_t)y * a.w + x;
      uint32_t bg[3] = {a.bg_color & 255, (a.bg_color >> 8) & 255, (a.bg_color >> 16) & 255};
      if (a.bg) {
        bg[0] = a.bg[3 * p];
        bg[1] = a.bg[3 * p + 1];
        bg[2] = a.bg[3 * p + 2];
      }
      TileAt at;
      at.at0 = tile + (ly + 1) * kHaloW + lx + k + 1;
      pixel_at(a.scan, a.hs, a.ws, at, x, y, a.h, a.w, bg, a.prm, a.shade_on != 0, rgb);
    }
    bytes[3 * k] = rgb[0];
    bytes[3 * k + 1] = rgb[1];
    bytes[3 * k + 2] = rgb[2];
  }
  uint8_t* dst = a.out + 3 * ((size_t)y * a.w + xa);
  if (kDwords) {
    Dwords3 d;
    d.a = bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24;
    d.b = bytes[4] | bytes[5] << 8 | bytes[6] << 16 | bytes[7] << 24;
    d.c = bytes[8] | bytes[9] << 8 | bytes[10] << 16 | bytes[11] << 24;
    *reinterpret_cast<Dwords3*>(dst) = d;              // w and xa are multiples of 4 and `out` is dword-aligned
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (xa + k < a.w) {
        dst[3 * k] = (uint8_t)bytes[3 * k];
        dst[3 * k + 1] = (uint8_t)bytes[3 * k + 1];
        dst[3 * k + 2] = (uint8_t)bytes[3 * k + 2];
      }
  }
}

__global__ __launch_bounds__(kBlock) void footprint_kernel(const float* __restrict__ fwd, int h, int w, int hs, int ws, float kx, float ky,
                                                           uint8_t* __restrict__ out) {
  __shared__ Pos tile[kHaloW * kHaloH];
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  stage_tile(fwd, h, w, hs, ws, kx, ky, x0, y0, tile);
  const int ly = threadIdx.x / (kTileW / kPer), lx = (threadIdx.x % (kTileW / kPer)) * kPer;
  const int y = y0 + ly;
  if (y >= h) return;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int x = x0 + lx + k;
    if (x >= w) continue;
    TileAt at;
    at.at0 = tile + (ly + 1) * kHaloW + lx + k + 1;
    uint8_t rx = 0, ry = 0;
    if (at(0, 0).x >= 0) {
      const Foot f = foot_at(at);
      rx = (uint8_t)f.rx;
      ry = (uint8_t)f.ry;
    }
    const size_t p = (size_t)y * w + x;
    out[2 * p] = rx;
    out[2 * p + 1] = ry;
  }
}

}  // namespace sy
}  // namespace dvd

using namespace dvd;

#define SYNTH_REQUIRE(cond, code, ...) \
  do {                                 \
    if (!(cond)) {                     \
      dvd::set_error(__VA_ARGS__);     \
      return code;                     \
    }                                  \
  } while (0)

#define SYNTH_CHECK_SIZE(name)                                                                                                       \
  SYNTH_REQUIRE(sy::check_size(hs, ws, h, w) == DVD_OK, DVD_E_SYNTH_SHAPE, name ": scan %d x %d, photograph %d x %d: sides 1..%d", hs, \
                ws, h, w, sy::kMaxSide)

static dim3 synth_grid(int h, int w) { return dim3((unsigned)((w + sy::kTileW - 1) / sy::kTileW), (unsigned)((h + sy::kTileH - 1) / sy::kTileH)); }

extern "C" int dvd_synth_render_rgb8(const uint8_t* scan, int hs, int ws, const float* fwd, int h, int w, const uint8_t* bg,
                                     uint32_t bg_color, const dvd_synth_params* params, uint8_t* out, void* stream) {
  SYNTH_CHECK_SIZE("synth_render_rgb8");
  DVD_REQUIRE(scan && fwd && params && out, "synth_render_rgb8: null pointer");
  SYNTH_REQUIRE(sy::check_params(*params) == DVD_OK, DVD_E_SYNTH_PARAM,
                "synth_render_rgb8: l0 = %g, lgx = %g, lgy = %g, k = %g, a_ref = %g: finite numbers, a_ref > 0 with shading on",
                (double)params->l0, (double)params->lgx, (double)params->lgy, (double)params->k, (double)params->a_ref);
  const bool dwords = w % 4 == 0;
  DVD_REQUIRE(((uintptr_t)fwd & 7) == 0 && (!dwords || ((uintptr_t)out & 3) == 0), "synth_render_rgb8: misaligned pointer");
  DVD_REQUIRE(out != scan && out != bg, "synth_render_rgb8: out must not be scan or bg");
  sy::Args a;
  a.scan = scan;
  a.fwd = fwd;
  a.bg = bg;
  a.out = out;
  a.hs = hs;
  a.ws = ws;
  a.h = h;
  a.w = w;
  a.kx = sy::axis_scale(ws, w);
  a.ky = sy::axis_scale(hs, h);
  a.bg_color = bg_color;
  a.shade_on = sy::shading_on(*params) ? 1 : 0;
  a.prm = *params;
  if (dwords)
    sy::render_kernel<true><<<synth_grid(h, w), sy::kBlock, 0, (hipStream_t)stream>>>(a);
  else
    sy::render_kernel<false><<<synth_grid(h, w), sy::kBlock, 0, (hipStream_t)stream>>>(a);
  return check_launch("synth_render_rgb8");
}

extern "C" int dvd_synth_footprint(const float* fwd, int h, int w, int hs, int ws, uint8_t* out, void* stream) {
  SYNTH_CHECK_SIZE("synth_footprint");
  DVD_REQUIRE(fwd && out, "synth_footprint: null pointer");
  DVD_REQUIRE(((uintptr_t)fwd & 7) == 0, "synth_footprint: misaligned pointer");
  sy::footprint_kernel<<<synth_grid(h, w), sy::kBlock, 0, (hipStream_t)stream>>>(fwd, h, w, hs, ws, sy::axis_scale(ws, w), sy::axis_scale(hs, h),
                                                                                 out);
  return check_launch("synth_footprint");
}
