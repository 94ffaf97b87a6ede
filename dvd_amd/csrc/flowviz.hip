// Flow pictures and the .flo payload of a predicted map.  The arithmetic is flowviz_core.h's;
// tests/flowviz_model.py restates it byte for byte.
//   flow_rgb8_kernel<Src>         [n,h,w,3] u8 colour-wheel picture of a displacement field.  One lane per group of four pixels of
//                                 the batch's flat pixel index: twelve bytes, stored as three whole dwords; the last, short group
//                                 stores bytes.  Src = FieldSrc reads the field [n,h,w,2] f32 (dvd_flow_to_image_rgb8), Src =
//                                 CoarseSrc computes it from the coarse map [n,2,g,g] (dvd_flow_picture_rgb8: nothing but the
//                                 picture is written) - one pixel function, pixel_rgb, for both.
//   flow_radius_partials<Src>     norm 'max': the largest radius of each image.  Lane maxima over kRadPer pixels, block_ops.h's
//   flow_radius_finalize          wave_max, the four waves in order; then one workgroup per image over the block partials.  No
//                                 atomics; the order is fixed (and a maximum without NaN does not depend on it).
//   flow_full_uv_kernel           [n,h,w,2] f32 pixel displacement of a coarse map, one pixel (8 bytes) per lane.
// Every kernel is pointwise; none uses scratch memory, none uses LDS beyond the reduction's few floats.  Every shape takes the
// same kernels.
#include "block_ops.h"
#include "common.h"
#include "flowviz_core.h"

namespace dvd {
namespace fv {

struct FieldSrc {
  static constexpr bool kNeedsRowCol = false;
  const float* field;        // [n,h,w,2]
  size_t hw;
  __device__ __forceinline__ void at(uint32_t img, uint32_t pix, int, int, float* u, float* v) const {
    const float2 d = *reinterpret_cast<const float2*>(field + 2 * ((size_t)img * hw + pix));
    *u = d.x;
    *v = d.y;
  }
};

struct CoarseSrc {
  static constexpr bool kNeedsRowCol = true;
  const float* flow;         // [n,2,g,g]
  Up up;
  __device__ __forceinline__ void at(uint32_t img, uint32_t, int i, int j, float* u, float* v) const {
    full_uv_at(flow + (size_t)img * 2 * up.g * up.g, up, i, j, u, v);
  }
};

struct alignas(4) Dwords3 {
  uint32_t a, b, c;
};

__device__ __forceinline__ size_t flat_block() { return (size_t)blockIdx.y * gridDim.x + blockIdx.x; }

template <typename Src>
__global__ __launch_bounds__(kBlock) void flow_rgb8_kernel(Src src, size_t total, uint32_t hw, uint32_t w, float diag_rm,
                                                           const float* __restrict__ largest, float clip, int bgr,
                                                           uint8_t* __restrict__ out) {
  const size_t p0 = (flat_block() * kBlock + threadIdx.x) * kGroup;
  if (p0 >= total) return;
  uint32_t img = (uint32_t)(p0 / hw);
  uint32_t pix = (uint32_t)(p0 - (size_t)img * hw);
  uint32_t i = pix / w, j = pix - i * w;
  const int live = total - p0 < kGroup ? (int)(total - p0) : kGroup;
  uint32_t bytes[3 * kGroup];
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    int rgb[3] = {0, 0, 0};
    if (k < live) {
      float u, v;
      src.at(img, pix, (int)i, (int)j, &u, &v);
      pixel_rgb(u, v, largest ? max_rad_max(largest[img]) : diag_rm, clip, rgb);
    }
    bytes[3 * k] = (uint32_t)(bgr ? rgb[2] : rgb[0]);
    bytes[3 * k + 1] = (uint32_t)rgb[1];
    bytes[3 * k + 2] = (uint32_t)(bgr ? rgb[0] : rgb[2]);
    ++pix;
    if (++j == w) {
      j = 0;
      ++i;
    }
    if (pix == hw) {
      pix = 0;
      i = 0;
      ++img;
    }
  }
  uint8_t* dst = out + 3 * p0;
  if (live == kGroup) {
    Dwords3 d;
    d.a = bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24;
    d.b = bytes[4] | bytes[5] << 8 | bytes[6] << 16 | bytes[7] << 24;
    d.c = bytes[8] | bytes[9] << 8 | bytes[10] << 16 | bytes[11] << 24;
    *reinterpret_cast<Dwords3*>(dst) = d;            // 3 p0 is a multiple of 12 and `out` is dword-aligned
  } else {
#pragma unroll
    for (int b = 0; b < 3 * (kGroup - 1); ++b)
      if (b < 3 * live) dst[b] = (uint8_t)bytes[b];
  }
}

// grid (blocks of an image, images); partials [n][blocks]
template <typename Src>
__global__ __launch_bounds__(kBlock) void flow_radius_partials_kernel(Src src, uint32_t hw, uint32_t w, float clip,
                                                                      float* __restrict__ partials) {
  __shared__ float red[kBlock / 64];
  float m = 0.f;
#pragma unroll 4
  for (int k = 0; k < kRadPer; ++k) {
    const uint32_t pix = (blockIdx.x * kRadPer + k) * kBlock + threadIdx.x;      // below 2^28 + 4096
    if (pix < hw) {
      uint32_t i = 0, j = 0;
      if (Src::kNeedsRowCol) {
        i = pix / w;
        j = pix - i * w;
      }
      float u, v;
      src.at(blockIdx.y, pix, (int)i, (int)j, &u, &v);
      const float r = radius_of(u, v, clip);
      m = r > m ? r : m;
    }
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
    for (int q = 1; q < kBlock / 64; ++q) t = red[q] > t ? red[q] : t;
    partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// one workgroup per image: lane t takes partials t, t + 256, ... in order, then a tree over the 256 lanes
__global__ __launch_bounds__(kBlock) void flow_radius_finalize_kernel(const float* __restrict__ partials, int blocks,
                                                                      float* __restrict__ out) {
  __shared__ float red[kBlock];
  const int tid = threadIdx.x;
  const float* mine = partials + (size_t)blockIdx.x * blocks;
  float v = 0.f;
  for (int t = tid; t < blocks; t += kBlock) v = mine[t] > v ? mine[t] : v;
  red[tid] = v;
  __syncthreads();
  for (int s = kBlock / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kBlock) void flow_full_uv_kernel(const float* __restrict__ flow, Up up, size_t total, uint32_t hw,
                                                              float* __restrict__ out) {
  const size_t p = flat_block() * kBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t img = (uint32_t)(p / hw);
  const uint32_t pix = (uint32_t)(p - (size_t)img * hw);
  const uint32_t i = pix / (uint32_t)up.w, j = pix - i * (uint32_t)up.w;
  float u, v;
  full_uv_at(flow + (size_t)img * 2 * up.g * up.g, up, (int)i, (int)j, &u, &v);
  *reinterpret_cast<float2*>(out + 2 * p) = make_float2(u, v);
}

// a flat launch of `blocks` workgroups: x up to 2^23, the rest in y (flat_block)
static dim3 flat_grid(long blocks) {
  const long gx = blocks < (1l << 23) ? blocks : (1l << 23);
  return dim3((unsigned)gx, (unsigned)((blocks + gx - 1) / gx));
}

template <typename Src>
static void launch_radius(const Src& src, int n, int h, int w, float clip, float* out, float* partials, hipStream_t s) {
  const int blocks = (int)radius_blocks(h, w);
  flow_radius_partials_kernel<Src><<<dim3(blocks, n), kBlock, 0, s>>>(src, (uint32_t)h * w, (uint32_t)w, clip, partials);
  flow_radius_finalize_kernel<<<n, kBlock, 0, s>>>(partials, blocks, out);
}

template <typename Src>
static void launch_rgb8(const Src& src, int n, int h, int w, const float* largest, float clip, int bgr, uint8_t* out, hipStream_t s) {
  const size_t total = (size_t)n * h * w;
  const long blocks = (long)((total + (size_t)kBlock * kGroup - 1) / ((size_t)kBlock * kGroup));
  flow_rgb8_kernel<Src><<<flat_grid(blocks), kBlock, 0, s>>>(src, total, (uint32_t)h * w, (uint32_t)w, diag_rad_max(h, w), largest, clip,
                                                             bgr, out);
}

}  // namespace fv
}  // namespace dvd

using namespace dvd;

#define FLOW_REQUIRE_SHAPE(what, n, h, w)                                                                                  \
  do {                                                                                                                     \
    if (fv::check_shape(n, h, w) != DVD_OK) {                                                                              \
      set_error(what ": n = %d, h = %d, w = %d: n 0..%d, sides 1..%d", n, h, w, fv::kMaxImages, fv::kMaxSide);           \
      return DVD_E_FLOW_SHAPE;                                                                                             \
    }                                                                                                                      \
  } while (0)
#define FLOW_REQUIRE_GRID(what, g)                                                          \
  do {                                                                                      \
    if (fv::check_grid(g) != DVD_OK) {                                                      \
      set_error(what ": g = %d: g %d..%d", g, fv::kMinGrid, fv::kMaxGrid);                  \
      return DVD_E_FLOW_SHAPE;                                                              \
    }                                                                                       \
  } while (0)

extern "C" long dvd_flow_workspace_bytes(int n, int h, int w) {
  if (fv::check_shape(n, h, w) != DVD_OK) {
    set_error("flow_workspace_bytes: n = %d, h = %d, w = %d: n 0..%d, sides 1..%d", n, h, w, fv::kMaxImages, fv::kMaxSide);
    return DVD_E_FLOW_SHAPE;
  }
  return (long)n * fv::radius_blocks(h, w) * (long)sizeof(float);
}

extern "C" int dvd_flow_radius_max(const float* field, int n, int h, int w, float clip, float* out, void* ws, void* stream) {
  FLOW_REQUIRE_SHAPE("flow_radius_max", n, h, w);
  DVD_REQUIRE(fv::check_clip(clip) == DVD_OK, "flow_radius_max: clip is NaN");
  if (n == 0) return DVD_OK;
  DVD_REQUIRE(field && out && ws, "flow_radius_max: null pointer");
  DVD_REQUIRE(((uintptr_t)field & 7) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)ws & 3) == 0, "flow_radius_max: misaligned pointer");
  fv::launch_radius(fv::FieldSrc{field, (size_t)h * w}, n, h, w, clip, out, (float*)ws, (hipStream_t)stream);
  return check_launch("flow_radius_max");
}

extern "C" int dvd_flow_to_image_rgb8(const float* field, int n, int h, int w, int norm, float clip, int bgr, uint8_t* out,
                                      float* largest, void* ws, void* stream) {
  FLOW_REQUIRE_SHAPE("flow_to_image_rgb8", n, h, w);
  DVD_REQUIRE(fv::check_norm(norm) == DVD_OK, "flow_to_image_rgb8: norm = %d: DVD_FLOW_NORM_DIAG or DVD_FLOW_NORM_MAX", norm);
  DVD_REQUIRE(fv::check_clip(clip) == DVD_OK, "flow_to_image_rgb8: clip is NaN");
  if (n == 0) return DVD_OK;
  const bool by_max = norm == DVD_FLOW_NORM_MAX;
  DVD_REQUIRE(field && out && (!by_max || (largest && ws)), "flow_to_image_rgb8: null pointer");
  DVD_REQUIRE(((uintptr_t)field & 7) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)largest & 3) == 0 && ((uintptr_t)ws & 3) == 0,
              "flow_to_image_rgb8: misaligned pointer");
  const fv::FieldSrc src{field, (size_t)h * w};
  hipStream_t s = (hipStream_t)stream;
  if (by_max) fv::launch_radius(src, n, h, w, clip, largest, (float*)ws, s);
  fv::launch_rgb8(src, n, h, w, by_max ? largest : nullptr, clip, bgr != 0, out, s);
  return check_launch("flow_to_image_rgb8");
}

extern "C" int dvd_flow_full_uv(const float* flow, int n, int g, int h, int w, float* out, void* stream) {
  FLOW_REQUIRE_SHAPE("flow_full_uv", n, h, w);
  FLOW_REQUIRE_GRID("flow_full_uv", g);
  if (n == 0) return DVD_OK;
  DVD_REQUIRE(flow && out, "flow_full_uv: null pointer");
  DVD_REQUIRE(((uintptr_t)flow & 3) == 0 && ((uintptr_t)out & 7) == 0, "flow_full_uv: misaligned pointer");
  const size_t total = (size_t)n * h * w;
  const long blocks = (long)((total + fv::kBlock - 1) / fv::kBlock);
  fv::flow_full_uv_kernel<<<fv::flat_grid(blocks), fv::kBlock, 0, (hipStream_t)stream>>>(flow, fv::make_up(g, h, w), total, (uint32_t)h * w, out);
  return check_launch("flow_full_uv");
}

extern "C" int dvd_flow_picture_rgb8(const float* flow, int n, int g, int h, int w, int norm, int bgr, uint8_t* out, float* largest,
                                     void* ws, void* stream) {
  FLOW_REQUIRE_SHAPE("flow_picture_rgb8", n, h, w);
  FLOW_REQUIRE_GRID("flow_picture_rgb8", g);
  DVD_REQUIRE(fv::check_norm(norm) == DVD_OK, "flow_picture_rgb8: norm = %d: DVD_FLOW_NORM_DIAG or DVD_FLOW_NORM_MAX", norm);
  if (n == 0) return DVD_OK;
  const bool by_max = norm == DVD_FLOW_NORM_MAX;
  DVD_REQUIRE(flow && out && (!by_max || (largest && ws)), "flow_picture_rgb8: null pointer");
  DVD_REQUIRE(((uintptr_t)flow & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)largest & 3) == 0 && ((uintptr_t)ws & 3) == 0,
              "flow_picture_rgb8: misaligned pointer");
  const fv::CoarseSrc src{flow, fv::make_up(g, h, w)};
  hipStream_t s = (hipStream_t)stream;
  if (by_max) fv::launch_radius(src, n, h, w, -1.f, largest, (float*)ws, s);
  fv::launch_rgb8(src, n, h, w, by_max ? largest : nullptr, -1.f, bgr != 0, out, s);
  return check_launch("flow_picture_rgb8");
}
