// Pages at a chosen size: the photograph unwarped to a page of any size, filtered by the footprint the
// page's own sampling grid gives.  The arithmetic is sized_core.h's; tests/sized_model.py restates it.
//   sized_unwarp_kernel         a workgroup owns a tile of 64 x 16 page pixels.  The axis terms of the tile's 66 columns and 18
//                               rows (flowgrid_core.h: source indices, lambdas and the two divisions by 511) are computed once
//                               each into LDS; from them the Q8 positions of the tile and of its one-pixel halo, once each
//                               (66 x 18 x 8 bytes).  Then a lane draws four neighbouring pixels of a row - footprint from the
//                               LDS tile, taps gathered from global memory - and stores their twelve bytes as three dwords where
//                               they begin on one, and otherwise as two dwords between 4 single bytes (a row begins anywhere
//                               when 3 wp is no multiple of 4); the last lane of a row that is no multiple of 4 wide stores bytes.
//                               The filter's branch is per pixel: in a wave whose lanes all have radii 1 x 1 no lane enters
//                               the general tent loop.  The three counts go through LDS atomics into one global atomic each per
//                               workgroup: integers, so the order does not matter.
//   sized_unwarp_ragged_kernel  the same tile function on a flat grid over the tiles of up to DVD_RAGGED_CAP documents, their
//                               table a kernel argument
//   sized_footprint_kernel      the same staging; the radii as two bytes per pixel, no gather
// No scratch memory.
#include "common.h"
#include "hwc_bytes.h"
#include "sized_core.h"

namespace dvd {
namespace sz {

struct Stage {
  Pos tile[kHaloW * kHaloH];
  AxisTerm xt[kHaloW], yt[kHaloH];
  unsigned cnt[DVD_SIZED_STATS];
};

// a pixel's neighbourhood in the LDS tile
struct TileAt {
  const Pos* at0;
  __device__ __forceinline__ Pos operator()(int dy, int dx) const { return at0[dy * kHaloW + dx]; }
};

// the Q8 positions of the tile at (x0, y0) and of its halo; off the page: kNone.  up = make_up(g, hp, wp, scale).
__device__ __forceinline__ void stage_tile(const float* __restrict__ flow, const UpParams& up, int hs, int ws, int x0, int y0, Stage& s) {
  const int t = threadIdx.x;
  if (t < kHaloW) {                                        // waves 0 and 1: the columns
    const int x = x0 - 1 + t;
    if (x >= 0 && x < up.w) s.xt[t] = axis_term(up.sx, up.sbx, x, up.g);
  }
  if (t >= 128 && t < 128 + kHaloH) {                      // wave 2: the rows
    const int y = y0 - 1 + (t - 128);
    if (y >= 0 && y < up.h) s.yt[t - 128] = axis_term(up.sy, up.sby, y, up.g);
  }
  if (t >= 192 && t < 192 + DVD_SIZED_STATS) s.cnt[t - 192] = 0;
  __syncthreads();
  for (int i = t; i < kHaloW * kHaloH; i += kBlock) {
    const int ty = i / kHaloW, tx = i - ty * kHaloW;
    const int y = y0 - 1 + ty, x = x0 - 1 + tx;
    Pos p;
    p.x = kNone;
    p.y = 0;
    if (y >= 0 && y < up.h && x >= 0 && x < up.w) {
      float gx, gy;
      flow_grid_from(flow, up, s.yt[ty], s.xt[tx], gx, gy);
      p = pos_of(gx, gy, hs, ws);
    }
    s.tile[i] = p;
  }
  __syncthreads();
}

// One tile of one document.  Every thread of the workgroup comes here and reaches every barrier.
__device__ __forceinline__ void unwarp_tile(const float* __restrict__ flow, const UpParams& up, const uint8_t* __restrict__ src, int hs,
                                            int ws, uint8_t* __restrict__ out, int max_radius, unsigned long long* __restrict__ stats,
                                            int x0, int y0, Stage& s) {
  stage_tile(flow, up, hs, ws, x0, y0, s);
  const int ly = threadIdx.x / (kTileW / kPer), lx = (threadIdx.x % (kTileW / kPer)) * kPer;
  const int y = y0 + ly, xa = x0 + lx;
  Counts n;
  n.capped = n.outside = n.invalid = 0;
  if (y < up.h && xa < up.w) {
    const int npix = up.w - xa < kPer ? up.w - xa : kPer;
    uint32_t bytes[3 * kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      uint32_t rgb[3] = {0, 0, 0};
      if (k < npix) {
        TileAt at;
        at.at0 = s.tile + (ly + 1) * kHaloW + lx + k + 1;
        pixel_at(src, hs, ws, at, max_radius, rgb, n);
      }
      bytes[3 * k] = rgb[0];
      bytes[3 * k + 1] = rgb[1];
      bytes[3 * k + 2] = rgb[2];
    }
    uint8_t* dst = out + 3 * ((size_t)y * up.w + xa);
    if (npix == kPer) {
      store12(dst, bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24, bytes[4] | bytes[5] << 8 | bytes[6] << 16 | bytes[7] << 24,
              bytes[8] | bytes[9] << 8 | bytes[10] << 16 | bytes[11] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < kPer - 1; ++k)
        if (k < npix) {
          dst[3 * k] = (uint8_t)bytes[3 * k];
          dst[3 * k + 1] = (uint8_t)bytes[3 * k + 1];
          dst[3 * k + 2] = (uint8_t)bytes[3 * k + 2];
        }
    }
  }
  if (stats) {                                             // uniform over the launch
    if (n.capped) atomicAdd(&s.cnt[0], n.capped);
    if (n.outside) atomicAdd(&s.cnt[1], n.outside);
    if (n.invalid) atomicAdd(&s.cnt[2], n.invalid);
    __syncthreads();
    if (threadIdx.x < DVD_SIZED_STATS && s.cnt[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (unsigned long long)s.cnt[threadIdx.x]);
  }
}

__global__ __launch_bounds__(kBlock) void sized_unwarp_kernel(const float* __restrict__ flow, UpParams up, const uint8_t* __restrict__ src,
                                                              int hs, int ws, uint8_t* __restrict__ out, int max_radius,
                                                              unsigned long long* __restrict__ stats) {
  __shared__ Stage s;
  unwarp_tile(flow, up, src, hs, ws, out, max_radius, stats, blockIdx.x * kTileW, blockIdx.y * kTileH, s);
}

// The per-document table of the ragged launch: by value, a structure of arrays, as ragged.h's.  64 x 52 B = 3328 B of the
// 4 KiB a HIP kernel may take.
struct RaggedSized {
  const uint8_t* src[DVD_RAGGED_CAP];
  uint8_t* out[DVD_RAGGED_CAP];
  int hs[DVD_RAGGED_CAP], ws[DVD_RAGGED_CAP], hp[DVD_RAGGED_CAP], wp[DVD_RAGGED_CAP];
  unsigned tile_end[DVD_RAGGED_CAP];                       // inclusive prefix sum of the documents' tile counts
  float sy[DVD_RAGGED_CAP], sx[DVD_RAGGED_CAP], sby[DVD_RAGGED_CAP], sbx[DVD_RAGGED_CAP];   // make_up of each page
  int n;
};

__global__ __launch_bounds__(kBlock) void sized_unwarp_ragged_kernel(const float* __restrict__ flow, int g, float scale, int max_radius,
                                                                     unsigned long long* __restrict__ stats, RaggedSized tab) {
  __shared__ Stage s;
  const unsigned tile = blockIdx.x;
  int lo = 0, hi = tab.n - 1;                              // the first d with tile < tile_end[d]: wave-uniform, on the scalar unit
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tile >= tab.tile_end[mid]) lo = mid + 1;
    else hi = mid;
  }
  const int d = __builtin_amdgcn_readfirstlane(lo);
  UpParams up;
  up.g = g;
  up.h = tab.hp[d];
  up.w = tab.wp[d];
  up.sy = tab.sy[d];
  up.sx = tab.sx[d];
  up.sby = tab.sby[d];
  up.sbx = tab.sbx[d];
  up.scale = scale;
  up.small = (up.h + up.w <= 128) ? 1 : 0;
  const unsigned local = tile - (d ? tab.tile_end[d - 1] : 0u);
  const unsigned ntx = ((unsigned)up.w + kTileW - 1) / kTileW;
  const unsigned by = local / ntx, bx = local - by * ntx;
  unwarp_tile(flow + (size_t)d * 2 * g * g, up, tab.src[d], tab.hs[d], tab.ws[d], tab.out[d], max_radius,
              stats ? stats + (size_t)d * DVD_SIZED_STATS : nullptr, (int)bx * kTileW, (int)by * kTileH, s);
}

__global__ __launch_bounds__(kBlock) void sized_footprint_kernel(const float* __restrict__ flow, UpParams up, int hs, int ws, int max_radius,
                                                                 uint16_t* __restrict__ out) {
  __shared__ Stage s;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  stage_tile(flow, up, hs, ws, x0, y0, s);
  const int ly = threadIdx.x / (kTileW / kPer), lx = (threadIdx.x % (kTileW / kPer)) * kPer;
  const int y = y0 + ly;
  if (y >= up.h) return;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int x = x0 + lx + k;
    if (x >= up.w) continue;
    TileAt at;
    at.at0 = s.tile + (ly + 1) * kHaloW + lx + k + 1;
    out[(size_t)y * up.w + x] = radii_at(at, max_radius);
  }
}

static long tiles_of(int hp, int wp) { return (long)cdiv(wp, kTileW) * cdiv(hp, kTileH); }

// The documents d0 .. d0 + launch_len - 1 go into one launch: at most DVD_RAGGED_CAP of them and at most kMaxTiles tiles, so
// that gridDim.x * blockDim.x stays below 2^32 (HIP's limit; 2^23 tiles x 256 lanes = 2^31).  One page has at most
// 256 x 1024 = 2^18 tiles, so a launch always takes at least one document.
constexpr long kMaxTiles = 1l << 23;
static int launch_len(const dvd_sized_image* docs, int d0, int n) {
  long tiles = 0;
  int m = 0;
  for (; m < DVD_RAGGED_CAP && d0 + m < n; ++m) {
    tiles += tiles_of(docs[d0 + m].hp, docs[d0 + m].wp);
    if (tiles > kMaxTiles && m > 0) break;
  }
  return m;
}

}  // namespace sz
}  // namespace dvd

using namespace dvd;

#define SIZED_REQUIRE(cond, code, ...) \
  do {                                 \
    if (!(cond)) {                     \
      dvd::set_error(__VA_ARGS__);     \
      return code;                     \
    }                                  \
  } while (0)

#define SIZED_CHECK_PARAMS(name)                                                                                                         \
  SIZED_REQUIRE(sz::check_params(scale, max_radius) == DVD_OK, DVD_E_SIZED_PARAM, name ": scale = %g, max_radius = %d: a finite scale, " \
                "max_radius 1..%d", (double)scale, max_radius, sz::kMaxRadius)

extern "C" int dvd_unwarp_u8_sized(const float* flow, int g, const uint8_t* src, int hs, int ws, uint8_t* out, int hp, int wp, float scale,
                                   int max_radius, unsigned long long* stats, void* stream) {
  SIZED_REQUIRE(sz::check_shape(g, hs, ws, hp, wp) == DVD_OK, DVD_E_SIZED_SHAPE,
                "unwarp_u8_sized: photograph %d x %d, page %d x %d, g = %d: sides 1..%d, g %d..%d", hs, ws, hp, wp, g, sz::kMaxSide,
                nz::kMinGrid, nz::kMaxGrid);
  SIZED_CHECK_PARAMS("unwarp_u8_sized");
  DVD_REQUIRE(flow && src && out, "unwarp_u8_sized: null pointer");
  DVD_REQUIRE(sz::check_pointers(flow, src, out, hs, ws, hp, wp) == DVD_OK, "unwarp_u8_sized: out must share no byte with src");
  DVD_REQUIRE(((uintptr_t)stats & 7) == 0, "unwarp_u8_sized: misaligned stats");
  if (stats && hipMemsetAsync(stats, 0, DVD_SIZED_STATS * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
    return check_launch("unwarp_u8_sized");
  const dim3 grid((unsigned)cdiv(wp, sz::kTileW), (unsigned)cdiv(hp, sz::kTileH));
  sz::sized_unwarp_kernel<<<grid, sz::kBlock, 0, (hipStream_t)stream>>>(flow, make_up(g, hp, wp, scale), src, hs, ws, out, max_radius, stats);
  return check_launch("unwarp_u8_sized");
}

extern "C" int dvd_unwarp_u8_sized_ragged(const float* flow, int g, const dvd_sized_image* docs, int n, float scale, int max_radius,
                                          unsigned long long* stats, void* stream) {
  DVD_REQUIRE(flow && docs, "unwarp_u8_sized_ragged: null pointer");
  DVD_REQUIRE(n >= 0, "unwarp_u8_sized_ragged: bad batch %d", n);
  SIZED_CHECK_PARAMS("unwarp_u8_sized_ragged");
  for (int d = 0; d < n; ++d) {                            // every document is checked before the first HIP call
    const dvd_sized_image& im = docs[d];
    SIZED_REQUIRE(sz::check_shape(g, im.hs, im.ws, im.hp, im.wp) == DVD_OK, DVD_E_SIZED_SHAPE,
                  "unwarp_u8_sized_ragged: document %d: photograph %d x %d, page %d x %d, g = %d: sides 1..%d, g %d..%d", d, im.hs, im.ws,
                  im.hp, im.wp, g, sz::kMaxSide, nz::kMinGrid, nz::kMaxGrid);
    DVD_REQUIRE(im.src && im.out, "unwarp_u8_sized_ragged: null pointer in document %d", d);
    DVD_REQUIRE(sz::check_pointers(flow, im.src, im.out, im.hs, im.ws, im.hp, im.wp) == DVD_OK,
                "unwarp_u8_sized_ragged: out of document %d must share no byte with its src", d);
  }
  DVD_REQUIRE(((uintptr_t)stats & 7) == 0, "unwarp_u8_sized_ragged: misaligned stats");
  // the documents of ONE launch run side by side: there a page may share no byte with any photograph or any other page
  for (int d0 = 0; d0 < n; d0 += sz::launch_len(docs, d0, n))
    for (int a = d0, end = d0 + sz::launch_len(docs, d0, n); a < end; ++a)
      for (int b = d0; b < end; ++b) {
        if (a == b) continue;
        const size_t an = sz::image_bytes(docs[a].hp, docs[a].wp);
        DVD_REQUIRE(!sz::bytes_overlap(docs[a].out, an, docs[b].src, sz::image_bytes(docs[b].hs, docs[b].ws)) &&
                        !sz::bytes_overlap(docs[a].out, an, docs[b].out, sz::image_bytes(docs[b].hp, docs[b].wp)),
                    "unwarp_u8_sized_ragged: out of document %d must share no byte with src or out of document %d", a, b);
      }
  if (n == 0) return DVD_OK;
  if (stats && hipMemsetAsync(stats, 0, (size_t)n * DVD_SIZED_STATS * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
    return check_launch("unwarp_u8_sized_ragged");
  for (int d0 = 0; d0 < n;) {
    sz::RaggedSized tab;
    long tiles = 0;
    const int m = sz::launch_len(docs, d0, n);
    for (int k = 0; k < m; ++k) {
      const dvd_sized_image& im = docs[d0 + k];
      tiles += sz::tiles_of(im.hp, im.wp);
      const UpParams p = make_up(g, im.hp, im.wp, scale);
      tab.src[k] = im.src; tab.out[k] = im.out; tab.hs[k] = im.hs; tab.ws[k] = im.ws; tab.hp[k] = im.hp; tab.wp[k] = im.wp;
      tab.tile_end[k] = (unsigned)tiles;
      tab.sy[k] = p.sy; tab.sx[k] = p.sx; tab.sby[k] = p.sby; tab.sbx[k] = p.sbx;
    }
    for (int k = m; k < DVD_RAGGED_CAP; ++k) {             // unused entries: defined values in the kernel argument
      tab.src[k] = nullptr; tab.out[k] = nullptr; tab.hs[k] = tab.ws[k] = tab.hp[k] = tab.wp[k] = 0; tab.tile_end[k] = (unsigned)tiles;
      tab.sy[k] = tab.sx[k] = tab.sby[k] = tab.sbx[k] = 0.f;
    }
    tab.n = m;
    sz::sized_unwarp_ragged_kernel<<<(unsigned)tiles, sz::kBlock, 0, (hipStream_t)stream>>>(
        flow + (size_t)d0 * 2 * g * g, g, scale, max_radius, stats ? stats + (size_t)d0 * DVD_SIZED_STATS : nullptr, tab);
    if (int e = check_launch("unwarp_u8_sized_ragged")) return e;
    d0 += m;
  }
  return DVD_OK;
}

extern "C" int dvd_sized_footprint(const float* flow, int g, int hs, int ws, int hp, int wp, float scale, int max_radius, uint16_t* out,
                                   void* stream) {
  SIZED_REQUIRE(sz::check_shape(g, hs, ws, hp, wp) == DVD_OK, DVD_E_SIZED_SHAPE,
                "sized_footprint: photograph %d x %d, page %d x %d, g = %d: sides 1..%d, g %d..%d", hs, ws, hp, wp, g, sz::kMaxSide,
                nz::kMinGrid, nz::kMaxGrid);
  SIZED_CHECK_PARAMS("sized_footprint");
  DVD_REQUIRE(flow && out, "sized_footprint: null pointer");
  DVD_REQUIRE(((uintptr_t)out & 1) == 0, "sized_footprint: misaligned pointer");
  const dim3 grid((unsigned)cdiv(wp, sz::kTileW), (unsigned)cdiv(hp, sz::kTileH));
  sz::sized_footprint_kernel<<<grid, sz::kBlock, 0, (hipStream_t)stream>>>(flow, make_up(g, hp, wp, scale), hs, ws, max_radius, out);
  return check_launch("sized_footprint");
}
