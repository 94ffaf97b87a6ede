// The map inverse: the predicted backward map page pixel -> photograph position turned round on the
// device.  The arithmetic is mapinv_core.h's; tests/mapinv_model.py restates it.
//   lattice_kernel        one lane per lattice vertex: its Q8 photograph position (flowgrid_core.h's flow_grid_at, the unwarp
//                         tail's own) and its validity flag
//   fill_kernel           the winner plane to 0xffffffff, the fold flags to 0
//   raster_kernel         one lane per triangle: the exact edge tests over its clipped box (at most `budget` pixels, else the
//                         triangle is skipped) and an integer atomicMin of its id into the winner plane; an atomicMin that finds
//                         an id already there marks the pixel as covered twice (every lane stores the same 1).  Per workgroup the
//                         counts of flipped, degenerate and skipped triangles.
//   resolve_kernel        per photograph pixel: the winner's edge values again, fwd, and per workgroup the counts of covered and
//                         of doubly covered pixels
//   stats_kernel          one workgroup adds the block counts in a fixed order
//   cycle_kernel          |backward(fwd(p)) - p| per covered pixel; per workgroup n, the f64 sum (block_ops.h's wave_sum, the four
//   cycle_finalize_kernel waves left to right) and the maximum; one workgroup adds them: lane t takes t, t + 256, .., then a tree
//   overlay_kernel        the mesh picture, three bytes per lane
//   transfer_points_kernel, map_points_kernel   one lane per point
// The only atomic is the integer minimum, whose result does not depend on the order of arrival.  No kernel uses scratch memory;
// every shape takes the same kernels.
#include "block_ops.h"
#include "common.h"
#include "mapinv_core.h"

namespace dvd {
namespace mi {

__global__ __launch_bounds__(kBlock) void lattice_kernel(const float* __restrict__ flow, UpParams up, Mesh m, Vertex* __restrict__ verts,
                                                         uint8_t* __restrict__ valid) {
  const long at = (long)blockIdx.x * kBlock + threadIdx.x;
  if (at >= (long)m.rows * m.cols) return;
  const int r = (int)(at / m.cols), c = (int)(at - (long)r * m.cols);
  Vertex v;
  const bool ok = vertex_at(flow, up, lattice_at(r, m.h, m.step), lattice_at(c, m.w, m.step), &v);
  verts[at] = v;
  valid[at] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void fill_kernel(uint32_t* __restrict__ winner, uint8_t* __restrict__ multi, long n) {
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (long)gridDim.x * kBlock) {
    winner[p] = kInvalid;
    multi[p] = 0;
  }
}

// the sums of up to three per-lane counts over a workgroup, to part[blockIdx.x][words]
template <int kWords>
__device__ __forceinline__ void block_counts(const uint32_t (&c)[kWords], unsigned long long* __restrict__ part) {
  __shared__ uint32_t red[kBlock / 64][kWords];
#pragma unroll
  for (int q = 0; q < kWords; ++q) {
    const uint32_t s = wave_sum(c[q]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < kWords)
    part[(size_t)blockIdx.x * kWords + threadIdx.x] =
        (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void raster_kernel(Mesh m, const Vertex* __restrict__ verts, const uint8_t* __restrict__ valid,
                                                        long tris, uint32_t* __restrict__ winner, uint8_t* __restrict__ multi,
                                                        unsigned long long* __restrict__ part) {
  const long id = (long)blockIdx.x * kBlock + threadIdx.x;
  uint32_t c[3] = {0, 0, 0};
  if (id < tris) {
    const Tri t = make_tri(m, verts, valid, id);
    c[0] = t.kind == kFlipped;
    c[1] = t.kind == kDegenerate;
    c[2] = t.kind == kSkipped;
    // the box lies inside the photograph and holds at most m.budget pixels
    for (int y = t.ymin; y <= t.ymax; ++y)
      for (int x = t.xmin; x <= t.xmax; ++x) {
        long long e[3];
        if (!tri_covers(t, x, y, e)) continue;
        const size_t p = (size_t)y * m.w + x;
        if (atomicMin(&winner[p], (uint32_t)id) != kInvalid) multi[p] = 1;
      }
  }
  block_counts<3>(c, part);
}

__global__ __launch_bounds__(kBlock) void resolve_kernel(Mesh m, const Vertex* __restrict__ verts, const uint8_t* __restrict__ valid,
                                                         const uint32_t* __restrict__ winner, const uint8_t* __restrict__ multi,
                                                         long n, float* __restrict__ fwd, unsigned long long* __restrict__ part) {
  uint32_t c[2] = {0, 0};
#pragma unroll 1
  for (int k = 0; k < kPer; ++k) {
    const long p = ((long)blockIdx.x * kPer + k) * kBlock + threadIdx.x;
    if (p >= n) continue;
    const uint32_t id = winner[p];
    float u = float_of(kInvalid), v = float_of(kInvalid);
    if (id != kInvalid) {
      const int y = (int)(p / m.w), x = (int)(p - (long)y * m.w);
      const Tri t = make_tri(m, verts, valid, (long)id);
      long long e[3];
      tri_covers(t, x, y, e);
      tri_page(t, e, &u, &v);
      c[0] += 1;
      c[1] += multi[p];
    }
    reinterpret_cast<float2*>(fwd)[p] = make_float2(u, v);
  }
  block_counts<2>(c, part);
}

// out[0..5]: covered, fold_px, flipped_tris, degenerate_tris, skipped_tris, tris
__global__ __launch_bounds__(kBlock) void stats_kernel(const unsigned long long* __restrict__ px_part, long px_blocks,
                                                       const unsigned long long* __restrict__ tri_part, long tri_blocks, long tris,
                                                       unsigned long long* __restrict__ out) {
  __shared__ unsigned long long cnt[kBlock];
  const int tid = threadIdx.x;
  for (int q = 0; q < 5; ++q) {
    const unsigned long long* part = q < 2 ? px_part + q : tri_part + (q - 2);
    const long blocks = q < 2 ? px_blocks : tri_blocks;
    const int words = q < 2 ? 2 : 3;
    unsigned long long c = 0;
    for (long t = tid; t < blocks; t += kBlock) c += part[(size_t)t * words];
    cnt[tid] = c;
    __syncthreads();
    for (int st = kBlock / 2; st >= 1; st >>= 1) {
      if (tid < st) cnt[tid] += cnt[tid + st];
      __syncthreads();
    }
    if (tid == 0) out[q] = cnt[0];
    __syncthreads();
  }
  if (tid == 0) out[5] = (unsigned long long)tris;
}

__global__ __launch_bounds__(kBlock) void cycle_kernel(const float* __restrict__ flow, UpParams up, const float* __restrict__ fwd, long n,
                                                       unsigned long long* __restrict__ part) {
  __shared__ unsigned long long red[kBlock / 64][kCycleWords];
  uint32_t cnt = 0, top = 0;
  double sum = 0.0;
#pragma unroll 1
  for (int k = 0; k < kPer; ++k) {
    const long p = ((long)blockIdx.x * kPer + k) * kBlock + threadIdx.x;
    if (p >= n) continue;
    const float2 uv = reinterpret_cast<const float2*>(fwd)[p];
    if (bits_of(uv.x) == kInvalid) continue;
    const int y = (int)(p / up.w), x = (int)(p - (long)y * up.w);
    bool ok;
    const float d = cycle_at(flow, up, uv.x, uv.y, x, y, &ok);
    if (!ok) continue;
    cnt += 1;
    sum += (double)d;
    top = bits_of(d) > top ? bits_of(d) : top;            // a non-negative finite f32 orders as its bit pattern
  }
  cnt = wave_sum(cnt);
  sum = wave_sum(sum);
  top = wave_max(top);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* r = red[threadIdx.x >> 6];
    r[0] = cnt;
    r[1] = (unsigned long long)__double_as_longlong(sum);
    r[2] = top;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* o = part + (size_t)blockIdx.x * kCycleWords;
    o[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    const double t = ((__longlong_as_double((long long)red[0][1]) + __longlong_as_double((long long)red[1][1])) +
                      __longlong_as_double((long long)red[2][1])) + __longlong_as_double((long long)red[3][1]);
    o[1] = (unsigned long long)__double_as_longlong(t);
    unsigned long long mx = red[0][2];
    for (int wv = 1; wv < 4; ++wv) mx = red[wv][2] > mx ? red[wv][2] : mx;
    o[2] = mx;
  }
}

// out[0] n, out[1] the bits of the f64 sum, out[2] the bits of the f32 maximum
__global__ __launch_bounds__(kBlock) void cycle_finalize_kernel(const unsigned long long* __restrict__ part, long blocks,
                                                                unsigned long long* __restrict__ out) {
  __shared__ unsigned long long cnt[kBlock], top[kBlock];
  __shared__ double sum[kBlock];
  const int tid = threadIdx.x;
  unsigned long long c = 0, mx = 0;
  double s = 0.0;
  for (long t = tid; t < blocks; t += kBlock) {
    const unsigned long long* p = part + (size_t)t * kCycleWords;
    c += p[0];
    s += __longlong_as_double((long long)p[1]);
    mx = p[2] > mx ? p[2] : mx;
  }
  cnt[tid] = c;
  sum[tid] = s;
  top[tid] = mx;
  __syncthreads();
  for (int st = kBlock / 2; st >= 1; st >>= 1) {
    if (tid < st) {
      cnt[tid] += cnt[tid + st];
      sum[tid] += sum[tid + st];
      top[tid] = top[tid + st] > top[tid] ? top[tid + st] : top[tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = cnt[0];
    out[1] = (unsigned long long)__double_as_longlong(sum[0]);
    out[2] = top[0];
  }
}

__global__ __launch_bounds__(kBlock) void overlay_kernel(const uint8_t* __restrict__ src, const float* __restrict__ fwd, Overlay o,
                                                         uint8_t* __restrict__ out) {
  const long p = (long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (long)o.h * o.w) return;
  const int y = (int)(p / o.w), x = (int)(p - (long)y * o.w);
  uint8_t rgb[3];
  overlay_at(src, fwd, o, y, x, rgb);
  out[3 * p] = rgb[0];
  out[3 * p + 1] = rgb[1];
  out[3 * p + 2] = rgb[2];
}

__global__ __launch_bounds__(kBlock) void transfer_points_kernel(const float* __restrict__ fwd, int h, int w, const float* __restrict__ pts,
                                                                 long n, float* __restrict__ out) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float u = 0.f, v = 0.f;
  const bool ok = transfer_at(fwd, h, w, pts[2 * i], pts[2 * i + 1], &u, &v);
  out[2 * i] = ok ? u : float_of(kInvalid);
  out[2 * i + 1] = ok ? v : float_of(kInvalid);
}

__global__ __launch_bounds__(kBlock) void map_points_kernel(const float* __restrict__ flow, UpParams up, const float* __restrict__ pts, long n,
                                                            float* __restrict__ out) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float x = 0.f, y = 0.f;
  const bool ok = backward_at(flow, up, pts[2 * i], pts[2 * i + 1], &x, &y);
  out[2 * i] = ok ? x : float_of(kInvalid);
  out[2 * i + 1] = ok ? y : float_of(kInvalid);
}

}  // namespace mi
}  // namespace dvd

using namespace dvd;

#define INV_REQUIRE(cond, code, ...) \
  do {                               \
    if (!(cond)) {                   \
      dvd::set_error(__VA_ARGS__);   \
      return code;                   \
    }                                \
  } while (0)

#define INV_CHECK_SIZE(name)                                                                                                          \
  INV_REQUIRE(mi::check_size(h, w) == DVD_OK, DVD_E_INV_SHAPE, name ": h = %d, w = %d: sides 1..%d", h, w, mi::kMaxSide)
#define INV_CHECK_GRID(name)                                                                                                          \
  INV_REQUIRE(mi::check_grid(g) == DVD_OK, DVD_E_INV_SHAPE, name ": g = %d: %d..%d", g, mi::kMinGrid, mi::kMaxGrid)

static const long kMaxPoints = 1l << 28;

extern "C" long dvd_map_invert_workspace_bytes(int h, int w, int step) {
  INV_CHECK_SIZE("map_invert_workspace_bytes");
  INV_REQUIRE(mi::check_step(step) == DVD_OK, DVD_E_INV_STEP, "map_invert_workspace_bytes: step = %d: 1..%d", step, mi::kMaxSide);
  return mi::layout(mi::make_mesh(h, w, step)).total;
}

extern "C" int dvd_map_invert(const float* flow, int g, int h, int w, int step, float scale, float* fwd, unsigned long long* stats,
                              void* ws, void* stream) {
  INV_CHECK_SIZE("map_invert");
  INV_CHECK_GRID("map_invert");
  INV_REQUIRE(mi::check_step(step) == DVD_OK, DVD_E_INV_STEP, "map_invert: step = %d: 1..%d", step, mi::kMaxSide);
  DVD_REQUIRE(flow && fwd && stats && ws, "map_invert: null pointer");
  DVD_REQUIRE(((uintptr_t)flow & 3) == 0 && ((uintptr_t)fwd & 7) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)ws & 255) == 0,
              "map_invert: misaligned pointer");
  const mi::Mesh m = mi::make_mesh(h, w, step);
  const mi::Layout l = mi::layout(m);
  const UpParams up = make_up(g, h, w, scale);
  char* base = (char*)ws;
  auto* verts = (mi::Vertex*)(base + l.verts);
  auto* valid = (uint8_t*)(base + l.valid);
  auto* winner = (uint32_t*)(base + l.winner);
  auto* multi = (uint8_t*)(base + l.multi);
  auto* tri_part = (unsigned long long*)(base + l.tri_part);
  auto* px_part = (unsigned long long*)(base + l.px_part);
  const long n = (long)h * w, nv = (long)m.rows * m.cols, tris = mi::mesh_tris(m);
  const long fill = (n + mi::kBlock - 1) / mi::kBlock;
  hipStream_t s = (hipStream_t)stream;
  mi::lattice_kernel<<<(unsigned)((nv + mi::kBlock - 1) / mi::kBlock), mi::kBlock, 0, s>>>(flow, up, m, verts, valid);
  mi::fill_kernel<<<(unsigned)(fill < 4096 ? fill : 4096), mi::kBlock, 0, s>>>(winner, multi, n);
  mi::raster_kernel<<<(unsigned)mi::tri_blocks(tris), mi::kBlock, 0, s>>>(m, verts, valid, tris, winner, multi, tri_part);
  mi::resolve_kernel<<<(unsigned)mi::pixel_blocks(n), mi::kBlock, 0, s>>>(m, verts, valid, winner, multi, n, fwd, px_part);
  mi::stats_kernel<<<1, mi::kBlock, 0, s>>>(px_part, mi::pixel_blocks(n), tri_part, mi::tri_blocks(tris), tris, stats);
  return check_launch("map_invert");
}

extern "C" int dvd_map_cycle_error(const float* flow, int g, const float* fwd, int h, int w, float scale, unsigned long long* out,
                                   void* ws, void* stream) {
  INV_CHECK_SIZE("map_cycle_error");
  INV_CHECK_GRID("map_cycle_error");
  DVD_REQUIRE(flow && fwd && out && ws, "map_cycle_error: null pointer");
  DVD_REQUIRE(((uintptr_t)flow & 3) == 0 && ((uintptr_t)fwd & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)ws & 255) == 0,
              "map_cycle_error: misaligned pointer");
  const long n = (long)h * w, blocks = mi::pixel_blocks(n);
  auto* part = (unsigned long long*)((char*)ws + mi::layout(mi::make_mesh(h, w, 1)).cycle_part);
  hipStream_t s = (hipStream_t)stream;
  mi::cycle_kernel<<<(unsigned)blocks, mi::kBlock, 0, s>>>(flow, make_up(g, h, w, scale), fwd, n, part);
  mi::cycle_finalize_kernel<<<1, mi::kBlock, 0, s>>>(part, blocks, out);
  return check_launch("map_cycle_error");
}

extern "C" int dvd_mesh_overlay_rgb8(const uint8_t* src, const float* fwd, int h, int w, int lines, int thickness, uint32_t color,
                                     uint32_t outline_color, int dim, uint8_t* out, void* stream) {
  INV_CHECK_SIZE("mesh_overlay_rgb8");
  INV_REQUIRE(mi::check_overlay(lines, thickness) == DVD_OK, DVD_E_INV_LINES, "mesh_overlay_rgb8: lines = %d, thickness = %d: lines 2..%d, thickness 1..3",
              lines, thickness, mi::kMaxSide);
  DVD_REQUIRE(src && fwd && out, "mesh_overlay_rgb8: null pointer");
  DVD_REQUIRE(((uintptr_t)fwd & 7) == 0, "mesh_overlay_rgb8: misaligned pointer");
  DVD_REQUIRE(src != out, "mesh_overlay_rgb8: out must not be src");
  mi::Overlay o;
  o.h = h;
  o.w = w;
  o.lines = lines;
  o.thickness = thickness;
  o.dim = dim != 0;
  o.color = color;
  o.outline = outline_color;
  const long n = (long)h * w;
  mi::overlay_kernel<<<(unsigned)((n + mi::kBlock - 1) / mi::kBlock), mi::kBlock, 0, (hipStream_t)stream>>>(src, fwd, o, out);
  return check_launch("mesh_overlay_rgb8");
}

extern "C" int dvd_transfer_points(const float* fwd, int h, int w, const float* pts, long n, float* out, void* stream) {
  INV_CHECK_SIZE("transfer_points");
  INV_REQUIRE(n >= 0 && n <= kMaxPoints, DVD_E_INV_POINTS, "transfer_points: n = %ld points: 0..%ld", n, kMaxPoints);
  if (n == 0) return DVD_OK;
  DVD_REQUIRE(fwd && pts && out, "transfer_points: null pointer");
  DVD_REQUIRE(((uintptr_t)fwd & 7) == 0 && ((uintptr_t)pts & 3) == 0 && ((uintptr_t)out & 3) == 0, "transfer_points: misaligned pointer");
  mi::transfer_points_kernel<<<(unsigned)((n + mi::kBlock - 1) / mi::kBlock), mi::kBlock, 0, (hipStream_t)stream>>>(fwd, h, w, pts, n, out);
  return check_launch("transfer_points");
}

extern "C" int dvd_map_points(const float* flow, int g, int h, int w, float scale, const float* pts, long n, float* out, void* stream) {
  INV_CHECK_SIZE("map_points");
  INV_CHECK_GRID("map_points");
  INV_REQUIRE(n >= 0 && n <= kMaxPoints, DVD_E_INV_POINTS, "map_points: n = %ld points: 0..%ld", n, kMaxPoints);
  if (n == 0) return DVD_OK;
  DVD_REQUIRE(flow && pts && out, "map_points: null pointer");
  DVD_REQUIRE(((uintptr_t)flow & 3) == 0 && ((uintptr_t)pts & 3) == 0 && ((uintptr_t)out & 3) == 0, "map_points: misaligned pointer");
  mi::map_points_kernel<<<(unsigned)((n + mi::kBlock - 1) / mi::kBlock), mi::kBlock, 0, (hipStream_t)stream>>>(flow, make_up(g, h, w, scale), pts,
                                                                                                            n, out);
  return check_launch("map_points");
}
