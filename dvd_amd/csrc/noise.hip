// Keyed sampler noise and the map deviation.  The arithmetic is noise_core.h's; tests/noise_model.py
// restates it bit for bit.
//   randn_keyed_kernel      [docs*n_hyp,2,g,g] standard normals: a function of (key of the document, hypothesis, slot, element)
//                           only - not of the batch, of the loader's order or of any generator's state.  One lane per quad of
//                           four elements (one Philox block, two Box-Muller pairs); flat grid; registers only.
//   map_deviation_kernel    per document the f64 sum of the f32 point distances of two maps [docs,2,g,g]: lane partials,
//   map_deviation_finalize  block_ops.h's wave_sum, the four waves in order; then one workgroup per document adds the block
//                           partials in a fixed order and scales by kPx / g^2.  No atomics.
// No kernel uses LDS beyond the reduction's few doubles, none uses scratch memory.
#include "block_ops.h"
#include "common.h"
#include "noise_core.h"

namespace dvd {
namespace nz {

constexpr int kFinThreads = 256;

__global__ __launch_bounds__(256) void randn_keyed_kernel(const uint32_t* __restrict__ keys, uint32_t n_hyp, uint32_t elems,
                                                          uint32_t quads, uint32_t slot, size_t total, float* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;       // over docs * n_hyp * quads
  if (idx >= total) return;
  const size_t sample = idx / quads;
  const uint32_t q = (uint32_t)(idx - sample * quads);
  const uint32_t doc = (uint32_t)(sample / n_hyp), h = (uint32_t)(sample - (size_t)doc * n_hyp);
  float z[4];
  quad_normals(keys[2 * doc], keys[2 * doc + 1], q, slot, h, z);
  const uint32_t e = 4 * q;
  float* dst = out + sample * elems + e;
  if (e + 4 <= elems && ((uintptr_t)dst & 15) == 0) {
    *reinterpret_cast<float4*>(dst) = make_float4(z[0], z[1], z[2], z[3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (e + r < elems) dst[r] = z[r];                          // the last quad of an odd g: its surplus is dropped
  }
}

// grid (blocks of a document, documents); partials [docs][blocks]
__global__ __launch_bounds__(kDevBlock) void map_deviation_kernel(const float* __restrict__ a, const float* __restrict__ b, uint32_t gg,
                                                                  double* __restrict__ partials) {
  __shared__ double red[kDevBlock / 64];
  const size_t base = (size_t)blockIdx.y * 2 * gg;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kDevPer; ++k) {
    const uint32_t p = (blockIdx.x * kDevPer + k) * kDevBlock + threadIdx.x;
    if (p < gg) acc += (double)point_distance(a[base + p], a[base + gg + p], b[base + p], b[base + gg + p]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup per document: lane t adds partials t, t + 256, ... in order, then a tree over the 256 lanes
__global__ __launch_bounds__(kFinThreads) void map_deviation_finalize_kernel(const double* __restrict__ partials, int blocks, double count,
                                                                            double* __restrict__ out) {
  __shared__ double red[kFinThreads];
  const int tid = threadIdx.x;
  const double* mine = partials + (size_t)blockIdx.x * blocks;
  double v = 0.0;
  for (int t = tid; t < blocks; t += kFinThreads) v += mine[t];
  red[tid] = v;
  __syncthreads();
  for (int s = kFinThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = kPx * (red[0] / count);
}

}  // namespace nz
}  // namespace dvd

using namespace dvd;

extern "C" int dvd_randn_keyed(const uint32_t* keys, int docs, int n_hyp, int g, uint32_t slot, float* out, void* stream) {
  DVD_REQUIRE(nz::check_randn(docs, n_hyp, g) == DVD_OK,
              "randn_keyed: docs = %d, n_hyp = %d, g = %d: docs and n_hyp 0..65535, g %d..%d, at most 2^38 quads", docs, n_hyp, g,
              nz::kMinGrid, nz::kMaxGrid);
  if (docs == 0 || n_hyp == 0) return DVD_OK;
  DVD_REQUIRE(keys && out, "randn_keyed: null pointer");
  DVD_REQUIRE(((uintptr_t)keys & 3) == 0 && ((uintptr_t)out & 3) == 0, "randn_keyed: misaligned pointer");
  const uint32_t elems = 2u * g * g, quads = (elems + 3) / 4;
  const size_t total = (size_t)docs * n_hyp * quads;
  nz::randn_keyed_kernel<<<cdiv((long)total, 256), 256, 0, (hipStream_t)stream>>>(keys, (uint32_t)n_hyp, elems, quads, slot, total, out);
  return check_launch("randn_keyed");
}

extern "C" long dvd_map_deviation_workspace_bytes(int docs, int g) {
  if (nz::check_deviation(docs, g) != DVD_OK) {
    set_error("map_deviation_workspace_bytes: docs = %d, g = %d: docs 0..65535, g %d..%d", docs, g, nz::kMinGrid, nz::kMaxGrid);
    return DVD_E_ARG;
  }
  return (long)docs * nz::deviation_blocks(g) * (long)sizeof(double);
}

extern "C" int dvd_map_deviation(const float* a, const float* b, int docs, int g, double* out, void* ws, void* stream) {
  DVD_REQUIRE(nz::check_deviation(docs, g) == DVD_OK, "map_deviation: docs = %d, g = %d: docs 0..65535, g %d..%d", docs, g,
              nz::kMinGrid, nz::kMaxGrid);
  if (docs == 0) return DVD_OK;
  DVD_REQUIRE(a && b && out && ws, "map_deviation: null pointer");
  DVD_REQUIRE(((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)ws & 7) == 0,
              "map_deviation: misaligned pointer");
  const uint32_t gg = (uint32_t)g * g;
  const int blocks = (int)nz::deviation_blocks(g);
  hipStream_t s = (hipStream_t)stream;
  nz::map_deviation_kernel<<<dim3(blocks, docs), nz::kDevBlock, 0, s>>>(a, b, gg, (double*)ws);
  nz::map_deviation_finalize_kernel<<<docs, nz::kFinThreads, 0, s>>>((const double*)ws, blocks, (double)gg, out);
  return check_launch("map_deviation");
}
