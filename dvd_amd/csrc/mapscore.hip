// A predicted map scored against a ground-truth map.  The arithmetic is mapscore_core.h's;
// tests/mapscore_model.py restates it.
//   map_errors_kernel<Pred, Gt>    the planes e[n] (end-point error) and sigma[n] (spread of the hypotheses) of one document at
//                                  the ground truth's h x w, 0xffffffff at an invalid pixel, and per workgroup the partials of the
//                                  headline numbers: five exact counts and the f64 sums of e and e^2 (block_ops.h's wave_sum,
//                                  the four waves left to right).  Either source is FieldSrc, a field [h,w,2], or CoarseSrc, a map [2,g,g].
//   map_metrics_finalize_kernel    one workgroup adds the partials: lane t takes t, t + 256, .. in order, then a tree.
//   select_hist_kernel             exact selection of up to 50 order statistics of u32 keys at once, MSD radix in four 8-bit
//   select_scan_kernel             levels.  Each workgroup strides over the plane and keeps a [slot][256] u32 histogram in LDS
//                                  (a slot = one distinct prefix still alive, found by binary search); the scan kernel, one
//                                  workgroup per rank, adds the block histograms of the rank's slot and turns (histogram,
//                                  remaining rank) into the next level's (prefix, rank).  Nothing crosses to the host between
//                                  the levels.
//   sparsify_bins_kernel           each pixel finds its interval among the 50 thresholds (binary search in LDS) and adds into
//   sparsify_finalize_kernel       [51] x (count, #(e <= 1), #(e <= 5), sum of rint(e 2^20)) with integer LDS atomics; one
//                                  workgroup adds the block partials.
// The only atomics are integer additions, whose result does not depend on their order.  No kernel uses scratch memory; every
// shape takes the same kernels.
#include "block_ops.h"
#include "common.h"
#include "mapscore_core.h"

namespace dvd {
namespace ms {

struct FieldSrc {
  const float* field;        // [h,w,2]
  __device__ __forceinline__ void at(uint32_t pix, int, int, float* u, float* v) const {
    const float2 d = *reinterpret_cast<const float2*>(field + 2 * (size_t)pix);
    *u = d.x;
    *v = d.y;
  }
};

struct CoarseSrc {
  const float* flow;         // [2,g,g]
  Up up;
  __device__ __forceinline__ void at(uint32_t, int i, int j, float* u, float* v) const { full_uv_at(flow, up, i, j, u, v); }
};

template <typename Pred, typename Gt>
__global__ __launch_bounds__(kBlock) void map_errors_kernel(Pred pred, Up up, Gt gt,
                                                            const float* __restrict__ hyps, int n_hyp, uint32_t n,
                                                            uint32_t* __restrict__ e_out, uint32_t* __restrict__ s_out,
                                                            unsigned long long* __restrict__ partials) {
  __shared__ unsigned long long red[kBlock / 64][kPartial];
  uint32_t c_valid = 0, c1 = 0, c3 = 0, c5 = 0, cfl = 0;
  double se = 0.0, se2 = 0.0;
#pragma unroll 1
  for (int k = 0; k < kPer; ++k) {
    const uint32_t pix = (blockIdx.x * kPer + k) * kBlock + threadIdx.x;       // below 2^28 + 1024
    if (pix >= n) continue;
    const uint32_t i = pix / (uint32_t)up.w, j = pix - i * (uint32_t)up.w;
    float pu, pv, gu, gv, e = 0.f, m = 0.f, sigma = 0.f;
    pred.at(pix, (int)i, (int)j, &pu, &pv);
    gt.at(pix, (int)i, (int)j, &gu, &gv);
    bool sigma_ok = true;
    if (n_hyp >= 2) sigma = spread_at(hyps, n_hyp, up, (int)i, (int)j, &sigma_ok);
    const bool valid = pixel_error(pu, pv, gu, gv, sigma_ok, &e, &m);
    e_out[pix] = valid ? bits_of(e) : kInvalid;
    s_out[pix] = valid ? bits_of(sigma) : kInvalid;
    if (valid) {
      c_valid += 1;
      c1 += e <= 1.f;
      c3 += e <= 3.f;
      c5 += e <= 5.f;
      cfl += fl_outlier(e, m);
      se += (double)e;
      se2 += (double)e * (double)e;
    }
  }
  c_valid = wave_sum(c_valid);
  c1 = wave_sum(c1);
  c3 = wave_sum(c3);
  c5 = wave_sum(c5);
  cfl = wave_sum(cfl);
  se = wave_sum(se);
  se2 = wave_sum(se2);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* r = red[threadIdx.x >> 6];
    r[0] = c_valid;
    r[1] = c1;
    r[2] = c3;
    r[3] = c5;
    r[4] = cfl;
    r[5] = (unsigned long long)__double_as_longlong(se);
    r[6] = (unsigned long long)__double_as_longlong(se2);
  }
  __syncthreads();
  if (threadIdx.x < kPartial) {
    const int q = threadIdx.x;
    unsigned long long out;
    if (q < 5) {
      out = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    } else {
      const double t = ((__longlong_as_double((long long)red[0][q]) + __longlong_as_double((long long)red[1][q])) +
                        __longlong_as_double((long long)red[2][q])) + __longlong_as_double((long long)red[3][q]);
      out = (unsigned long long)__double_as_longlong(t);
    }
    partials[(size_t)blockIdx.x * kPartial + q] = out;
  }
}

// out[0..4] u64 counts, out[5..6] the bits of the f64 sums
__global__ __launch_bounds__(kBlock) void map_metrics_finalize_kernel(const unsigned long long* __restrict__ partials, long blocks,
                                                                      unsigned long long* __restrict__ out) {
  __shared__ unsigned long long cnt[kBlock];
  __shared__ double sum[kBlock];
  const int tid = threadIdx.x;
  for (int q = 0; q < kPartial; ++q) {
    unsigned long long c = 0;
    double s = 0.0;
    for (long t = tid; t < blocks; t += kBlock) {
      const unsigned long long v = partials[(size_t)t * kPartial + q];
      if (q < 5) c += v;
      else s += __longlong_as_double((long long)v);
    }
    cnt[tid] = c;
    sum[tid] = s;
    __syncthreads();
    for (int st = kBlock / 2; st >= 1; st >>= 1) {
      if (tid < st) {
        cnt[tid] += cnt[tid + st];
        sum[tid] += sum[tid + st];
      }
      __syncthreads();
    }
    if (tid == 0) out[q] = q < 5 ? cnt[0] : (unsigned long long)__double_as_longlong(sum[0]);
    __syncthreads();
  }
}

// part [gridDim.x][kMaxRanks][256]: the histogram of the next digit of every key whose prefix is a live slot's
__global__ __launch_bounds__(kBlock) void select_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, int level, int k,
                                                             const SelState* __restrict__ st, uint32_t* __restrict__ part) {
  __shared__ uint32_t hist[kMaxRanks * 256];
  __shared__ uint32_t table[kMaxRanks];
  __shared__ int live;
  if (threadIdx.x == 0) {
    int unused = 0;
    live = level ? sel_slots(st->prefix[level & 1], k, 0, table, &unused) : 1;
  }
  __syncthreads();
  const int nslots = live;
  for (int i = threadIdx.x; i < nslots * 256; i += kBlock) hist[i] = 0;
  __syncthreads();
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n; p += gridDim.x * kBlock) {
    const uint32_t key = keys[p];
    const int slot = level ? sel_slot(table, nslots, sel_prefix(key, level)) : 0;
    if (slot >= 0) atomicAdd(&hist[slot * 256 + sel_digit(key, level)], 1u);
  }
  __syncthreads();
  uint32_t* mine = part + (size_t)blockIdx.x * kMaxRanks * 256;
  for (int i = threadIdx.x; i < nslots * 256; i += kBlock) mine[i] = hist[i];
}

// One workgroup per rank: add the block histograms of the rank's slot (lane t the bin t, the blocks in order), then find the
// rank's digit.  After level 3 the key is complete.
__global__ __launch_bounds__(kBlock) void select_scan_kernel(const uint32_t* __restrict__ part, int blocks, int level, Ranks ranks, int k,
                                                             SelState* __restrict__ st, uint32_t* __restrict__ out) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t table[kMaxRanks];
  __shared__ int mine;
  const int r = blockIdx.x, tid = threadIdx.x;
  const uint32_t* prefix = st->prefix[level & 1];
  if (tid == 0) {
    int slot = 0;
    if (level) sel_slots(prefix, k, r, table, &slot);
    mine = slot;
  }
  __syncthreads();
  const uint32_t* col = part + (size_t)mine * 256 + tid;
  uint32_t acc = 0;
#pragma unroll 8
  for (int b = 0; b < blocks; ++b) acc += col[(size_t)b * kMaxRanks * 256];
  hist[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    uint32_t rem = level ? st->rem[level & 1][r] : ranks.r[r];
    const uint32_t now = ((level ? prefix[r] : 0u) << 8) | sel_walk(hist, &rem);
    st->prefix[(level + 1) & 1][r] = now;
    st->rem[(level + 1) & 1][r] = rem;
    if (level == 3) out[r] = now;
  }
}

// part [gridDim.x][k + 1][kBinWords] u64; bin b = the pixels whose key lies below or on exactly b of the thresholds
__global__ __launch_bounds__(kBlock) void sparsify_bins_kernel(const uint32_t* __restrict__ e_bits, const uint32_t* __restrict__ keys,
                                                               uint32_t n, const uint32_t* __restrict__ thr, int k,
                                                               unsigned long long* __restrict__ part) {
  __shared__ unsigned long long bins[(kMaxRanks + 1) * kBinWords];
  __shared__ uint32_t table[kMaxRanks];
  if (threadIdx.x < k) table[threadIdx.x] = thr[threadIdx.x];
  for (int i = threadIdx.x; i < (k + 1) * kBinWords; i += kBlock) bins[i] = 0;
  __syncthreads();
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n; p += gridDim.x * kBlock) {
    const uint32_t eb = e_bits[p];
    if (eb == kInvalid) continue;
    const float e = float_of(eb);
    unsigned long long* b = bins + bin_of(table, k, keys[p]) * kBinWords;
    atomicAdd(&b[0], 1ull);
    if (e <= 1.f) atomicAdd(&b[1], 1ull);
    if (e <= 5.f) atomicAdd(&b[2], 1ull);
    atomicAdd(&b[3], fixed_of(e));
  }
  __syncthreads();
  unsigned long long* mine = part + (size_t)blockIdx.x * (kMaxRanks + 1) * kBinWords;
  for (int i = threadIdx.x; i < (k + 1) * kBinWords; i += kBlock) mine[i] = bins[i];
}

__global__ __launch_bounds__(kBlock) void sparsify_finalize_kernel(const unsigned long long* __restrict__ part, int blocks, int words,
                                                                   unsigned long long* __restrict__ out) {
  if ((int)threadIdx.x >= words) return;
  unsigned long long acc = 0;
  for (int b = 0; b < blocks; ++b) acc += part[(size_t)b * (kMaxRanks + 1) * kBinWords + threadIdx.x];
  out[threadIdx.x] = acc;
}

}  // namespace ms
}  // namespace dvd

using namespace dvd;

#define MAP_REQUIRE(cond, code, ...) \
  do {                               \
    if (!(cond)) {                   \
      dvd::set_error(__VA_ARGS__);   \
      return code;                   \
    }                                \
  } while (0)

extern "C" long dvd_mapscore_workspace_bytes(int h, int w) {
  MAP_REQUIRE(ms::check_size(h, w) == DVD_OK, DVD_E_MAP_SHAPE, "mapscore_workspace_bytes: h = %d, w = %d: sides 1..%d", h, w,
              ms::kMaxSide);
  return ms::layout(ms::pixels(h, w)).total;
}

extern "C" int dvd_map_errors(const float* flow, int g, const float* gt, int gt_g, const float* hyps, int n_hyp, int h, int w,
                              float* e, float* sigma, void* ws, void* stream) {
  MAP_REQUIRE(ms::check_errors(g, gt_g, n_hyp, h, w) == DVD_OK, DVD_E_MAP_SHAPE,
              "map_errors: g = %d, gt_g = %d, n_hyp = %d, h = %d, w = %d: sides 1..%d, g and gt_g %d..%d or 0 (a field), n_hyp 1..%d (1 with g = 0)", g,
              gt_g, n_hyp, h, w, ms::kMaxSide, ms::kMinGrid, ms::kMaxGrid, ms::kMaxHyp);
  DVD_REQUIRE(flow && gt && e && sigma && ws && (n_hyp < 2 || hyps), "map_errors: null pointer");
  DVD_REQUIRE(((uintptr_t)flow & (g ? 3 : 7)) == 0 && ((uintptr_t)gt & (gt_g ? 3 : 7)) == 0 && ((uintptr_t)hyps & 3) == 0 &&
                  ((uintptr_t)e & 3) == 0 && ((uintptr_t)sigma & 3) == 0 && ((uintptr_t)ws & 255) == 0,
              "map_errors: misaligned pointer");
  const long n = ms::pixels(h, w);
  const long blocks = ms::error_blocks(n);
  auto* partials = (unsigned long long*)((char*)ws + ms::layout(n).partials);
  const fv::Up up = fv::make_up(g ? g : 2, h, w);       // g = 0: only its w is read
  const ms::FieldSrc pf{flow}, gf{gt};
  const ms::CoarseSrc pc{flow, up}, gc{gt, fv::make_up(gt_g ? gt_g : 2, h, w)};
  const unsigned grid = (unsigned)blocks;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* eb = (uint32_t*)e;
  uint32_t* sb = (uint32_t*)sigma;
  if (g && gt_g) ms::map_errors_kernel<<<grid, ms::kBlock, 0, s>>>(pc, up, gc, hyps, n_hyp, (uint32_t)n, eb, sb, partials);
  else if (g) ms::map_errors_kernel<<<grid, ms::kBlock, 0, s>>>(pc, up, gf, hyps, n_hyp, (uint32_t)n, eb, sb, partials);
  else if (gt_g) ms::map_errors_kernel<<<grid, ms::kBlock, 0, s>>>(pf, up, gc, hyps, n_hyp, (uint32_t)n, eb, sb, partials);
  else ms::map_errors_kernel<<<grid, ms::kBlock, 0, s>>>(pf, up, gf, hyps, n_hyp, (uint32_t)n, eb, sb, partials);
  return check_launch("map_errors");
}

extern "C" int dvd_map_metrics(const void* ws, int h, int w, void* out, void* stream) {
  MAP_REQUIRE(ms::check_size(h, w) == DVD_OK, DVD_E_MAP_SHAPE, "map_metrics: h = %d, w = %d: sides 1..%d", h, w, ms::kMaxSide);
  DVD_REQUIRE(ws && out, "map_metrics: null pointer");
  DVD_REQUIRE(((uintptr_t)ws & 255) == 0 && ((uintptr_t)out & 7) == 0, "map_metrics: misaligned pointer");
  const long n = ms::pixels(h, w);
  const auto* partials = (const unsigned long long*)((const char*)ws + ms::layout(n).partials);
  ms::map_metrics_finalize_kernel<<<1, ms::kBlock, 0, (hipStream_t)stream>>>(partials, ms::error_blocks(n), (unsigned long long*)out);
  return check_launch("map_metrics");
}

extern "C" int dvd_select_u32(const uint32_t* keys, long n, const uint32_t* ranks, int k, uint32_t* out, void* ws, void* stream) {
  MAP_REQUIRE(ms::check_plane(n) == DVD_OK, DVD_E_MAP_SHAPE, "select_u32: n = %ld: 1..%ld keys", n, (long)ms::kMaxSide * ms::kMaxSide);
  MAP_REQUIRE(ms::check_ranks(ranks, k, n) == DVD_OK, DVD_E_MAP_RANKS,
              "select_u32: k = %d ranks: 1..%d of them on the host, non-decreasing, each below n = %ld", k, ms::kMaxRanks, n);
  DVD_REQUIRE(keys && out && ws, "select_u32: null pointer");
  DVD_REQUIRE(((uintptr_t)keys & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)ws & 255) == 0, "select_u32: misaligned pointer");
  const ms::Layout l = ms::layout(n);
  auto* st = (ms::SelState*)((char*)ws + l.state);
  auto* part = (uint32_t*)((char*)ws + l.hist);
  ms::Ranks r;
  for (int i = 0; i < ms::kMaxRanks; ++i) r.r[i] = i < k ? ranks[i] : 0u;
  const int blocks = ms::strided_blocks(n);
  hipStream_t s = (hipStream_t)stream;
  for (int level = 0; level < 4; ++level) {
    ms::select_hist_kernel<<<blocks, ms::kBlock, 0, s>>>(keys, (uint32_t)n, level, k, st, part);
    ms::select_scan_kernel<<<k, ms::kBlock, 0, s>>>(part, blocks, level, r, k, st, out);
  }
  return check_launch("select_u32");
}

extern "C" int dvd_sparsify_bins(const float* e, const float* key, long n, const uint32_t* thr, int k, unsigned long long* out, void* ws,
                                 void* stream) {
  MAP_REQUIRE(ms::check_plane(n) == DVD_OK, DVD_E_MAP_SHAPE, "sparsify_bins: n = %ld: 1..%ld pixels", n, (long)ms::kMaxSide * ms::kMaxSide);
  MAP_REQUIRE(k >= 1 && k <= ms::kMaxRanks, DVD_E_MAP_RANKS, "sparsify_bins: k = %d thresholds: 1..%d", k, ms::kMaxRanks);
  DVD_REQUIRE(e && key && thr && out && ws, "sparsify_bins: null pointer");
  DVD_REQUIRE(((uintptr_t)e & 3) == 0 && ((uintptr_t)key & 3) == 0 && ((uintptr_t)thr & 3) == 0 && ((uintptr_t)out & 7) == 0 &&
                  ((uintptr_t)ws & 255) == 0,
              "sparsify_bins: misaligned pointer");
  auto* part = (unsigned long long*)((char*)ws + ms::layout(n).bins);
  const int blocks = ms::strided_blocks(n);
  hipStream_t s = (hipStream_t)stream;
  ms::sparsify_bins_kernel<<<blocks, ms::kBlock, 0, s>>>((const uint32_t*)e, (const uint32_t*)key, (uint32_t)n, thr, k, part);
  ms::sparsify_finalize_kernel<<<1, ms::kBlock, 0, s>>>(part, blocks, (k + 1) * ms::kBinWords, out);
  return check_launch("sparsify_bins");
}
