// Local distortion (LD) of the evaluation tail: dense SIFT descriptors of the ground-truth scan and of the dewarped page, a
// coarse-to-fine SIFT-flow field between them by synchronous min-sum belief propagation, and the mean length of that field.
// DESIGN.md section 4.7 holds the definition; tests/sflow_model.py states it in NumPy; the integer arithmetic itself lives in
// sflow_core.h, which sflow_host_check.cpp restates as a CPU program.  The reference leaves LD to offline MATLAB and mex code:
// parity with that pipeline is UNPINNED.
//   sflow_prep / sflow_reduce2   integer-valued f32 -> u8; the integer [1,4,6,4,1] reduce by 2
//   sflow_dsift                  one 16 x 16 tile per workgroup: responses and 3 x 3 cell sums staged in LDS with the halo
//   sflow_offsets                window centres of a level: twice the coarser flow of p >> 1
//   sflow_cost                   128-byte L1 distances with the packed byte SAD, one label row per thread
//   sflow_bp_iter                one synchronous iteration, sender-side: a pixel reads its cost and four messages and writes
//                                the four it sends (registers for a 5 x 5 label grid, LDS for every other window)
//   sflow_select / _finalize     argmin of the belief, the flow, and the LD sum in a fixed order
//   ad_fit / ad_align / ad_weighted (+ two finalizes)   aligned distortion, at the end of the file
// No atomics anywhere: every result is a pure function of its inputs (same bits on every launch, in any batch).  The sums inside
// a wave are block_ops.h's wave_sum, whose order the f64 results are defined by; the workspaces are carved with workspace.h.
#include "common.h"
#include "block_ops.h"
#include "sflow_core.h"
#include "adist_core.h"
#include "workspace.h"

namespace dvd {
namespace sf {

// ---------------------------------------------------------------- planes ----------------------------------------------------
__global__ void __launch_bounds__(256) sflow_prep_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int v = (int)src[i];
  dst[i] = (uint8_t)min(max(v, 0), 255);
}

// both planes per thread; out is ceil(h/2) x ceil(w/2)
__global__ void __launch_bounds__(256) sflow_reduce2_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                            uint8_t* __restrict__ ao, uint8_t* __restrict__ bo, int h, int w,
                                                            int oh, int ow) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= ow) return;
  ao[(size_t)i * ow + j] = (uint8_t)reduce2_at(a, h, w, i, j);
  bo[(size_t)i * ow + j] = (uint8_t)reduce2_at(b, h, w, i, j);
}

// ---------------------------------------------------------------- dense SIFT ------------------------------------------------
constexpr int kDsTile = 16;
constexpr int kDsR = kDsTile + 11;    // rows / columns of responses a tile can touch: -6 .. +20
constexpr int kDsC = kDsTile + 9;     // rows / columns of cell centres: -5 .. +19

// One 16 x 16 tile per workgroup of 256 threads; blockIdx.z = plane.  Every index the definition clamps is clamped into the
// image, so the staged regions are cut to the image: responses of rows [oy-6, oy+20] and cells of rows [oy-5, oy+19], likewise
// the columns.  LDS: 8 x 27 x 28 + 8 x 25 x 26 ints = 45.0 KB.
template <typename T>
__global__ void __launch_bounds__(256) sflow_dsift_kernel(const T* __restrict__ img, int h, int w, int eps,
                                                          uint8_t* __restrict__ out) {
  __shared__ int sr[8][kDsR][kDsR + 1];
  __shared__ int sc[8][kDsC][kDsC + 1];
  const int tid = threadIdx.x;
  const int oy = blockIdx.y * kDsTile, ox = blockIdx.x * kDsTile;
  const T* plane = img + (size_t)blockIdx.z * h * w;
  const int ry0 = max(oy - 6, 0), ry1 = min(oy + kDsTile + 4, h - 1), rx0 = max(ox - 6, 0), rx1 = min(ox + kDsTile + 4, w - 1);
  const int rh = ry1 - ry0 + 1, rw = rx1 - rx0 + 1;
  for (int i = tid; i < rh * rw; i += 256) {
    const int yy = i / rw, xx = i - yy * rw;
    int gx, gy;
    gradient(plane, h, w, ry0 + yy, rx0 + xx, &gx, &gy);
#pragma unroll
    for (int o = 0; o < 8; ++o) sr[o][yy][xx] = response(gx, gy, o);
  }
  __syncthreads();
  const int cy0 = max(oy - 5, 0), cy1 = min(oy + kDsTile + 3, h - 1), cx0 = max(ox - 5, 0), cx1 = min(ox + kDsTile + 3, w - 1);
  const int ch = cy1 - cy0 + 1, cw = cx1 - cx0 + 1;
  for (int i = tid; i < ch * cw; i += 256) {
    const int yy = i / cw, xx = i - yy * cw;
    int ys[3], xs[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ys[k] = clampi(cy0 + yy + k - 1, h) - ry0;
      xs[k] = clampi(cx0 + xx + k - 1, w) - rx0;
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      int s = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) s += sr[o][ys[a]][xs[b]];
      sc[o][yy][xx] = s;
    }
  }
  __syncthreads();
  const int y = oy + (tid >> 4), x = ox + (tid & 15);
  if (y >= h || x >= w) return;
  int cy[4], cx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    cy[i] = cell_at(y, i, h) - cy0;
    cx[i] = cell_at(x, i, w) - cx0;
  }
  // two passes over the 128 LDS values: the norm, then the bytes
  uint64_t ss = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const uint64_t v = (uint64_t)sc[o][cy[i]][cx[j]];
        ss += v * v;
      }
  const uint32_t norm = isqrt64(ss);
  uint4* dst = (uint4*)(out + (((size_t)blockIdx.z * h + y) * w + x) * kDesc);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      uint32_t wd[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = jj * 2 + (k >> 1), o0 = (k & 1) * 4;
        uint32_t pk = 0;
#pragma unroll
        for (int o = 0; o < 4; ++o) pk |= quantise(sc[o0 + o][cy[i]][cx[j]], norm, eps) << (8 * o);
        wd[k] = pk;
      }
      dst[i * 2 + jj] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
}

// ---------------------------------------------------------------- offsets ---------------------------------------------------
// off [2,h,w] = 2 * coarse [2,ch,cw] at (y >> 1, x >> 1)
__global__ void __launch_bounds__(256) sflow_offsets_kernel(const int16_t* __restrict__ coarse, int ch, int cw,
                                                            int16_t* __restrict__ off, int h, int w) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const size_t p = (size_t)y * w + x, q = (size_t)(y >> 1) * cw + (x >> 1);
  off[p] = (int16_t)(2 * coarse[q]);
  off[(size_t)h * w + p] = (int16_t)(2 * coarse[(size_t)ch * cw + q]);
}

// ---------------------------------------------------------------- cost volume -----------------------------------------------
// One thread per (pixel, label row lv): the pixel's own descriptor in 32 registers, the 2 win + 1 descriptors of the row read
// straight from global memory as 16-byte vectors.  A direct gather on every level: below the top level the window centre
// varies per pixel, so there is no common box to stage, a descriptor is exactly one 128-byte line, and neighbouring pixels
// (neighbouring lanes) read neighbouring lines that L2 serves 25 times over; the top level (about 9 000 pixels at the
// benchmark's size) takes the same kernel rather than a second, staged one.
__global__ void __launch_bounds__(256) sflow_cost_kernel(const uint8_t* __restrict__ da, const uint8_t* __restrict__ db,
                                                         const int16_t* __restrict__ off, int h, int w, int win, int gamma,
                                                         int T, uint16_t* __restrict__ cost) {
  const size_t hw = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int n = 2 * win + 1, lv = blockIdx.y;
  const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
  const int ou = off[p], ov = off[hw + p];
  uint32_t a[32];
  const uint4* ap = (const uint4*)(da + p * kDesc);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint4 v = ap[k];
    a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w;
  }
  const int fv = ov + lv - win, qy = y + fv;
  uint16_t* dst = cost + p * (size_t)(n * n) + (size_t)lv * n;
  for (int lu = 0; lu < n; ++lu) {
    const int fu = ou + lu - win, qx = x + fu;
    const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
    uint32_t s = 0;
    if (inside) {
      const uint4* bp = (const uint4*)(db + ((size_t)qy * w + qx) * kDesc);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint4 v = bp[k];
        s = sad4(a[4 * k], v.x, s);
        s = sad4(a[4 * k + 1], v.y, s);
        s = sad4(a[4 * k + 2], v.z, s);
        s = sad4(a[4 * k + 3], v.w, s);
      }
    }
    dst[lu] = (uint16_t)data_cost(inside, s, fu, fv, gamma, T);
  }
}

// ---------------------------------------------------------------- belief propagation ----------------------------------------
// Messages: [4, h, w, L] u16, slot k of a pixel = the message from its left / right / upper / lower neighbour.  An iteration is
// sender-side: pixel q reads its cost and its four incoming messages (5 L values) and writes the message it sends to each
// neighbour into that neighbour's slot (4 L values) of the other buffer.  Every (slot, pixel) has exactly one writer; the slot
// of an absent neighbour is never written and keeps the zero both buffers start with.

// N x N labels held in registers: one pixel per thread.
template <int N>
__global__ void __launch_bounds__(256) sflow_bp_iter_reg_kernel(const uint16_t* __restrict__ cost, const uint16_t* __restrict__ min_,
                                                                uint16_t* __restrict__ mout, const int16_t* __restrict__ off,
                                                                int h, int w, int alpha, int d) {
  constexpr int L = N * N;
  const size_t hw = (size_t)h * w;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= hw) return;
  const int y = (int)(q / w), x = (int)(q - (size_t)y * w);
  int tot[L];
  {
    const uint16_t* c = cost + q * L;
    const uint16_t* m0 = min_ + q * L;
#pragma unroll
    for (int i = 0; i < L; ++i) tot[i] = (int)c[i] + (int)m0[i] + (int)m0[hw * L + i] + (int)m0[2 * hw * L + i] + (int)m0[3 * hw * L + i];
  }
  const int ou = off[q], ov = off[hw + q];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int dy, dx, slot, excl;
    direction(k, &dy, &dx, &slot, &excl);
    const int py = y + dy, px = x + dx;
    if (py < 0 || py >= h || px < 0 || px >= w) continue;
    const size_t p = (size_t)py * w + px;
    const int du0 = (int)off[p] - ou, dv0 = (int)off[hw + p] - ov;
    int pu[2 * N - 1], pv[2 * N - 1];
#pragma unroll
    for (int j = 0; j < 2 * N - 1; ++j) {
      pu[j] = penalty(alpha, d, du0 + j - (N - 1));
      pv[j] = penalty(alpha, d, dv0 + j - (N - 1));
    }
    int hq[L], t[L];
    const uint16_t* me = min_ + ((size_t)excl * hw + q) * L;
#pragma unroll
    for (int i = 0; i < L; ++i) hq[i] = tot[i] - (int)me[i];
#pragma unroll
    for (int vq = 0; vq < N; ++vq)
#pragma unroll
      for (int u = 0; u < N; ++u) {
        int best = 0x7fffffff;
#pragma unroll
        for (int uq = 0; uq < N; ++uq) best = min(best, hq[vq * N + uq] + pu[u - uq + N - 1]);
        t[vq * N + u] = best;
      }
    int mn = 0x7fffffff;
#pragma unroll
    for (int v = 0; v < N; ++v)
#pragma unroll
      for (int u = 0; u < N; ++u) {
        int best = 0x7fffffff;
#pragma unroll
        for (int vq = 0; vq < N; ++vq) best = min(best, t[vq * N + u] + pv[v - vq + N - 1]);
        hq[v * N + u] = best;
        mn = min(mn, best);
      }
    uint16_t* dst = mout + ((size_t)slot * hw + p) * L;
#pragma unroll
    for (int i = 0; i < L; ++i) dst[i] = (uint16_t)(hq[i] - mn);
  }
}

// Any window: one pixel per wave, four pixels per workgroup, the label grids in LDS (3 x 441 ints per pixel, 20.7 KB in all).
// Every wave takes the same barriers; a wave without a pixel, or without the neighbour of the direction, idles through them.
constexpr int kBpWaves = 4;
__global__ void __launch_bounds__(256) sflow_bp_iter_lds_kernel(const uint16_t* __restrict__ cost, const uint16_t* __restrict__ min_,
                                                                uint16_t* __restrict__ mout, const int16_t* __restrict__ off,
                                                                int h, int w, int n, int alpha, int d) {
  __shared__ int s_tot[kBpWaves][kMaxLabels], s_h[kBpWaves][kMaxLabels], s_t[kBpWaves][kMaxLabels];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int L = n * n;
  const size_t hw = (size_t)h * w;
  const size_t q = (size_t)blockIdx.x * kBpWaves + wave;
  const bool valid = q < hw;
  const int y = valid ? (int)(q / w) : 0, x = valid ? (int)(q - (size_t)y * w) : 0;
  int* tot = s_tot[wave];
  int* hq = s_h[wave];
  int* t = s_t[wave];
  int ou = 0, ov = 0;
  if (valid) {
    ou = off[q];
    ov = off[hw + q];
    const uint16_t* c = cost + q * L;
    const uint16_t* m0 = min_ + q * L;
    for (int i = lane; i < L; i += 64)
      tot[i] = (int)c[i] + (int)m0[i] + (int)m0[hw * L + i] + (int)m0[2 * hw * L + i] + (int)m0[3 * hw * L + i];
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    int dy, dx, slot, excl;
    direction(k, &dy, &dx, &slot, &excl);
    const int py = y + dy, px = x + dx;
    const bool act = valid && py >= 0 && py < h && px >= 0 && px < w;
    const size_t p = act ? (size_t)py * w + px : 0;
    int du0 = 0, dv0 = 0;
    if (act) {
      du0 = (int)off[p] - ou;
      dv0 = (int)off[hw + p] - ov;
      const uint16_t* me = min_ + ((size_t)excl * hw + q) * L;
      for (int i = lane; i < L; i += 64) hq[i] = tot[i] - (int)me[i];
    }
    __syncthreads();
    if (act)
      for (int i = lane; i < L; i += 64) {
        const int vq = i / n, u = i - vq * n;
        t[i] = minconv_u(hq, n, vq, u, du0, alpha, d);
      }
    __syncthreads();
    int mn = 0x7fffffff;
    if (act)
      for (int i = lane; i < L; i += 64) {
        const int v = i / n, u = i - v * n;
        const int o = minconv_v(t, n, v, u, dv0, alpha, d);
        hq[i] = o;                      // read back below by this lane only
        mn = min(mn, o);
      }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mn = min(mn, __shfl_xor(mn, s, 64));
    if (act) {
      uint16_t* dst = mout + ((size_t)slot * hw + p) * L;
      for (int i = lane; i < L; i += 64) dst[i] = (uint16_t)(hq[i] - mn);
    }
    __syncthreads();                    // the next direction overwrites hq and t
  }
}

// ---------------------------------------------------------------- argmin and LD ---------------------------------------------
// One pixel per thread, 256 consecutive pixels (row-major) per workgroup.  partials[block] = the block's sum of flow lengths:
// a butterfly inside each wave, then the four waves in order.
__global__ void __launch_bounds__(kSelBlock) sflow_select_kernel(const uint16_t* __restrict__ cost, const uint16_t* __restrict__ msg,
                                                                 const int16_t* __restrict__ off, int h, int w, int win,
                                                                 int16_t* __restrict__ flow, double* __restrict__ partials) {
  __shared__ double red[kSelBlock / 64];
  const size_t hw = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * kSelBlock + threadIdx.x;
  const int n = 2 * win + 1, L = n * n;
  double len = 0.0;
  if (p < hw) {
    const uint16_t* c = cost + p * L;
    const uint16_t* m = msg + p * L;
    int best = 0x7fffffff, arg = 0;
    for (int i = 0; i < L; ++i) {
      const int b = (int)c[i] + (int)m[i] + (int)m[hw * L + i] + (int)m[2 * hw * L + i] + (int)m[3 * hw * L + i];
      if (b < best) { best = b; arg = i; }
    }
    const int lv = arg / n, lu = arg - lv * n;
    const int fu = (int)off[p] + lu - win, fv = (int)off[hw + p] + lv - win;
    flow[p] = (int16_t)fu;
    flow[hw + p] = (int16_t)fv;
    len = flow_length(fu, fv);
  }
  len = wave_sum(len);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = len;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup: lane t adds partials t, t + 256, ... in order, then a tree over the 256 lanes; *out = sum / count
__global__ void __launch_bounds__(kFinThreads) sflow_finalize_kernel(const double* __restrict__ partials, int blocks, double count,
                                                                     double* __restrict__ out) {
  __shared__ double red[kFinThreads];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int t = tid; t < blocks; t += kFinThreads) a += partials[t];
  red[tid] = a;
  __syncthreads();
  for (int s = kFinThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) *out = red[0] / count;
}

// ---------------------------------------------------------------- host side -------------------------------------------------
static void dsift_launch_u8(const uint8_t* img, int n, int h, int w, int eps, uint8_t* out, hipStream_t st) {
  sflow_dsift_kernel<uint8_t><<<dim3(cdiv(w, kDsTile), cdiv(h, kDsTile), n), 256, 0, st>>>(img, h, w, eps, out);
}

static void cost_launch(const uint8_t* da, const uint8_t* db, const int16_t* off, int h, int w, int win,
                        const dvd_sflow_params& pr, uint16_t* cost, hipStream_t st) {
  sflow_cost_kernel<<<dim3(cdiv((long)h * w, 256), 2 * win + 1), 256, 0, st>>>(da, db, off, h, w, win, pr.gamma, pr.T, cost);
}

// one level's workspace, as offsets: the cost volume, two message buffers (one behind the other), the LD partials
struct LevelWork {
  size_t cost, msg[2], partials, total;
};

static LevelWork level_work(int h, int w, int win) {
  const size_t L = (size_t)(2 * win + 1) * (2 * win + 1), hw = (size_t)h * w;
  LevelWork lw;
  Carver c;
  lw.cost = c.take(hw * L * sizeof(uint16_t));
  for (int s = 0; s < 2; ++s) lw.msg[s] = c.take(4 * hw * L * sizeof(uint16_t));
  lw.partials = c.take((size_t)cdiv((long)hw, kSelBlock) * sizeof(double));
  lw.total = c.at;
  return lw;
}

// cost, BP and the argmin of one level of one document; ld_out may be null
static void level_launch(const uint8_t* da, const uint8_t* db, const int16_t* off, int h, int w, int win, int iters,
                         const dvd_sflow_params& pr, void* workspace, int16_t* flow, double* ld_out, hipStream_t st) {
  const LevelWork lw = level_work(h, w, win);
  char* base = (char*)workspace;
  uint16_t* cost = (uint16_t*)(base + lw.cost);
  uint16_t* msg[2] = {(uint16_t*)(base + lw.msg[0]), (uint16_t*)(base + lw.msg[1])};
  double* partials = (double*)(base + lw.partials);
  const long hw = (long)h * w;
  cost_launch(da, db, off, h, w, win, pr, cost, st);
  (void)hipMemsetAsync(msg[0], 0, lw.partials - lw.msg[0], st);   // both message buffers
  for (int it = 0; it < iters; ++it) {
    const uint16_t* in = msg[it & 1];
    uint16_t* out = msg[(it + 1) & 1];
    if (win == 2)
      sflow_bp_iter_reg_kernel<5><<<cdiv(hw, 256), 256, 0, st>>>(cost, in, out, off, h, w, pr.alpha, pr.d);
    else
      sflow_bp_iter_lds_kernel<<<cdiv(hw, kBpWaves), 256, 0, st>>>(cost, in, out, off, h, w, 2 * win + 1, pr.alpha, pr.d);
  }
  const int blocks = cdiv(hw, kSelBlock);
  sflow_select_kernel<<<blocks, kSelBlock, 0, st>>>(cost, msg[iters & 1], off, h, w, win, flow, partials);
  if (ld_out) sflow_finalize_kernel<<<1, kFinThreads, 0, st>>>(partials, blocks, (double)hw, ld_out);
}

// The whole chain's workspace, for ONE document (the documents of a batch follow each other in it):
//   planes     2 sum_l h_l w_l                      u8 planes of both images on every level
//   desc       2 * 128 h_0 w_0                      descriptors of both images, one level at a time
//   off, flow  3 * 2 * 2 h_0 w_0                    window centres and two flow fields (coarser, current) as int16
//   level      max_l (1 + 8) * 2 h_l w_l L_l + 8 ceil(h_l w_l / 256)    cost volume, two message buffers, LD partials
struct ChainWork {
  size_t plane[kMaxLevels][2], desc[2], off, flow[2], level, total;
};

static ChainWork chain_work(int h, int w, const dvd_sflow_params& pr) {
  const LevelDims dm = level_dims(h, w, pr.levels);
  ChainWork cw;
  Carver c;
  for (int l = 0; l < pr.levels; ++l)
    for (int s = 0; s < 2; ++s) cw.plane[l][s] = c.take((size_t)dm.h[l] * dm.w[l]);
  for (int s = 0; s < 2; ++s) cw.desc[s] = c.take((size_t)h * w * kDesc);
  cw.off = c.take((size_t)h * w * 2 * sizeof(int16_t));
  for (int s = 0; s < 2; ++s) cw.flow[s] = c.take((size_t)h * w * 2 * sizeof(int16_t));
  size_t lvl = 0;
  for (int l = 0; l < pr.levels; ++l) {
    const size_t t = level_work(dm.h[l], dm.w[l], level_win(pr, l)).total;
    lvl = t > lvl ? t : lvl;
  }
  cw.level = c.take(lvl);
  cw.total = c.at;
  return cw;
}

// the whole chain of one document: planes to u8, the pyramid, then coarse to fine
static void chain_launch(const float* a, const float* b, int h, int w, const dvd_sflow_params& pr, const ChainWork& cw, char* base,
                         int16_t* flow, double* ld, hipStream_t st) {
  const LevelDims dm = level_dims(h, w, pr.levels);
  const size_t hw = (size_t)h * w;
  uint8_t* plane[kMaxLevels][2];
  for (int l = 0; l < pr.levels; ++l)
    for (int s = 0; s < 2; ++s) plane[l][s] = (uint8_t*)(base + cw.plane[l][s]);
  sflow_prep_kernel<<<cdiv((long)hw, 256), 256, 0, st>>>(a, plane[0][0], hw);
  sflow_prep_kernel<<<cdiv((long)hw, 256), 256, 0, st>>>(b, plane[0][1], hw);
  for (int l = 1; l < pr.levels; ++l)
    sflow_reduce2_kernel<<<dim3(cdiv(dm.w[l], 256), dm.h[l]), 256, 0, st>>>(plane[l - 1][0], plane[l - 1][1], plane[l][0],
                                                                            plane[l][1], dm.h[l - 1], dm.w[l - 1], dm.h[l], dm.w[l]);
  uint8_t* da = (uint8_t*)(base + cw.desc[0]);
  uint8_t* db = (uint8_t*)(base + cw.desc[1]);
  int16_t* off = (int16_t*)(base + cw.off);
  int16_t* coarse = nullptr;
  for (int l = pr.levels - 1; l >= 0; --l) {
    const int lh = dm.h[l], lw_ = dm.w[l];
    dsift_launch_u8(plane[l][0], 1, lh, lw_, pr.eps, da, st);
    dsift_launch_u8(plane[l][1], 1, lh, lw_, pr.eps, db, st);
    if (coarse)
      sflow_offsets_kernel<<<dim3(cdiv(lw_, 256), lh), 256, 0, st>>>(coarse, dm.h[l + 1], dm.w[l + 1], off, lh, lw_);
    else
      (void)hipMemsetAsync(off, 0, (size_t)lh * lw_ * 2 * sizeof(int16_t), st);
    int16_t* cur = l == 0 ? flow : (int16_t*)(base + cw.flow[l & 1]);
    level_launch(da, db, off, lh, lw_, level_win(pr, l), level_iters(pr, l), pr, base + cw.level, cur, l == 0 ? ld : nullptr, st);
    coarse = cur;
  }
}

static bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace sf
}  // namespace dvd

using namespace dvd;
using namespace dvd::sf;

extern "C" int dvd_dsift_u8(const float* gray, int n, int h, int w, int eps, uint8_t* out, void* stream) {
  DVD_REQUIRE(gray && out, "dsift_u8: null pointer");
  DVD_REQUIRE(n >= 1 && n <= 65535, "dsift_u8: bad batch %d", n);
  DVD_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "dsift_u8: bad shape %dx%d (each side 1..8192)", h, w);
  DVD_REQUIRE(eps >= 1 && eps <= (1 << 30), "dsift_u8: eps %d outside 1..2^30", eps);
  DVD_REQUIRE(aligned(out, 16), "dsift_u8: out must be 16-byte aligned");
  sflow_dsift_kernel<float><<<dim3(cdiv(w, kDsTile), cdiv(h, kDsTile), n), 256, 0, (hipStream_t)stream>>>(gray, h, w, eps, out);
  return check_launch("dsift_u8");
}

static int check_level_args(const char* what, const void* da, const void* db, const void* off, int h, int w, int win,
                            const dvd_sflow_params* params) {
  DVD_REQUIRE(da && db && off && params, "%s: null pointer", what);
  DVD_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "%s: bad shape %dx%d (each side 1..8192)", what, h, w);
  DVD_REQUIRE(win >= 1 && win <= kMaxWin, "%s: window %d outside 1..10", what, win);
  const char* why = check_params(*params);
  DVD_REQUIRE(!why, "%s: %s", what, why);
  DVD_REQUIRE(aligned(da, 16) && aligned(db, 16), "%s: descriptors must be 16-byte aligned", what);
  return DVD_OK;
}

extern "C" int dvd_sflow_cost(const uint8_t* desc_a, const uint8_t* desc_b, const int16_t* off, int h, int w, int win,
                              const dvd_sflow_params* params, uint16_t* cost, void* stream) {
  if (int e = check_level_args("sflow_cost", desc_a, desc_b, off, h, w, win, params)) return e;
  DVD_REQUIRE(cost, "sflow_cost: null pointer");
  cost_launch(desc_a, desc_b, off, h, w, win, *params, cost, (hipStream_t)stream);
  return check_launch("sflow_cost");
}

extern "C" long dvd_sflow_level_workspace_bytes(int h, int w, int win) {
  if (h < 1 || w < 1 || h > kMaxSide || w > kMaxSide || win < 1 || win > kMaxWin) {
    set_error("sflow_level_workspace_bytes: bad shape %dx%d (each side 1..8192) or window %d (1..10)", h, w, win);
    return DVD_E_ARG;
  }
  return (long)level_work(h, w, win).total;
}

extern "C" int dvd_sflow_level(const uint8_t* desc_a, const uint8_t* desc_b, const int16_t* off, int h, int w, int win,
                               int iters, const dvd_sflow_params* params, void* workspace, int16_t* flow, double* ld_out,
                               void* stream) {
  if (int e = check_level_args("sflow_level", desc_a, desc_b, off, h, w, win, params)) return e;
  DVD_REQUIRE(workspace && flow, "sflow_level: null pointer");
  DVD_REQUIRE(iters >= 1 && iters <= kMaxIters, "sflow_level: iterations %d outside 1..1000", iters);
  DVD_REQUIRE(aligned(workspace, 256), "sflow_level: workspace must be 256-byte aligned");
  level_launch(desc_a, desc_b, off, h, w, win, iters, *params, workspace, flow, ld_out, (hipStream_t)stream);
  return check_launch("sflow_level");
}

extern "C" long dvd_sflow_workspace_bytes(int h, int w, const dvd_sflow_params* params) {
  if (!params) {
    set_error("sflow_workspace_bytes: null pointer");
    return DVD_E_ARG;
  }
  const char* why = check_params(*params);
  if (!why) why = check_shape(h, w, *params);
  if (why) {
    set_error("sflow_workspace_bytes: %dx%d: %s", h, w, why);
    return DVD_E_ARG;
  }
  return (long)chain_work(h, w, *params).total;
}

extern "C" int dvd_sflow(const float* a, const float* b, int n, int h, int w, const dvd_sflow_params* params, void* workspace,
                         int16_t* flow, double* ld, void* stream) {
  DVD_REQUIRE(a && b && params && workspace && flow && ld, "sflow: null pointer");
  DVD_REQUIRE(n >= 1 && n <= 65535, "sflow: bad batch %d", n);
  const char* why = check_params(*params);
  if (!why) why = check_shape(h, w, *params);
  DVD_REQUIRE(!why, "sflow: %dx%d: %s", h, w, why);
  DVD_REQUIRE(aligned(workspace, 256), "sflow: workspace must be 256-byte aligned");
  const ChainWork cw = chain_work(h, w, *params);
  const size_t hw = (size_t)h * w;
  for (int doc = 0; doc < n; ++doc) {
    chain_launch(a + doc * hw, b + doc * hw, h, w, *params, cw, (char*)workspace, flow + doc * 2 * hw, ld + doc,
                 (hipStream_t)stream);
    if (int e = check_launch("sflow")) return e;
  }
  return DVD_OK;
}

// ================================================================ aligned distortion ========================================
// AD (tests/adist_model.py; the arithmetic: adist_core.h): the chain above from the scan A to the page B,
// a least-squares translation and scale per axis fitted to that field, B resampled through the fit, the chain again from A to
// the resampled page, and the mean of the second field's lengths weighted by A's gradient magnitude.  The coefficients stay
// on the device between the two flows.  All three stages move a few bytes per pixel and are launch-bound.
namespace dvd {
namespace sf {

// ---------------------------------------------------------------- fit -------------------------------------------------------
// 256 consecutive pixels per workgroup -> partials[block][4] = (sum f_u, sum X f_u, sum f_v, sum Y f_v), exact in int64
__global__ void __launch_bounds__(kSelBlock) ad_fit_kernel(const int16_t* __restrict__ flow, int h, int w,
                                                           int64_t* __restrict__ partials) {
  __shared__ long long red[kSelBlock / 64][4];
  const size_t hw = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * kSelBlock + threadIdx.x;
  long long s[4] = {0, 0, 0, 0};
  if (p < hw) {
    const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
    const int fu = flow[p], fv = flow[hw + p];
    s[0] = fu;
    s[1] = (long long)ad::centred(x, w) * fu;
    s[2] = fv;
    s[3] = (long long)ad::centred(y, h) * fv;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s[k] = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    partials[(size_t)blockIdx.x * 4 + k] = (int64_t)(red[0][k] + red[1][k] + red[2][k] + red[3][k]);
  }
}

// one workgroup: the four sums, then the four Q16 coefficients
__global__ void __launch_bounds__(kFinThreads) ad_fit_finalize_kernel(const int64_t* __restrict__ partials, int blocks, int h, int w,
                                                                      int64_t* __restrict__ sums, int32_t* __restrict__ coef) {
  __shared__ int64_t red[4][kFinThreads];
  const int tid = threadIdx.x;
  int64_t a[4] = {0, 0, 0, 0};
  for (int t = tid; t < blocks; t += kFinThreads)
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += partials[(size_t)t * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][tid] = a[k];
  __syncthreads();
  for (int s = kFinThreads / 2; s >= 1; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    int64_t sm[4];
    int32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sm[k] = red[k][0];
    ad::fit_coefs(sm, h, w, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sums[k] = sm[k];
      coef[k] = c[k];
    }
  }
}

// ---------------------------------------------------------------- align -----------------------------------------------------
// one lane per output pixel; the coefficients come from device memory (the fit's output: no read-back between the flows)
__global__ void __launch_bounds__(256) ad_align_kernel(const float* __restrict__ b, const int32_t* __restrict__ coef, int h, int w,
                                                       float* __restrict__ out) {
  const size_t hw = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int32_t c[4] = {coef[0], coef[1], coef[2], coef[3]};
  const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
  out[p] = (float)ad::aligned_at(b, h, w, y, x, c);
}

// ---------------------------------------------------------------- weighted mean ---------------------------------------------
// 256 consecutive pixels per workgroup -> one partial each of g |f| and |f| (f64, in the order of sflow_select: a butterfly
// inside each wave, then the four waves in order) and of g (int64)
__global__ void __launch_bounds__(kSelBlock) ad_weighted_kernel(const float* __restrict__ a, const int16_t* __restrict__ flow, int h,
                                                                int w, double* __restrict__ wpart, double* __restrict__ lpart,
                                                                int64_t* __restrict__ gpart) {
  __shared__ double rw[kSelBlock / 64], rl[kSelBlock / 64];
  __shared__ int rg[kSelBlock / 64];
  const size_t hw = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * kSelBlock + threadIdx.x;
  double len = 0.0, term = 0.0;
  int g = 0;                                   // at most 360 per pixel: 256 of them stay far inside 32 bits
  if (p < hw) {
    const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
    g = ad::weight_at(a, h, w, y, x);
    len = ad::flow_len(flow[p], flow[hw + p]);
    term = ad::weighted_term(g, len);
  }
  term = wave_sum(term);
  len = wave_sum(len);
  g = wave_sum(g);
  if ((threadIdx.x & 63) == 0) {
    rw[threadIdx.x >> 6] = term;
    rl[threadIdx.x >> 6] = len;
    rg[threadIdx.x >> 6] = g;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    wpart[blockIdx.x] = ((rw[0] + rw[1]) + rw[2]) + rw[3];
    lpart[blockIdx.x] = ((rl[0] + rl[1]) + rl[2]) + rl[3];
    gpart[blockIdx.x] = (int64_t)rg[0] + rg[1] + rg[2] + rg[3];
  }
}

// one workgroup: lane t adds partials t, t + 256, ... in order, then a tree over the 256 lanes (sflow_finalize's order for the
// two f64 sums); *out = the weighted mean, or the plain mean when no pixel has a weight
__global__ void __launch_bounds__(kFinThreads) ad_weighted_finalize_kernel(const double* __restrict__ wpart,
                                                                           const double* __restrict__ lpart,
                                                                           const int64_t* __restrict__ gpart, int blocks, long count,
                                                                           double* __restrict__ out) {
  __shared__ double rw[kFinThreads], rl[kFinThreads];
  __shared__ int64_t rg[kFinThreads];
  const int tid = threadIdx.x;
  double aw = 0.0, al = 0.0;
  int64_t ag = 0;
  for (int t = tid; t < blocks; t += kFinThreads) {
    aw += wpart[t];
    al += lpart[t];
    ag += gpart[t];
  }
  rw[tid] = aw;
  rl[tid] = al;
  rg[tid] = ag;
  __syncthreads();
  for (int s = kFinThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) {
      rw[tid] += rw[tid + s];
      rl[tid] += rl[tid + s];
      rg[tid] += rg[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) *out = ad::ad_value(rw[0], rl[0], rg[0], (int64_t)count);
}

// ---------------------------------------------------------------- host side -------------------------------------------------
static void fit_launch(const int16_t* flow, int h, int w, void* scratch, int64_t* sums, int32_t* coef, hipStream_t st) {
  const int blocks = cdiv((long)h * w, kSelBlock);
  ad_fit_kernel<<<blocks, kSelBlock, 0, st>>>(flow, h, w, (int64_t*)scratch);
  ad_fit_finalize_kernel<<<1, kFinThreads, 0, st>>>((const int64_t*)scratch, blocks, h, w, sums, coef);
}

static void align_launch(const float* b, const int32_t* coef, int h, int w, float* out, hipStream_t st) {
  ad_align_kernel<<<cdiv((long)h * w, 256), 256, 0, st>>>(b, coef, h, w, out);
}

// scratch: blocks f64 of g |f|, blocks f64 of |f|, blocks int64 of g
static void weighted_launch(const float* a, const int16_t* flow, int h, int w, void* scratch, double* out, hipStream_t st) {
  const int blocks = cdiv((long)h * w, kSelBlock);
  double* wpart = (double*)scratch;
  double* lpart = wpart + blocks;
  int64_t* gpart = (int64_t*)(lpart + blocks);
  ad_weighted_kernel<<<blocks, kSelBlock, 0, st>>>(a, flow, h, w, wpart, lpart, gpart);
  ad_weighted_finalize_kernel<<<1, kFinThreads, 0, st>>>(wpart, lpart, gpart, blocks, (long)h * w, out);
}

// The AD chain's workspace, for ONE document: one SIFT-flow workspace (both passes), the resampled plane (f32), the two flows,
// the partials of the fit (32 bytes per 256 pixels; the weighted mean's 24 reuse them), sums, coefficients, pass 2's LD
struct AdWork {
  size_t chain, aligned, flow[2], partials, sums, coef, ld2, total;
};

static AdWork ad_work(int h, int w, const dvd_sflow_params& pr) {
  AdWork aw;
  const size_t hw = (size_t)h * w;
  Carver c;
  aw.chain = c.take(chain_work(h, w, pr).total);
  aw.aligned = c.take(hw * sizeof(float));
  for (int s = 0; s < 2; ++s) aw.flow[s] = c.take(hw * 2 * sizeof(int16_t));
  aw.partials = c.take((size_t)cdiv((long)hw, kSelBlock) * 4 * sizeof(int64_t));
  aw.sums = c.take(4 * sizeof(int64_t));
  aw.coef = c.take(4 * sizeof(int32_t));
  aw.ld2 = c.take(sizeof(double));
  aw.total = c.at;
  return aw;
}

static int check_plane_args(const char* what, int n, int h, int w) {
  DVD_REQUIRE(n >= 1 && n <= 65535, "%s: bad batch %d", what, n);
  DVD_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "%s: bad shape %dx%d (each side 1..8192)", what, h, w);
  return DVD_OK;
}

}  // namespace sf
}  // namespace dvd

extern "C" int dvd_ad_fit(const int16_t* flow, int n, int h, int w, void* scratch, int64_t* sums, int32_t* coef, void* stream) {
  DVD_REQUIRE(flow && scratch && sums && coef, "ad_fit: null pointer");
  if (int e = check_plane_args("ad_fit", n, h, w)) return e;
  DVD_REQUIRE(aligned(scratch, 8) && aligned(sums, 8) && aligned(coef, 4) && aligned(flow, 2), "ad_fit: misaligned pointer");
  const size_t hw = (size_t)h * w;
  for (int doc = 0; doc < n; ++doc) fit_launch(flow + doc * 2 * hw, h, w, scratch, sums + 4 * doc, coef + 4 * doc, (hipStream_t)stream);
  return check_launch("ad_fit");
}

extern "C" int dvd_ad_align(const float* b, const int32_t* coef, int n, int h, int w, float* out, void* stream) {
  DVD_REQUIRE(b && coef && out, "ad_align: null pointer");
  if (int e = check_plane_args("ad_align", n, h, w)) return e;
  DVD_REQUIRE(aligned(b, 4) && aligned(coef, 4) && aligned(out, 4), "ad_align: misaligned pointer");
  DVD_REQUIRE(b != out, "ad_align: out must not be b");
  const size_t hw = (size_t)h * w;
  for (int doc = 0; doc < n; ++doc) align_launch(b + doc * hw, coef + 4 * doc, h, w, out + doc * hw, (hipStream_t)stream);
  return check_launch("ad_align");
}

extern "C" int dvd_ad_weighted(const float* a, const int16_t* flow, int n, int h, int w, void* scratch, double* ad, void* stream) {
  DVD_REQUIRE(a && flow && scratch && ad, "ad_weighted: null pointer");
  if (int e = check_plane_args("ad_weighted", n, h, w)) return e;
  DVD_REQUIRE(aligned(scratch, 8) && aligned(ad, 8) && aligned(a, 4) && aligned(flow, 2), "ad_weighted: misaligned pointer");
  const size_t hw = (size_t)h * w;
  for (int doc = 0; doc < n; ++doc) weighted_launch(a + doc * hw, flow + doc * 2 * hw, h, w, scratch, ad + doc, (hipStream_t)stream);
  return check_launch("ad_weighted");
}

extern "C" long dvd_adist_workspace_bytes(int h, int w, const dvd_sflow_params* params) {
  if (!params) {
    set_error("adist_workspace_bytes: null pointer");
    return DVD_E_ARG;
  }
  const char* why = check_params(*params);
  if (!why) why = check_shape(h, w, *params);
  if (why) {
    set_error("adist_workspace_bytes: %dx%d: %s", h, w, why);
    return DVD_E_ARG;
  }
  return (long)ad_work(h, w, *params).total;
}

extern "C" int dvd_adist(const float* a, const float* b, int n, int h, int w, const dvd_sflow_params* params, void* workspace,
                         double* ld, double* ad, int16_t* flow1, int64_t* sums, int32_t* coef, float* aligned_out, int16_t* flow2,
                         void* stream) {
  DVD_REQUIRE(a && b && params && workspace && ld && ad, "adist: null pointer");
  DVD_REQUIRE(n >= 1 && n <= 65535, "adist: bad batch %d", n);
  const char* why = check_params(*params);
  if (!why) why = check_shape(h, w, *params);
  DVD_REQUIRE(!why, "adist: %dx%d: %s", h, w, why);
  DVD_REQUIRE(aligned(workspace, 256), "adist: workspace must be 256-byte aligned");
  DVD_REQUIRE(aligned(ld, 8) && aligned(ad, 8) && aligned(sums, 8) && aligned(coef, 4) && aligned(aligned_out, 4) &&
                  aligned(flow1, 2) && aligned(flow2, 2), "adist: misaligned output pointer");
  hipStream_t st = (hipStream_t)stream;
  const dvd_sflow_params& pr = *params;
  const ChainWork cw = chain_work(h, w, pr);
  const AdWork aw = ad_work(h, w, pr);
  char* base = (char*)workspace;
  const size_t hw = (size_t)h * w;
  for (int doc = 0; doc < n; ++doc) {
    const float* ad_ = a + doc * hw;
    const float* bd = b + doc * hw;
    int16_t* f1 = flow1 ? flow1 + doc * 2 * hw : (int16_t*)(base + aw.flow[0]);
    int16_t* f2 = flow2 ? flow2 + doc * 2 * hw : (int16_t*)(base + aw.flow[1]);
    int64_t* sm = sums ? sums + 4 * doc : (int64_t*)(base + aw.sums);
    int32_t* cf = coef ? coef + 4 * doc : (int32_t*)(base + aw.coef);
    float* bp = aligned_out ? aligned_out + doc * hw : (float*)(base + aw.aligned);
    chain_launch(ad_, bd, h, w, pr, cw, base + aw.chain, f1, ld + doc, st);
    fit_launch(f1, h, w, base + aw.partials, sm, cf, st);
    align_launch(bd, cf, h, w, bp, st);
    chain_launch(ad_, bp, h, w, pr, cw, base + aw.chain, f2, (double*)(base + aw.ld2), st);
    weighted_launch(ad_, f2, h, w, base + aw.partials, ad + doc, st);
    if (int e = check_launch("adist")) return e;
  }
  return DVD_OK;
}
