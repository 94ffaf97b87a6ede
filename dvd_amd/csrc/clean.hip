// Scan-like pages: the paper estimate of a page, the page flattened by it, and Sauvola's black-and-white
// plane.  The arithmetic is clean_core.h's; tests/clean_model.py restates it.  All integers: any order of sums and maxima.
//   page_cellmax_kernel   a workgroup owns one row of cells and 256 page columns of it; a lane reads four pixels of a row as
//                         three dwords (single bytes where the row does not begin on one), keeps three maxima over its share of
//                         the rows, and the lanes of a cell meet in LDS: one byte per (channel, cell)
//   page_bg_kernel        a workgroup owns 16 x 16 cells; per channel an LDS tile with a halo of 2 close + smooth cells goes
//                         through the closing's two separable maxima and two separable minima (windows clipped to the plane:
//                         a cell off the plane is 0 under the maximum and 255 under the minimum) and the tent's two passes
//   page_flatten_kernel   a workgroup owns 64 x 16 page pixels; the column and row terms and the cells of bg the tile touches go
//                         to LDS once; a lane flattens four pixels (twelve 32-bit divisions) and stores them as dwords; optionally
//                         the gray plane of what it stored; counts as block partials and one atomic each
//   page_binarize_kernel  a workgroup owns 64 x 64 page pixels; the gray tile and its halo of `radius` sit in LDS as bytes
//                         (dynamic, sized by the radius); one thread per tile column slides the vertical window sums of g and
//                         g^2 down the tile, sixteen rows at a time into LDS; a lane slides the horizontal window over them for
//                         its four pixels, decides, and stores a dword
// No scratch memory.
#include "common.h"
#include "clean_core.h"
#include "hwc_bytes.h"
#include "workspace.h"

namespace dvd {
namespace cl {

constexpr int kCellTile = kBlock;              // page columns of a cell-maximum workgroup: 64 lanes x 4 pixels
constexpr int kBgT = 16;                       // cells of a background workgroup, per side
constexpr int kBgE = kBgT + 2 * (2 * kMaxClose + kMaxSmooth);   // its LDS tile with the largest halo, per side: 64
constexpr int kBinH = 64;                      // page rows of a binarise workgroup: four passes of kTileH

// four bytes to p, which may begin anywhere
__device__ __forceinline__ void store4(uint8_t* __restrict__ p, uint32_t d) {
  if (((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = d;
  } else {
    for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(d >> (8 * k));
  }
}

__global__ __launch_bounds__(kBlock) void page_cellmax_kernel(const uint8_t* __restrict__ img, int h, int w, int s, int hc, int wc,
                                                              uint8_t* __restrict__ cmax) {
  __shared__ unsigned m[3 * 64];                           // [channel][cell of the tile]: at most 256 / 4 cells
  const int t = threadIdx.x, lane = t & 63, wy = t >> 6;
  if (t < 3 * 64) m[t] = 0;
  __syncthreads();
  const int j = blockIdx.y, xa = blockIdx.x * kCellTile + kPer * lane;
  const int y1 = (j + 1) * s < h ? (j + 1) * s : h;
  if (xa < w) {
    const int npix = w - xa < kPer ? w - xa : kPer;
    uint32_t mx[3] = {0, 0, 0};
    for (int y = j * s + wy; y < y1; y += kBlock / 64) {
      const uint8_t* p = img + 3 * ((size_t)y * w + xa);
      if (npix == kPer) {
        uint32_t d0, d1, d2;
        load12(p, d0, d1, d2);
#pragma unroll
        for (int k = 0; k < 12; ++k) {
          const uint32_t v = byte12(d0, d1, d2, k);
          mx[k % 3] = mx[k % 3] > v ? mx[k % 3] : v;
        }
      } else {
        for (int k = 0; k < 3 * npix; ++k) {
          const uint32_t v = p[k];
          mx[k % 3] = mx[k % 3] > v ? mx[k % 3] : v;
        }
      }
    }
    const int cell = (kPer * lane) >> log2_of(s);          // s is a multiple of 4: a lane's four pixels share a cell
    for (int c = 0; c < 3; ++c) atomicMax(&m[c * 64 + cell], mx[c]);
  }
  __syncthreads();
  const int ncell = kCellTile >> log2_of(s);
  if (t < 3 * ncell) {
    const int c = t / ncell, i = t - c * ncell, gi = blockIdx.x * ncell + i;
    if (gi < wc) cmax[((size_t)c * hc + j) * wc + gi] = (uint8_t)m[c * 64 + i];
  }
}

// dst[y][x] = the maximum (MAX) or minimum of src[y][x .. x + 2k] (ALONG_X) or src[y .. y + 2k][x], for y < rows, x < cols;
// both tiles have the pitch kBgE.  OFF: the value of a cell off the plane afterwards; (gy0, gx0) is the plane position of dst[0][0].
template <bool MAX, bool ALONG_X>
__device__ __forceinline__ void morph_pass(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int cols, int k, int gy0,
                                           int gx0, int hc, int wc, int off) {
  for (int i = threadIdx.x; i < rows * cols; i += kBlock) {
    const int y = i / cols, x = i - y * cols;
    const uint8_t* p = src + y * kBgE + x;
    int v = p[0];
    for (int d = 1; d <= 2 * k; ++d) {
      const int q = p[ALONG_X ? d : d * kBgE];
      v = MAX ? (v > q ? v : q) : (v < q ? v : q);
    }
    const int gy = gy0 + y, gx = gx0 + x;
    dst[y * kBgE + x] = (uint8_t)(gy >= 0 && gy < hc && gx >= 0 && gx < wc ? v : off);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void page_bg_kernel(const uint8_t* __restrict__ cmax, int hc, int wc, int k, int b, int neutral,
                                                         uint8_t* __restrict__ bg) {
  __shared__ uint8_t ta[kBgE * kBgE], tb[kBgE * kBgE];
  __shared__ uint32_t tn[(kBgT + 2 * kMaxSmooth) * kBgT];  // the tent's first pass: [row of the haloed tile][column]
  __shared__ uint8_t res[3 * kBgT * kBgT];
  const int t = threadIdx.x, x0 = blockIdx.x * kBgT, y0 = blockIdx.y * kBgT;
  const int e0 = kBgT + 2 * (2 * k + b), e1 = kBgT + 2 * (k + b), e2 = kBgT + 2 * b;
  const int ty = t / kBgT, tx = t - ty * kBgT, gy = y0 + ty, gx = x0 + tx;
  for (int c = 0; c < 3; ++c) {
    const uint8_t* plane = cmax + (size_t)c * hc * wc;
    for (int i = t; i < e0 * e0; i += kBlock) {
      const int y = i / e0, x = i - y * e0, py = y0 - (2 * k + b) + y, px = x0 - (2 * k + b) + x;
      ta[y * kBgE + x] = py >= 0 && py < hc && px >= 0 && px < wc ? plane[(size_t)py * wc + px] : (uint8_t)0;
    }
    __syncthreads();
    morph_pass<true, true>(ta, tb, e0, e1, k, y0 - (2 * k + b), x0 - (k + b), hc, wc, 0);
    morph_pass<true, false>(tb, ta, e1, e1, k, y0 - (k + b), x0 - (k + b), hc, wc, 255);
    morph_pass<false, true>(ta, tb, e1, e2, k, y0 - (k + b), x0 - b, hc, wc, 255);
    morph_pass<false, false>(tb, ta, e2, e2, k, y0 - b, x0 - b, hc, wc, 0);
    for (int i = t; i < e2 * kBgT; i += kBlock) {          // the tent along x: a cell off the plane has no weight
      const int y = i / kBgT, x = i - y * kBgT;
      uint32_t num = 0;
      for (int d = -b; d <= b; ++d) {
        const int px = x0 + x + d;
        if (px >= 0 && px < wc) num += tent_w(d, b) * ta[y * kBgE + x + b + d];
      }
      tn[i] = num;
    }
    __syncthreads();
    if (gy < hc && gx < wc) {                              // and along y
      uint32_t num = 0;
      for (int d = -b; d <= b; ++d) {
        const int py = gy + d;
        if (py >= 0 && py < hc) num += tent_w(d, b) * tn[(ty + b + d) * kBgT + tx];
      }
      res[c * kBgT * kBgT + t] = (uint8_t)bg_round(num, tent_den(gx, wc, b) * tent_den(gy, hc, b));
    }
    __syncthreads();
  }
  if (gy < hc && gx < wc) {
    const uint32_t r = res[t], g = res[kBgT * kBgT + t], bl = res[2 * kBgT * kBgT + t], m = gray_of(r, g, bl);
    bg[(size_t)gy * wc + gx] = (uint8_t)(neutral ? r : m);
    bg[((size_t)hc + gy) * wc + gx] = (uint8_t)(neutral ? g : m);
    bg[((size_t)2 * hc + gy) * wc + gx] = (uint8_t)(neutral ? bl : m);
  }
}

constexpr int kFlatCx = kTileW / 4 + 2, kFlatCy = kTileH / 4 + 2;   // the cells of bg a tile touches at s = 4: 18 x 6

__global__ __launch_bounds__(kBlock) void page_flatten_kernel(const uint8_t* __restrict__ img, int h, int w, const uint8_t* __restrict__ bg,
                                                              int hc, int wc, int s, int white, uint8_t* __restrict__ out,
                                                              uint8_t* __restrict__ gray, unsigned long long* __restrict__ stats) {
  __shared__ Axis xt[kTileW], yt[kTileH];
  __shared__ uint8_t bt[3 * kFlatCy * kFlatCx];
  __shared__ unsigned cnt[2];
  const int t = threadIdx.x, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  if (t < kTileW) xt[t] = flat_axis(x0 + t < w ? x0 + t : w - 1, s, wc);
  if (t >= 64 && t < 64 + kTileH) yt[t - 64] = flat_axis(y0 + t - 64 < h ? y0 + t - 64 : h - 1, s, hc);
  if (t >= 128 && t < 130) cnt[t - 128] = 0;
  __syncthreads();
  const int cx0 = xt[0].i0, ncx = xt[kTileW - 1].i1 - cx0 + 1, cy0 = yt[0].i0, ncy = yt[kTileH - 1].i1 - cy0 + 1;   // monotone terms
  for (int i = t; i < 3 * ncy * ncx; i += kBlock) {
    const int c = i / (ncy * ncx), rest = i - c * ncy * ncx, yy = rest / ncx, xx = rest - yy * ncx;
    bt[(c * kFlatCy + yy) * kFlatCx + xx] = bg[((size_t)c * hc + cy0 + yy) * wc + cx0 + xx];
  }
  __syncthreads();
  const int ly = t / (kTileW / kPer), lx = (t % (kTileW / kPer)) * kPer;
  const int y = y0 + ly, xa = x0 + lx;
  Counts n;
  n.saturated = n.floored = n.ink = 0;
  if (y < h && xa < w) {
    const int npix = w - xa < kPer ? w - xa : kPer;
    const uint8_t* src = img + 3 * ((size_t)y * w + xa);
    uint32_t d0 = 0, d1 = 0, d2 = 0;
    if (npix == kPer) {
      load12(src, d0, d1, d2);
    } else {
      for (int k = 0; k < 3 * npix; ++k) {                 // at most three pixels: nine bytes
        const uint32_t v = (uint32_t)src[k] << (8 * (k & 3));
        if (k < 4) d0 |= v;
        else if (k < 8) d1 |= v;
        else d2 |= v;
      }
    }
    const Axis ay = yt[ly];
    const int r0 = (ay.i0 - cy0) * kFlatCx - cx0, r1 = (ay.i1 - cy0) * kFlatCx - cx0;
    uint32_t o[12];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const Axis ax = xt[lx + k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int pc = c * kFlatCy * kFlatCx;
        const uint32_t q = bgq_of(bt[pc + r0 + ax.i0], bt[pc + r0 + ax.i1], bt[pc + r1 + ax.i0], bt[pc + r1 + ax.i1], ax.f, ay.f, s);
        Counts one;
        one.saturated = one.floored = one.ink = 0;
        o[3 * k + c] = flatten_sample(byte12(d0, d1, d2, 3 * k + c), (uint32_t)white, s, q, one);
        if (k < npix) {
          n.saturated += one.saturated;
          n.floored += one.floored;
        }
      }
    }
    uint8_t* dst = out + 3 * ((size_t)y * w + xa);
    uint32_t gq = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) gq |= gray_of(o[3 * k], o[3 * k + 1], o[3 * k + 2]) << (8 * k);
    if (npix == kPer) {
      store12(dst, o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24, o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24,
              o[8] | o[9] << 8 | o[10] << 16 | o[11] << 24);
      if (gray) store4(gray + (size_t)y * w + xa, gq);
    } else {
#pragma unroll
      for (int k = 0; k < kPer - 1; ++k)
        if (k < npix) {
          dst[3 * k] = (uint8_t)o[3 * k];
          dst[3 * k + 1] = (uint8_t)o[3 * k + 1];
          dst[3 * k + 2] = (uint8_t)o[3 * k + 2];
          if (gray) gray[(size_t)y * w + xa + k] = (uint8_t)(gq >> (8 * k));
        }
    }
  }
  if (stats) {                                             // uniform over the launch
    if (n.saturated) atomicAdd(&cnt[0], n.saturated);
    if (n.floored) atomicAdd(&cnt[1], n.floored);
    __syncthreads();
    if (t < 2 && cnt[t]) atomicAdd(&stats[t], (unsigned long long)cnt[t]);
  }
}

// the dynamic LDS of a binarise workgroup at radius r: the vertical sums of one pass (g^2 as u32, g as u16) and the gray tile
static size_t binarize_lds(int r) {
  const size_t p = kTileW + 2 * r;
  return kTileH * p * 6 + p * (kBinH + 2 * r);
}

template <int CH>
__global__ __launch_bounds__(kBlock) void page_binarize_kernel(const uint8_t* __restrict__ img, int h, int w, int r, int kq,
                                                               uint8_t* __restrict__ out, unsigned long long* __restrict__ ink) {
  extern __shared__ __align__(16) uint8_t lds[];
  __shared__ unsigned cnt;
  const int t = threadIdx.x, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kBinH;
  const int p = kTileW + 2 * r, rows = kBinH + 2 * r;      // the tile's pitch = its columns, and its rows
  uint32_t* cs2 = reinterpret_cast<uint32_t*>(lds);
  uint16_t* cs1 = reinterpret_cast<uint16_t*>(cs2 + kTileH * p);
  uint8_t* tile = reinterpret_cast<uint8_t*>(cs1 + kTileH * p);
  for (int i = t; i < rows * p; i += kBlock) {             // a pixel off the page is 0: it adds nothing to either sum
    const int ty = i / p, tx = i - ty * p, gy = y0 - r + ty, gx = x0 - r + tx;
    uint32_t v = 0;
    if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
      const uint8_t* q = img + CH * ((size_t)gy * w + gx);
      v = CH == 1 ? q[0] : gray_of(q[0], q[1], q[2]);
    }
    tile[i] = (uint8_t)v;
  }
  if (t == 0) cnt = 0;
  __syncthreads();
  uint32_t s1 = 0, s2 = 0;                                 // thread t < p: the window of the pass's next row in tile column t
  if (t < p)
    for (int j = 0; j <= 2 * r; ++j) {
      const uint32_t v = tile[j * p + t];
      s1 += v;
      s2 += v * v;
    }
  const int ly = t / (kTileW / kPer), lx = (t % (kTileW / kPer)) * kPer, xa = x0 + lx;
  unsigned n_ink = 0;
  for (int pass = 0; pass < kBinH / kTileH && y0 + pass * kTileH < h; ++pass) {     // the bound is the workgroup's
    if (t < p)
      for (int ry = 0; ry < kTileH; ++ry) {
        const int row = pass * kTileH + ry;                // the page row y0 + row: tile rows row .. row + 2r
        cs1[ry * p + t] = (uint16_t)s1;
        cs2[ry * p + t] = s2;
        if (row + 2 * r + 1 < rows) {
          const uint32_t in = tile[(row + 2 * r + 1) * p + t], gone = tile[row * p + t];
          s1 += in - gone;
          s2 += in * in - gone * gone;
        }
      }
    __syncthreads();
    const int y = y0 + pass * kTileH + ly;
    if (y < h && xa < w) {
      const uint16_t* c1 = cs1 + ly * p + lx;              // the page column xa + k: tile columns lx + k .. lx + k + 2r
      const uint32_t* c2 = cs2 + ly * p + lx;
      uint32_t a1 = 0, a2 = 0;
      for (int d = 0; d <= 2 * r; ++d) {
        a1 += c1[d];
        a2 += c2[d];
      }
      const uint32_t ny = (uint32_t)win_count(y, h, r);
      const uint8_t* gp = tile + (pass * kTileH + ly + r) * p + lx + r;
      uint32_t bytes = 0;
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        if (k > 0) {
          a1 += (uint32_t)c1[k + 2 * r] - c1[k - 1];
          a2 += c2[k + 2 * r] - c2[k - 1];
        }
        if (xa + k < w) {
          const bool is_ink = sauvola_ink(gp[k], ny * (uint32_t)win_count(xa + k, w, r), a1, a2, kq);
          n_ink += is_ink ? 1u : 0u;
          bytes |= (is_ink ? 0u : 255u) << (8 * k);
        }
      }
      uint8_t* dst = out + (size_t)y * w + xa;
      if (xa + kPer <= w) {
        store4(dst, bytes);
      } else {
        for (int k = 0; k < w - xa; ++k) dst[k] = (uint8_t)(bytes >> (8 * k));
      }
    }
    __syncthreads();
  }
  if (ink) {                                               // uniform over the launch
    if (n_ink) atomicAdd(&cnt, n_ink);
    __syncthreads();
    if (t == 0 && cnt) atomicAdd(ink, (unsigned long long)cnt);
  }
}

// the pieces of the workspace, in the order dvd_page_clean_workspace_bytes documents
struct Workspace {
  size_t coarse_bytes, cmax, bg, gray, total;
};
static Workspace workspace_of(int h, int w, int cell) {
  Carver c;
  Workspace ws;
  ws.coarse_bytes = 3 * (size_t)coarse(h, cell) * coarse(w, cell);
  ws.cmax = c.take(ws.coarse_bytes);
  ws.bg = c.take(ws.coarse_bytes);
  ws.gray = c.take((size_t)h * w);
  ws.total = c.at;
  return ws;
}

static int launch_background(const uint8_t* img, int h, int w, int cell, int close, int smooth, int neutral, uint8_t* cmax, uint8_t* bg,
                             hipStream_t stream) {
  const int hc = coarse(h, cell), wc = coarse(w, cell);
  page_cellmax_kernel<<<dim3((unsigned)cdiv(w, kCellTile), (unsigned)hc), kBlock, 0, stream>>>(img, h, w, cell, hc, wc, cmax);
  if (int e = check_launch("page_background")) return e;
  page_bg_kernel<<<dim3((unsigned)cdiv(wc, kBgT), (unsigned)cdiv(hc, kBgT)), kBlock, 0, stream>>>(cmax, hc, wc, close, smooth, neutral, bg);
  return check_launch("page_background");
}

static int launch_flatten(const uint8_t* img, int h, int w, const uint8_t* bg, int cell, int white, uint8_t* out, uint8_t* gray,
                          unsigned long long* stats, hipStream_t stream) {
  if (stats && hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), stream) != hipSuccess) return check_launch("page_flatten_rgb8");
  const dim3 grid((unsigned)cdiv(w, kTileW), (unsigned)cdiv(h, kTileH));
  page_flatten_kernel<<<grid, kBlock, 0, stream>>>(img, h, w, bg, coarse(h, cell), coarse(w, cell), cell, white, out, gray, stats);
  return check_launch("page_flatten_rgb8");
}

static int launch_binarize(const uint8_t* img, int channels, int h, int w, int radius, int kq, uint8_t* out, unsigned long long* ink,
                           hipStream_t stream) {
  if (ink && hipMemsetAsync(ink, 0, sizeof(unsigned long long), stream) != hipSuccess) return check_launch("page_binarize_u8");
  const dim3 grid((unsigned)cdiv(w, kTileW), (unsigned)cdiv(h, kBinH));
  if (channels == 1)
    page_binarize_kernel<1><<<grid, kBlock, binarize_lds(radius), stream>>>(img, h, w, radius, kq, out, ink);
  else
    page_binarize_kernel<3><<<grid, kBlock, binarize_lds(radius), stream>>>(img, h, w, radius, kq, out, ink);
  return check_launch("page_binarize_u8");
}

}  // namespace cl
}  // namespace dvd

using namespace dvd;

#define CLEAN_REQUIRE(cond, code, ...) \
  do {                                 \
    if (!(cond)) {                     \
      dvd::set_error(__VA_ARGS__);     \
      return code;                     \
    }                                  \
  } while (0)

#define CLEAN_CHECK_PAGE(name) \
  CLEAN_REQUIRE(cl::check_page(h, w) == DVD_OK, DVD_E_CLEAN_SHAPE, name ": page %d x %d: sides 1..%d", h, w, cl::kMaxSide)
#define CLEAN_CHECK_BACKGROUND(name)                                                                                                 \
  CLEAN_REQUIRE(cl::check_background(cell, close, smooth) == DVD_OK, DVD_E_CLEAN_PARAM, name ": cell = %d, close = %d, smooth = %d: " \
                "cell 4, 8, 16, 32 or 64, close 0..%d, smooth 0..%d", cell, close, smooth, cl::kMaxClose, cl::kMaxSmooth)
#define CLEAN_CHECK_FLATTEN(name)                                                                                                   \
  CLEAN_REQUIRE(cl::check_flatten(cell, white) == DVD_OK, DVD_E_CLEAN_PARAM, name ": cell = %d, white = %d: cell 4, 8, 16, 32 or 64, " \
                "white 1..255", cell, white)
#define CLEAN_CHECK_BINARIZE(name)                                                                                                 \
  CLEAN_REQUIRE(cl::check_binarize(radius, kq) == DVD_OK, DVD_E_CLEAN_PARAM, name ": radius = %d, kq = %d: radius 1..%d, kq 0..%d", \
                radius, kq, cl::kMaxRadius, cl::kMaxKq)

extern "C" long dvd_page_clean_workspace_bytes(int h, int w, int cell) {
  CLEAN_CHECK_PAGE("page_clean_workspace_bytes");
  CLEAN_REQUIRE(cl::cell_ok(cell), DVD_E_CLEAN_PARAM, "page_clean_workspace_bytes: cell = %d: 4, 8, 16, 32 or 64", cell);
  return (long)cl::workspace_of(h, w, cell).total;
}

extern "C" int dvd_page_background(const uint8_t* img, int h, int w, int cell, int close, int smooth, int neutral, uint8_t* bg, void* ws,
                                   void* stream) {
  CLEAN_CHECK_PAGE("page_background");
  CLEAN_CHECK_BACKGROUND("page_background");
  DVD_REQUIRE(img && bg && ws, "page_background: null pointer");
  const cl::Workspace lay = cl::workspace_of(h, w, cell);
  DVD_REQUIRE(!cl::bytes_overlap(bg, lay.coarse_bytes, img, 3 * (size_t)h * w) && !cl::bytes_overlap(ws, lay.total, img, 3 * (size_t)h * w),
              "page_background: bg and ws must share no byte with img");
  DVD_REQUIRE(!cl::bytes_overlap(bg, lay.coarse_bytes, ws, lay.coarse_bytes), "page_background: bg must not lie over the cell maxima at the head of ws");
  return cl::launch_background(img, h, w, cell, close, smooth, neutral, (uint8_t*)ws + lay.cmax, bg, (hipStream_t)stream);
}

extern "C" int dvd_page_flatten_rgb8(const uint8_t* img, int h, int w, const uint8_t* bg, int cell, int white, uint8_t* out, uint8_t* gray,
                                     unsigned long long* stats, void* stream) {
  CLEAN_CHECK_PAGE("page_flatten_rgb8");
  CLEAN_CHECK_FLATTEN("page_flatten_rgb8");
  DVD_REQUIRE(img && bg && out, "page_flatten_rgb8: null pointer");
  DVD_REQUIRE(((uintptr_t)stats & 7) == 0, "page_flatten_rgb8: misaligned stats");
  const size_t n = (size_t)h * w, nb = 3 * (size_t)cl::coarse(h, cell) * cl::coarse(w, cell);
  DVD_REQUIRE(!cl::bytes_overlap(out, 3 * n, img, 3 * n) && !cl::bytes_overlap(out, 3 * n, bg, nb) && !cl::bytes_overlap(gray, n, img, 3 * n) &&
                  !cl::bytes_overlap(gray, n, bg, nb) && !cl::bytes_overlap(gray, n, out, 3 * n),
              "page_flatten_rgb8: out and gray must share no byte with img, bg or each other");
  return cl::launch_flatten(img, h, w, bg, cell, white, out, gray, stats, (hipStream_t)stream);
}

extern "C" int dvd_page_binarize_u8(const uint8_t* img, int channels, int h, int w, int radius, int kq, uint8_t* out, unsigned long long* ink,
                                    void* stream) {
  CLEAN_CHECK_PAGE("page_binarize_u8");
  CLEAN_CHECK_BINARIZE("page_binarize_u8");
  DVD_REQUIRE(channels == 1 || channels == 3, "page_binarize_u8: channels = %d: 1 or 3", channels);
  DVD_REQUIRE(img && out, "page_binarize_u8: null pointer");
  DVD_REQUIRE(((uintptr_t)ink & 7) == 0, "page_binarize_u8: misaligned ink");
  DVD_REQUIRE(!cl::bytes_overlap(out, (size_t)h * w, img, (size_t)channels * h * w), "page_binarize_u8: out must share no byte with img");
  return cl::launch_binarize(img, channels, h, w, radius, kq, out, ink, (hipStream_t)stream);
}

extern "C" int dvd_page_clean_rgb8(const uint8_t* img, int h, int w, int cell, int close, int smooth, int neutral, int white, int flatten,
                                   int binarize, int radius, int kq, uint8_t* page, uint8_t* plane, unsigned long long* stats, void* ws,
                                   void* stream) {
  CLEAN_CHECK_PAGE("page_clean_rgb8");
  DVD_REQUIRE(flatten || binarize, "page_clean_rgb8: neither flatten nor binarize");
  if (flatten) {
    CLEAN_CHECK_BACKGROUND("page_clean_rgb8");
    CLEAN_CHECK_FLATTEN("page_clean_rgb8");
  } else {
    CLEAN_REQUIRE(cl::cell_ok(cell), DVD_E_CLEAN_PARAM, "page_clean_rgb8: cell = %d: 4, 8, 16, 32 or 64 (it sizes ws)", cell);
  }
  if (binarize) CLEAN_CHECK_BINARIZE("page_clean_rgb8");
  DVD_REQUIRE(img && ws && (!flatten || page) && (!binarize || plane), "page_clean_rgb8: null pointer");
  DVD_REQUIRE(((uintptr_t)stats & 7) == 0, "page_clean_rgb8: misaligned stats");
  const size_t n = (size_t)h * w;
  const cl::Workspace lay = cl::workspace_of(h, w, cell);
  const uint8_t* outs[3] = {flatten ? page : nullptr, binarize ? plane : nullptr, (const uint8_t*)ws};
  const size_t sizes[3] = {3 * n, n, lay.total};
  for (int a = 0; a < 3; ++a) {
    DVD_REQUIRE(!cl::bytes_overlap(outs[a], sizes[a], img, 3 * n), "page_clean_rgb8: page, plane and ws must share no byte with img");
    for (int b = a + 1; b < 3; ++b)
      DVD_REQUIRE(!cl::bytes_overlap(outs[a], sizes[a], outs[b], sizes[b]), "page_clean_rgb8: page, plane and ws must share no byte");
  }
  const hipStream_t st = (hipStream_t)stream;
  uint8_t* base = (uint8_t*)ws;
  unsigned long long* cnt = stats;
  if (cnt && hipMemsetAsync(cnt, 0, DVD_CLEAN_STATS * sizeof(unsigned long long), st) != hipSuccess) return check_launch("page_clean_rgb8");
  if (flatten) {
    if (int e = cl::launch_background(img, h, w, cell, close, smooth, neutral, base + lay.cmax, base + lay.bg, st)) return e;
    if (int e = cl::launch_flatten(img, h, w, base + lay.bg, cell, white, page, binarize ? base + lay.gray : nullptr, cnt, st)) return e;
  }
  if (binarize)
    if (int e = cl::launch_binarize(flatten ? base + lay.gray : img, flatten ? 1 : 3, h, w, radius, kq, plane, cnt ? cnt + 2 : nullptr, st)) return e;
  return DVD_OK;
}
