// Image-quality metric of the evaluation tail: MS-SSIM of the dewarped page against the flat ground-truth scan, on the device
// where the page already lies (DESIGN.md section 4.3 holds the definition; the float64 statement of it is tests/msssim_model.py).
// The reference leaves this to offline MATLAB (matlab_code/run_docunet.m); parity with MATLAB's imresize / rgb2gray / ssim /
// impyramid is UNPINNED, like the ingest against a real OpenCV.
//   dvd_resize_gray_u8   u8 RGB -> anti-aliased triangle resize (f64 taps and sums), one rounding to u8, gray: f32 plane
//   dvd_ssim_scale       one scale: 11x11 Gaussian moments, the cs / ssim rationals, (sum ssim, sum cs) per 32x32 tile
//   dvd_ssim_finalize    per document: the tile partials summed in a fixed order (f64) -> the scale's two means
//   dvd_reduce2_pair     both planes reduced by 2 (box or [1,4,6,4,1]/16)
//   dvd_msssim_scales    the five scales of one pair of planes, enqueued back to back
// No atomics anywhere: every result is a pure function of its inputs (same bits on every launch, in any batch).
#include "common.h"
#include "block_ops.h"
#include "workspace.h"

#include <math.h>

namespace dvd {

// ---------------------------------------------------------------- resize + gray --------------------------------------------
// One axis of the resize.  Output index o has its centre at u = (o + 0.5) / r - 0.5 (r = out / in), taps
// j = ceil(u - 1/s) .. floor(u + 1/s) with s = min(r, 1), weight tri((u - j) s), normalised to sum 1; the tap INDEX is clamped
// into the axis where it is read (the weight stays with its tap).
struct ResizeGrayAxis {
  double* wt;   // [out, maxtaps] normalised weights
  int* j0;      // [out] first (unclamped) tap
  int* cnt;     // [out] taps
};

__global__ void resize_gray_axis_kernel(ResizeGrayAxis ax, int isize, int osize, int maxtaps) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= osize) return;
  const double r = (double)osize / (double)isize;
  const double s = r < 1.0 ? r : 1.0;
  const double u = ((double)o + 0.5) / r - 0.5;
  const double sup = 1.0 / s;
  const int lo = (int)ceil(u - sup);
  int n = (int)floor(u + sup) - lo + 1;
  n = n < 1 ? 1 : (n > maxtaps ? maxtaps : n);
  double* wt = ax.wt + (size_t)o * maxtaps;
  double sum = 0.0;
  for (int k = 0; k < n; ++k) {
    const double t = fabs((u - (double)(lo + k)) * s);
    const double v = t < 1.0 ? 1.0 - t : 0.0;
    wt[k] = v;
    sum += v;
  }
  for (int k = 0; k < n; ++k) wt[k] = wt[k] / sum;
  ax.j0[o] = lo;
  ax.cnt[o] = n;
}

// one output pixel per thread; blockIdx.z = document
__global__ void __launch_bounds__(256) resize_gray_kernel(const uint8_t* __restrict__ src, int h, int w, ResizeGrayAxis ay,
                                                          ResizeGrayAxis ax, int mty, int mtx, float* __restrict__ out,
                                                          int oh, int ow) {
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= ow) return;
  const uint8_t* img = src + (size_t)blockIdx.z * h * w * 3;
  const int y0 = ay.j0[dy], ny = ay.cnt[dy], x0 = ax.j0[dx], nx = ax.cnt[dx];
  const double* wy = ay.wt + (size_t)dy * mty;
  const double* wx = ax.wt + (size_t)dx * mtx;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = 0; i < ny; ++i) {
    const uint8_t* row = img + (size_t)min(max(y0 + i, 0), h - 1) * w * 3;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int j = 0; j < nx; ++j) {
      const uint8_t* p = row + (size_t)min(max(x0 + j, 0), w - 1) * 3;
      const double g = wx[j];
      r0 += g * (double)p[0];
      r1 += g * (double)p[1];
      r2 += g * (double)p[2];
    }
    const double g = wy[i];
    a0 += g * r0;
    a1 += g * r1;
    a2 += g * r2;
  }
  // the one rounding to u8 (half to even), then gray = round(0.2989 R + 0.5870 G + 0.1140 B) evaluated exactly in units of 1e-4
  const int R = min(max((int)rint(a0), 0), 255), G = min(max((int)rint(a1), 0), 255), B = min(max((int)rint(a2), 0), 255);
  const int t = 2989 * R + 5870 * G + 1140 * B;
  int q = t / 10000;
  const int rem = t - q * 10000;
  if (rem > 5000 || (rem == 5000 && (q & 1))) ++q;
  out[((size_t)blockIdx.z * oh + dy) * ow + dx] = (float)min(q, 255);
}

// ---------------------------------------------------------------- one SSIM scale -------------------------------------------
constexpr int kTile = 32;               // output tile side
constexpr int kTaps = 11;               // Gaussian window
constexpr int kHalo = kTile + kTaps - 1;
constexpr float kCentre = 127.5f;       // subtracted from both planes: variances unchanged, E[x^2] - mu^2 cancels 4x less
constexpr float kC1 = 6.5025f;          // (0.01 * 255)^2
constexpr float kC2 = 58.5225f;         // (0.03 * 255)^2

struct SsimWindow { float g[kTaps]; };

// One 32 x 32 tile of the map per workgroup of 256 threads; blockIdx.z = document.  VALID: the map is (h-10) x (w-10) and
// pixel (i, j) sees x[i..i+10][j..j+10]; otherwise the map is h x w and the window is centred, indices clamped (replicate).
// LDS: 2 halo planes 42 x 43 f32 (14.4 KB) + 5 row-filtered planes 42 x 32 f32 (26.9 KB).
template <bool VALID>
__global__ void __launch_bounds__(256) ssim_scale_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w,
                                                         int mh, int mw, SsimWindow win, double* __restrict__ partials) {
  __shared__ float sx[kHalo][kHalo + 1], sy[kHalo][kHalo + 1];
  __shared__ float hp[5][kHalo][kTile];
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  const int ox = blockIdx.x * kTile, oy = blockIdx.y * kTile;
  const size_t plane = (size_t)blockIdx.z * h * w;
  const float* xd = x + plane;
  const float* yd = y + plane;
  constexpr int off = VALID ? 0 : -(kTaps / 2);
  for (int i = tid; i < kHalo * kHalo; i += 256) {
    const int r = i / kHalo, c = i - r * kHalo;
    const int gy = min(max(oy + r + off, 0), h - 1), gx = min(max(ox + c + off, 0), w - 1);
    sx[r][c] = __fsub_rn(xd[(size_t)gy * w + gx], kCentre);
    sy[r][c] = __fsub_rn(yd[(size_t)gy * w + gx], kCentre);
  }
  __syncthreads();
  // horizontal pass: mu_x, mu_y, E[xx], E[yy], E[xy] of every halo row
  for (int i = tid; i < kHalo * kTile; i += 256) {
    const int r = i / kTile, c = i % kTile;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float a = sx[r][c + k], b = sy[r][c + k], g = win.g[k];
      m0 = fmaf(g, a, m0);
      m1 = fmaf(g, b, m1);
      m2 = fmaf(g, __fmul_rn(a, a), m2);
      m3 = fmaf(g, __fmul_rn(b, b), m3);
      m4 = fmaf(g, __fmul_rn(a, b), m4);
    }
    hp[0][r][c] = m0; hp[1][r][c] = m1; hp[2][r][c] = m2; hp[3][r][c] = m3; hp[4][r][c] = m4;
  }
  __syncthreads();
  // vertical pass in registers: column tx, rows 4 tq .. 4 tq + 3
  const int tx = tid & 31, tq = tid >> 5;
  float acc[4][5];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int p = 0; p < 5; ++p) acc[o][p] = 0.f;
#pragma unroll
  for (int r = 0; r < kTaps + 3; ++r) {
    float v[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) v[p] = hp[p][tq * 4 + r][tx];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int k = r - o;
      if (k >= 0 && k < kTaps) {
#pragma unroll
        for (int p = 0; p < 5; ++p) acc[o][p] = fmaf(win.g[k], v[p], acc[o][p]);
      }
    }
  }
  // the rationals: every product and sum rounded on its own, so that x == y gives num == den bit for bit (ssim = cs = 1.0f)
  double s_ssim = 0.0, s_cs = 0.0;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int py = oy + tq * 4 + o, px = ox + tx;
    if (py < mh && px < mw) {
      const float mx = acc[o][0], my = acc[o][1];
      const float vxx = __fsub_rn(acc[o][2], __fmul_rn(mx, mx));
      const float vyy = __fsub_rn(acc[o][3], __fmul_rn(my, my));
      const float vxy = __fsub_rn(acc[o][4], __fmul_rn(mx, my));
      const float cs = __fdiv_rn(__fadd_rn(__fadd_rn(vxy, vxy), kC2), __fadd_rn(__fadd_rn(vxx, vyy), kC2));
      const float ux = __fadd_rn(mx, kCentre), uy = __fadd_rn(my, kCentre);
      const float uxy = __fmul_rn(ux, uy);
      const float lum = __fdiv_rn(__fadd_rn(__fadd_rn(uxy, uxy), kC1),
                                  __fadd_rn(__fadd_rn(__fmul_rn(ux, ux), __fmul_rn(uy, uy)), kC1));
      s_cs += (double)cs;
      s_ssim += (double)__fmul_rn(cs, lum);
    }
  }
  // workgroup reduction in a fixed order: butterfly inside each wave, then the four waves in order
  s_ssim = wave_sum(s_ssim);
  s_cs = wave_sum(s_cs);
  if ((tid & 63) == 0) { red[0][tid >> 6] = s_ssim; red[1][tid >> 6] = s_cs; }
  __syncthreads();
  if (tid == 0) {
    const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[tile * 2] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    partials[tile * 2 + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// one workgroup per document: partials [n, tiles, 2] -> out[d, scale, 0..1] = (mean ssim, mean cs)
__global__ void __launch_bounds__(256) ssim_finalize_kernel(const double* __restrict__ partials, int tiles, double count,
                                                            float* __restrict__ out, int scale) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const double* p = partials + (size_t)blockIdx.x * tiles * 2;
  double a = 0.0, b = 0.0;
  for (int t = tid; t < tiles; t += 256) { a += p[(size_t)t * 2]; b += p[(size_t)t * 2 + 1]; }
  red[0][tid] = a; red[1][tid] = b;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) { red[0][tid] += red[0][tid + d]; red[1][tid] += red[1][tid + d]; }
    __syncthreads();
  }
  if (tid == 0) {
    float* o = out + ((size_t)blockIdx.x * 5 + scale) * 2;
    o[0] = (float)(red[0][0] / count);
    o[1] = (float)(red[1][0] / count);
  }
}

// ---------------------------------------------------------------- reduce by 2 ----------------------------------------------
// out is ceil(h/2) x ceil(w/2).  TAPS 2: out[i] = (x[2i] + x[min(2i+1, n-1)]) / 2;  TAPS 5: [1,4,6,4,1]/16 centred on 2i,
// indices clamped.  Along the row first, then down the column; both planes per thread; blockIdx.z = document.
template <int TAPS>
__device__ __forceinline__ float reduce2_row(const float* __restrict__ row, int j, int w) {
  if (TAPS == 2) return __fmul_rn(__fadd_rn(row[2 * j], row[min(2 * j + 1, w - 1)]), 0.5f);
  const float a = row[max(2 * j - 2, 0)], b = row[max(2 * j - 1, 0)], c = row[2 * j], d = row[min(2 * j + 1, w - 1)],
              e = row[min(2 * j + 2, w - 1)];
  // (a + e) + 4 (b + d) + 6 c, each step rounded on its own, then / 16 (exact)
  return __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(a, e), __fmul_rn(4.f, __fadd_rn(b, d))), __fmul_rn(6.f, c)), 0.0625f);
}

template <int TAPS>
__device__ __forceinline__ float reduce2_at(const float* __restrict__ src, int i, int j, int h, int w) {
  if (TAPS == 2) {
    const float a = reduce2_row<2>(src + (size_t)(2 * i) * w, j, w);
    const float b = reduce2_row<2>(src + (size_t)min(2 * i + 1, h - 1) * w, j, w);
    return __fmul_rn(__fadd_rn(a, b), 0.5f);
  }
  const float a = reduce2_row<5>(src + (size_t)max(2 * i - 2, 0) * w, j, w);
  const float b = reduce2_row<5>(src + (size_t)max(2 * i - 1, 0) * w, j, w);
  const float c = reduce2_row<5>(src + (size_t)(2 * i) * w, j, w);
  const float d = reduce2_row<5>(src + (size_t)min(2 * i + 1, h - 1) * w, j, w);
  const float e = reduce2_row<5>(src + (size_t)min(2 * i + 2, h - 1) * w, j, w);
  return __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(a, e), __fmul_rn(4.f, __fadd_rn(b, d))), __fmul_rn(6.f, c)), 0.0625f);
}

template <int TAPS>
__global__ void __launch_bounds__(256) reduce2_pair_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           float* __restrict__ xo, float* __restrict__ yo, int h, int w,
                                                           int oh, int ow) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= ow) return;
  const size_t in = (size_t)blockIdx.z * h * w, out = ((size_t)blockIdx.z * oh + i) * ow + j;
  xo[out] = reduce2_at<TAPS>(x + in, i, j, h, w);
  yo[out] = reduce2_at<TAPS>(y + in, i, j, h, w);
}

// ---------------------------------------------------------------- host side ------------------------------------------------
static SsimWindow gaussian_window() {
  double g[kTaps], sum = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double d = (double)(k - kTaps / 2);
    g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  SsimWindow win;
  for (int k = 0; k < kTaps; ++k) win.g[k] = (float)(g[k] / sum);
  return win;
}

static int resize_maxtaps(int isize, int osize) {
  const double inv = (double)isize / (double)osize;
  return (int)floor(2.0 * (inv > 1.0 ? inv : 1.0)) + 2;     // floor(2/s) + 1 taps, and one of slack
}

constexpr int kMinSide = 176;          // the fifth scale (11 x 11) still holds one full window
constexpr int kMaxSide = 32768;        // tile grids and index arithmetic stay far inside int
constexpr int kMaxDocs = 65535;        // grid z

static void ssim_launch(const float* x, const float* y, int n, int h, int w, int border, double* partials, hipStream_t st) {
  const int mh = border == DVD_SSIM_VALID ? h - (kTaps - 1) : h, mw = border == DVD_SSIM_VALID ? w - (kTaps - 1) : w;
  const dim3 grd(cdiv(mw, kTile), cdiv(mh, kTile), n);
  const SsimWindow win = gaussian_window();
  if (border == DVD_SSIM_VALID)
    ssim_scale_kernel<true><<<grd, 256, 0, st>>>(x, y, h, w, mh, mw, win, partials);
  else
    ssim_scale_kernel<false><<<grd, 256, 0, st>>>(x, y, h, w, mh, mw, win, partials);

}

static void reduce2_launch(const float* x, const float* y, float* xo, float* yo, int n, int h, int w, int taps, hipStream_t st) {
  const int oh = (h + 1) / 2, ow = (w + 1) / 2;
  const dim3 grd(cdiv(ow, 256), oh, n);
  if (taps == 2)
    reduce2_pair_kernel<2><<<grd, 256, 0, st>>>(x, y, xo, yo, h, w, oh, ow);
  else
    reduce2_pair_kernel<5><<<grd, 256, 0, st>>>(x, y, xo, yo, h, w, oh, ow);
}

}  // namespace dvd

using namespace dvd;

extern "C" long dvd_resize_gray_scratch_bytes(int h, int w, int out_h, int out_w) {
  if (h < 1 || w < 1 || out_h < 1 || out_w < 1 || h > kMaxSide || w > kMaxSide || out_h > kMaxSide || out_w > kMaxSide) {
    set_error("resize_gray_scratch_bytes: bad shape %dx%d -> %dx%d", h, w, out_h, out_w);
    return DVD_E_ARG;
  }
  const size_t wt = ((size_t)out_h * resize_maxtaps(h, out_h) + (size_t)out_w * resize_maxtaps(w, out_w)) * sizeof(double);
  return (long)(wt + 2 * ((size_t)out_h + out_w) * sizeof(int));
}

extern "C" int dvd_resize_gray_u8(const uint8_t* src_nhwc, int n, int h, int w, float* out, int out_h, int out_w,
                                  void* scratch, void* stream) {
  DVD_REQUIRE(src_nhwc && out && scratch, "resize_gray_u8: null pointer");
  DVD_REQUIRE(n >= 1 && n <= kMaxDocs, "resize_gray_u8: bad batch %d", n);
  DVD_REQUIRE(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1 && h <= kMaxSide && w <= kMaxSide && out_h <= kMaxSide &&
                  out_w <= kMaxSide, "resize_gray_u8: bad shape %dx%d -> %dx%d", h, w, out_h, out_w);
  hipStream_t st = (hipStream_t)stream;
  const int mty = resize_maxtaps(h, out_h), mtx = resize_maxtaps(w, out_w);
  ResizeGrayAxis ay, ax;
  ay.wt = (double*)scratch;
  ax.wt = ay.wt + (size_t)out_h * mty;
  ay.j0 = (int*)(ax.wt + (size_t)out_w * mtx);
  ay.cnt = ay.j0 + out_h;
  ax.j0 = ay.cnt + out_h;
  ax.cnt = ax.j0 + out_w;
  resize_gray_axis_kernel<<<cdiv(out_h, 256), 256, 0, st>>>(ay, h, out_h, mty);
  resize_gray_axis_kernel<<<cdiv(out_w, 256), 256, 0, st>>>(ax, w, out_w, mtx);
  resize_gray_kernel<<<dim3(cdiv(out_w, 256), out_h, n), 256, 0, st>>>(src_nhwc, h, w, ay, ax, mty, mtx, out, out_h, out_w);
  return check_launch("resize_gray_u8");
}

extern "C" int dvd_ssim_scale(const float* x, const float* y, int n, int h, int w, int border, double* partials, void* stream) {
  DVD_REQUIRE(x && y && partials, "ssim_scale: null pointer");
  DVD_REQUIRE(n >= 1 && n <= kMaxDocs, "ssim_scale: bad batch %d", n);
  DVD_REQUIRE(border == DVD_SSIM_REPLICATE || border == DVD_SSIM_VALID, "ssim_scale: unknown border flag %d", border);
  DVD_REQUIRE(h >= kTaps && w >= kTaps && h <= kMaxSide && w <= kMaxSide, "ssim_scale: bad shape %dx%d (each side 11..32768)", h, w);
  ssim_launch(x, y, n, h, w, border, partials, (hipStream_t)stream);
  return check_launch("ssim_scale");
}

extern "C" int dvd_ssim_finalize(const double* partials, int n, int tiles, long count, float* out_n52, int scale, void* stream) {
  DVD_REQUIRE(partials && out_n52, "ssim_finalize: null pointer");
  DVD_REQUIRE(n >= 1 && n <= kMaxDocs, "ssim_finalize: bad batch %d", n);
  DVD_REQUIRE(tiles >= 1 && count >= 1 && count <= (long)tiles * kTile * kTile, "ssim_finalize: bad tiles %d / count %ld", tiles,
              count);
  DVD_REQUIRE(scale >= 0 && scale < 5, "ssim_finalize: bad scale %d", scale);
  ssim_finalize_kernel<<<n, 256, 0, (hipStream_t)stream>>>(partials, tiles, (double)count, out_n52, scale);
  return check_launch("ssim_finalize");
}

extern "C" int dvd_reduce2_pair(const float* x, const float* y, float* x_out, float* y_out, int n, int h, int w, int taps,
                                void* stream) {
  DVD_REQUIRE(x && y && x_out && y_out, "reduce2_pair: null pointer");
  DVD_REQUIRE(n >= 1 && n <= kMaxDocs, "reduce2_pair: bad batch %d", n);
  DVD_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "reduce2_pair: bad shape %dx%d", h, w);
  DVD_REQUIRE(taps == 2 || taps == 5, "reduce2_pair: taps must be 2 or 5, got %d", taps);
  reduce2_launch(x, y, x_out, y_out, n, h, w, taps, (hipStream_t)stream);
  return check_launch("reduce2_pair");
}

// workspace: partials [n, tiles of scale 1, 2] f64, then for each of scales 2..5 the planes x [n,h_s,w_s] and y [n,h_s,w_s] f32
struct MsssimWork { size_t partials, plane[5][2], total; };   // plane[0] is unused: scale 1 reads the caller's planes

static MsssimWork msssim_work(int h, int w, int n) {
  MsssimWork wk{};
  Carver c;
  wk.partials = c.take((size_t)n * cdiv(h, kTile) * cdiv(w, kTile) * 2 * sizeof(double));
  for (int s = 1; s < 5; ++s) {
    h = (h + 1) / 2, w = (w + 1) / 2;
    for (int k = 0; k < 2; ++k) wk.plane[s][k] = c.take((size_t)n * h * w * sizeof(float));
  }
  wk.total = c.at;
  return wk;
}

extern "C" long dvd_msssim_workspace_bytes(int h, int w, int n) {
  if (h < kMinSide || w < kMinSide || h > kMaxSide || w > kMaxSide || n < 1 || n > kMaxDocs) {
    set_error("msssim_workspace_bytes: bad shape %dx%d (each side 176..32768) or batch %d", h, w, n);
    return DVD_E_ARG;
  }
  return (long)msssim_work(h, w, n).total;
}

extern "C" int dvd_msssim_scales(const float* x, const float* y, int n, int h, int w, int preset, void* workspace,
                                 float* out_n52, void* stream) {
  DVD_REQUIRE(x && y && workspace && out_n52, "msssim_scales: null pointer");
  DVD_REQUIRE(n >= 1 && n <= kMaxDocs, "msssim_scales: bad batch %d", n);
  DVD_REQUIRE(preset == DVD_MSSSIM_DOCUNET || preset == DVD_MSSSIM_WANG, "msssim_scales: unknown preset flag %d", preset);
  DVD_REQUIRE(h >= kMinSide && w >= kMinSide && h <= kMaxSide && w <= kMaxSide,
              "msssim_scales: bad shape %dx%d (each side 176..32768: the fifth scale must hold one 11x11 window)", h, w);
  hipStream_t st = (hipStream_t)stream;
  const int border = preset == DVD_MSSSIM_WANG ? DVD_SSIM_VALID : DVD_SSIM_REPLICATE;
  const int taps = preset == DVD_MSSSIM_WANG ? 2 : 5;
  const MsssimWork wk = msssim_work(h, w, n);
  char* base = (char*)workspace;
  double* partials = (double*)(base + wk.partials);
  const float* cx = x;
  const float* cy = y;
  for (int s = 0; s < 5; ++s) {
    const int mh = border == DVD_SSIM_VALID ? h - (kTaps - 1) : h, mw = border == DVD_SSIM_VALID ? w - (kTaps - 1) : w;
    ssim_launch(cx, cy, n, h, w, border, partials, st);
    ssim_finalize_kernel<<<n, 256, 0, st>>>(partials, cdiv(mh, kTile) * cdiv(mw, kTile), (double)mh * (double)mw, out_n52, s);
    if (s < 4) {
      const int oh = (h + 1) / 2, ow = (w + 1) / 2;
      float* nx = (float*)(base + wk.plane[s + 1][0]);
      float* ny = (float*)(base + wk.plane[s + 1][1]);
      reduce2_launch(cx, cy, nx, ny, n, h, w, taps, st);
      cx = nx; cy = ny; h = oh; w = ow;
    }
    if (int e = check_launch("msssim_scales")) return e;
  }
  return DVD_OK;
}
