// Image ingest of the sampling path: what Doc_benchmark.__getitem__ does on the CPU
// (datasets/doc_dataset/doc_benchmark.py:75-97) after the file is decoded:
//   img_ori = cv2.imread(path)[:, :, ::-1]             BGR -> RGB, uint8 [H,W,3]
//   img     = cv2.resize(img_ori, (512, 512))          INTER_LINEAR on uint8
//   source_image = ArrayToTensor(img) / 255.           float32 [3,512,512] in 0..1
// cv2 (opencv-python, un-pinned in the reference's requirements.txt) is absent from this image, so the resize
// restates OpenCV's published 8-bit INTER_LINEAR algorithm (imgproc/src/resize.cpp: half-pixel centres, 11-bit
// fixed-point coefficients rounded to nearest-even, horizontal pass into int32, vertical pass
// ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2; an exactly-2x downscale takes cv::resize's INTER_AREA switch).  Integer arithmetic throughout: bit-exact against
// oracle/ingest_oracle.py; parity with a real cv2 build is UNPINNED.
#include "common.h"
#include "ragged.h"

namespace dvd {

struct ResizeAxis {   // per destination index: source index and the two 11-bit coefficients
  int s;
  short a0, a1;
};

// coefficients of one axis at destination index d (shared by resize_axis_kernel and the ragged batch's table kernel)
__device__ __forceinline__ void resize_axis_at(ResizeAxis* __restrict__ tab, int ssize, int dsize, int d) {
  const double scale = (double)ssize / (double)dsize;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  // saturate_cast<short>(float * 2048): round to nearest, ties to even (cvRound)
  tab[d].s = s;
  tab[d].a0 = (short)__float2int_rn((1.f - f) * 2048.f);
  tab[d].a1 = (short)__float2int_rn(f * 2048.f);
}

// launched once per axis (<= 512 threads of work)
__global__ void resize_axis_kernel(ResizeAxis* __restrict__ tab, int ssize, int dsize) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= dsize) return;
  resize_axis_at(tab, ssize, dsize, d);
}

// one output pixel (dx, dy) of one image, all three channels; shared by ingest_resize_kernel and ingest_resize_ragged_kernel
__device__ __forceinline__ void ingest_resize_at(const uint8_t* __restrict__ src, int h, int w, int swap_rb,
                                                 const ResizeAxis* __restrict__ tx, const ResizeAxis* __restrict__ ty,
                                                 float* __restrict__ out, int osize, int dx, int dy) {
  if (h == 2 * osize && w == 2 * osize) {
    // exactly 2x in both axes: cv::resize switches INTER_LINEAR to INTER_AREA, whose 8-bit fast path is the rounded
    // mean of the 2x2 block (resizeAreaFast_: (S00 + S01 + S10 + S11 + 2) >> 2)
    const uint8_t* r0 = src + ((size_t)(2 * dy) * w + 2 * dx) * 3;
    const uint8_t* r1 = r0 + (size_t)w * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int sc = swap_rb ? 2 - ch : ch;
      const int u = ((int)r0[sc] + (int)r0[3 + sc] + (int)r1[sc] + (int)r1[3 + sc] + 2) >> 2;
      out[((size_t)ch * osize + dy) * osize + dx] = __fdiv_rn((float)u, 255.f);
    }
    return;
  }
  const ResizeAxis ax = tx[dx], ay = ty[dy];
  const int x0 = ax.s, x1 = min(ax.s + 1, w - 1), y0 = ay.s, y1 = min(ay.s + 1, h - 1);
  const uint8_t* r0 = src + ((size_t)y0 * w) * 3;
  const uint8_t* r1 = src + ((size_t)y1 * w) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int sc = swap_rb ? 2 - ch : ch;
    const int S0 = (int)r0[(size_t)x0 * 3 + sc] * ax.a0 + (int)r0[(size_t)x1 * 3 + sc] * ax.a1;   // horizontal pass, row y0
    const int S1 = (int)r1[(size_t)x0 * 3 + sc] * ax.a0 + (int)r1[(size_t)x1 * 3 + sc] * ax.a1;   // row y1
    const int v = ((((int)ay.a0 * (S0 >> 4)) >> 16) + (((int)ay.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
    const int u = min(max(v, 0), 255);
    out[((size_t)ch * osize + dy) * osize + dx] = __fdiv_rn((float)u, 255.f);
  }
}

__global__ void __launch_bounds__(256) ingest_resize_kernel(const uint8_t* __restrict__ src, int h, int w, int swap_rb,
                                                            const ResizeAxis* __restrict__ tx,
                                                            const ResizeAxis* __restrict__ ty, float* __restrict__ out,
                                                            int osize) {
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= osize) return;
  ingest_resize_at(src, h, w, swap_rb, tx, ty, out, osize, dx, dy);
}

__global__ void __launch_bounds__(256) swap_rb_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long px) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= px) return;
  const uint8_t b = src[i * 3], g = src[i * 3 + 1], r = src[i * 3 + 2];
  dst[i * 3] = r; dst[i * 3 + 1] = g; dst[i * 3 + 2] = b;
}

// ---- n images of n sizes per launch (dvd_ingest_u8_ragged).  The tables of image d are scratch[(2 d) * osize ..]: x, then y.
// Table and resize work is the same for every image (osize entries / osize^2 pixels), so those two grids carry the image in
// z; the full-resolution RGB copies differ by an order of magnitude and take the flat grid of ragged.h.
__global__ void resize_axis_ragged_kernel(ResizeAxis* __restrict__ scratch, RaggedTab tab, int dsize) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= dsize) return;
  const int img = blockIdx.z, axis = blockIdx.y;     // axis 0: x (source size w), 1: y (h)
  resize_axis_at(scratch + ((size_t)img * 2 + axis) * dsize, axis ? tab.h[img] : tab.w[img], dsize, d);
}

__global__ void __launch_bounds__(256) ingest_resize_ragged_kernel(RaggedTab tab, int swap_rb,
                                                                   const ResizeAxis* __restrict__ scratch,
                                                                   float* __restrict__ out, int osize) {
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y, img = blockIdx.z;
  if (dx >= osize) return;
  const ResizeAxis* tx = scratch + (size_t)img * 2 * osize;
  ingest_resize_at(tab.src[img], tab.h[img], tab.w[img], swap_rb, tx, tx + osize, out + (size_t)img * 3 * osize * osize, osize,
                   dx, dy);
}

// the RGB-order full-resolution copies: one thread per pixel, 256 pixels per block, flat over the images that want one
__global__ void __launch_bounds__(256) rgb_copy_ragged_kernel(RaggedTab tab, int swap_rb) {
  const unsigned tile = blockIdx.x;
  const int d = ragged_doc_of(tab, tile);
  const long i = (long)(tile - (d ? tab.tile_end[d - 1] : 0u)) * 256 + threadIdx.x;
  if (i >= (long)tab.h[d] * tab.w[d]) return;
  const uint8_t* src = tab.src[d];
  uint8_t* dst = tab.out[d];
  const uint8_t a = src[i * 3], g = src[i * 3 + 1], b = src[i * 3 + 2];
  dst[i * 3] = swap_rb ? b : a; dst[i * 3 + 1] = g; dst[i * 3 + 2] = swap_rb ? a : b;
}

}  // namespace dvd

using namespace dvd;

extern "C" long dvd_ingest_scratch_bytes(int out_size) { return (long)out_size * 2 * (long)sizeof(ResizeAxis); }

extern "C" int dvd_ingest_u8(const uint8_t* src_hwc, int h, int w, int swap_rb, float* y_chw, int out_size,
                             uint8_t* rgb_hwc_out, void* scratch, void* stream) {
  DVD_REQUIRE(src_hwc && y_chw && scratch, "ingest_u8: null pointer");
  DVD_REQUIRE(h >= 1 && w >= 1 && out_size >= 1 && out_size <= 65535, "ingest_u8: bad shape %dx%d -> %d", h, w, out_size);
  hipStream_t st = (hipStream_t)stream;
  ResizeAxis* tx = (ResizeAxis*)scratch;
  ResizeAxis* ty = tx + out_size;
  resize_axis_kernel<<<cdiv(out_size, 256), 256, 0, st>>>(tx, w, out_size);
  resize_axis_kernel<<<cdiv(out_size, 256), 256, 0, st>>>(ty, h, out_size);
  dim3 grd(cdiv(out_size, 256), out_size);
  ingest_resize_kernel<<<grd, 256, 0, st>>>(src_hwc, h, w, swap_rb ? 1 : 0, tx, ty, y_chw, out_size);
  if (rgb_hwc_out) {
    const long px = (long)h * w;
    if (swap_rb) {
      swap_rb_kernel<<<cdiv(px, 256), 256, 0, st>>>(src_hwc, rgb_hwc_out, px);
    } else if (rgb_hwc_out != src_hwc) {
      if (hipMemcpyAsync(rgb_hwc_out, src_hwc, (size_t)px * 3, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("ingest_u8: device copy failed");
        return DVD_E_LAUNCH;
      }
    }
  }
  return check_launch("ingest_u8");
}

extern "C" long dvd_ingest_ragged_scratch_bytes(int out_size, int n) {
  return (long)(n > 0 ? n : 0) * dvd_ingest_scratch_bytes(out_size);
}

extern "C" int dvd_ingest_u8_ragged(const dvd_ragged_image* docs, int n, int swap_rb, float* y_nchw, int out_size,
                                    void* scratch, void* stream) {
  DVD_REQUIRE(docs && y_nchw && scratch, "ingest_u8_ragged: null pointer");
  DVD_REQUIRE(n >= 0, "ingest_u8_ragged: bad batch %d", n);
  DVD_REQUIRE(out_size >= 1 && out_size <= 65535, "ingest_u8_ragged: bad output size %d", out_size);
  for (int d = 0; d < n; ++d) {       // every image is checked before the first launch
    DVD_REQUIRE(docs[d].src, "ingest_u8_ragged: null pointer in image %d", d);
    DVD_REQUIRE(docs[d].h >= 1 && docs[d].w >= 1 && docs[d].h <= 65535, "ingest_u8_ragged: bad shape h=%d w=%d of image %d",
                docs[d].h, docs[d].w, d);
    DVD_REQUIRE(!(swap_rb && docs[d].out == docs[d].src), "ingest_u8_ragged: image %d cannot be swapped in place", d);
    DVD_REQUIRE((long)docs[d].h * docs[d].w <= 256l * 0x7fffffffl, "ingest_u8_ragged: image %d too large", d);
  }
  hipStream_t st = (hipStream_t)stream;
  for (int d0 = 0; d0 < n;) {
    RaggedTab tab;
    size_t tiles = 0;
    int m = 0;
    for (; m < kRaggedCap && d0 + m < n; ++m) {
      const dvd_ragged_image& im = docs[d0 + m];
      const bool copy = im.out && (swap_rb || im.out != im.src);
      const size_t t = copy ? (size_t)cdiv((long)im.h * im.w, 256) : 0;
      if (tiles + t >= (1ull << 31)) break;
      tiles += t;
      tab.src[m] = im.src; tab.out[m] = im.out; tab.h[m] = im.h; tab.w[m] = im.w; tab.tile_end[m] = (unsigned)tiles;
    }
    for (int k = m; k < kRaggedCap; ++k) {    // unused entries: defined values in the kernel argument
      tab.src[k] = nullptr; tab.out[k] = nullptr; tab.h[k] = tab.w[k] = 0; tab.tile_end[k] = (unsigned)tiles;
    }
    tab.n = m;
    ResizeAxis* axes = (ResizeAxis*)scratch + (size_t)d0 * 2 * out_size;
    resize_axis_ragged_kernel<<<dim3(cdiv(out_size, 256), 2, m), 256, 0, st>>>(axes, tab, out_size);
    ingest_resize_ragged_kernel<<<dim3(cdiv(out_size, 256), out_size, m), 256, 0, st>>>(
        tab, swap_rb ? 1 : 0, axes, y_nchw + (size_t)d0 * 3 * out_size * out_size, out_size);
    if (tiles) rgb_copy_ragged_kernel<<<(unsigned)tiles, 256, 0, st>>>(tab, swap_rb ? 1 : 0);
    if (int e = check_launch("ingest_u8_ragged")) return e;
    d0 += m;
  }
  return DVD_OK;
}
