// Common corruptions of the 512 x 512 network input (run_sampling.py --corruption) on [n,h,w,3] uint8
// images: the arithmetic is corrupt_core.h's, integer throughout; tests/corrupt_model.py restates every kind byte for byte.
// No kernel uses scratch memory or atomics, and no corruption kernel a float (the two ends of the stage, y = k / 255 and back,
// are the only float arithmetic: one correctly rounded multiplication or division).  The real-valued tables (Poisson CDFs,
// FIR weights) are built on the host once per process and copied once per device into the __device__ arrays below.
#include <mutex>

#include "block_ops.h"
#include "common.h"
#include "corrupt_core.h"

namespace dvd {
namespace cr {

__device__ uint32_t g_shot[5][256 * kShotMax];                          // [severity][x][j], rows of c entries
__device__ uint32_t g_fir[2][5][kMaxTaps * kMaxTaps];                   // defocus, gaussian: [severity][side][side]
__device__ uint32_t g_motion[5][kAngles][kMotionSide * kMotionSide];    // [severity][angle + 45][side][side]

constexpr int kNoisePer = 4;          // consecutive elements per thread of the noise kernel
constexpr int kTileW = 32, kTileH = 16, kFirLds = (kTileW + 2 * kMaxRadius) * (kTileH + 2 * kMaxRadius);

// kinds 0, 1, 2, 15: one Philox stream per element, in registers
__global__ __launch_bounds__(256) void corrupt_noise_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n3,
                                                            const uint32_t* __restrict__ keys, Params p) {
  const uint32_t k0 = keys[2 * blockIdx.y], k1 = keys[2 * blockIdx.y + 1];
  const size_t base = (size_t)blockIdx.y * n3;
  const uint32_t first = (blockIdx.x * 256u + threadIdx.x) * kNoisePer;
  const uint32_t* shot = g_shot[p.severity - 1];
#pragma unroll
  for (int i = 0; i < kNoisePer; ++i) {
    const uint32_t e = first + i;
    if (e >= n3) return;
    const int x = in[base + e];
    int v;
    if (p.kind == kGaussianNoise) {
      v = gaussian_px(x, p.gain, irwin_hall(k0, k1, e));
    } else if (p.kind == kSpeckleNoise) {
      v = speckle_px(x, p.gain, irwin_hall(k0, k1, e));
    } else {
      uint32_t u[4];
      philox(k0, k1, e, 0, (uint32_t)p.kind, 0, u);
      v = p.kind == kImpulseNoise ? impulse_px(x, u[0], p.t_hi, p.t_lo) : shot_px(u[0], shot + x * p.photons, p.photons);
    }
    out[base + e] = (uint8_t)v;
  }
}

// kinds 3, 5, 16: a 32 x 16 tile of outputs per workgroup; the tile and its halo sit in LDS as one packed pixel per word, the
// weights are read at wave-uniform addresses.  Lanes beyond the image compute on saturated indices and store nothing.
__global__ __launch_bounds__(256) void corrupt_fir_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int h, int w,
                                                          const uint32_t* __restrict__ keys, Params p) {
  __shared__ uint32_t tile[kFirLds];
  const int side = p.side, r = side / 2, lw = kTileW + 2 * r, lh = kTileH + 2 * r;
  const size_t base = (size_t)blockIdx.z * h * w * 3;
  const uint32_t* wt;
  if (p.kind == kMotionBlur)
    wt = g_motion[p.severity - 1][motion_angle(keys[2 * blockIdx.z], keys[2 * blockIdx.z + 1]) + 45];
  else
    wt = g_fir[p.kind == kGaussianBlur][p.severity - 1];
  const int x0 = blockIdx.x * kTileW - r, y0 = blockIdx.y * kTileH - r;
  for (int i = threadIdx.x; i < lw * lh; i += 256) {
    const int ly = i / lw, lx = i - ly * lw;
    const uint8_t* px = in + base + ((size_t)reflect101(y0 + ly, h) * w + reflect101(x0 + lx, w)) * 3;
    tile[i] = px[0] | (px[1] << 8) | (px[2] << 16);
  }
  __syncthreads();
  const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;      // rows ty and ty + 8
  uint32_t acc[2][3] = {};
  for (int dy = 0; dy < side; ++dy)
    for (int dx = 0; dx < side; ++dx) {
      const uint32_t wv = wt[dy * side + dx];
      if (!wv) continue;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint32_t px = tile[(ty + 8 * k + dy) * lw + tx + dx];
        acc[k][0] += wv * (px & 255);
        acc[k][1] += wv * ((px >> 8) & 255);
        acc[k][2] += wv * (px >> 16);
      }
    }
  const int x = blockIdx.x * kTileW + tx;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int y = blockIdx.y * kTileH + ty + 8 * k;
    if (x < w && y < h)
      for (int c = 0; c < 3; ++c) out[base + ((size_t)y * w + x) * 3 + c] = (uint8_t)((acc[k][c] + 32768) >> 16);
  }
}

// kinds 6, 10, 13: one thread per pixel, reads of the image only
__global__ __launch_bounds__(256) void corrupt_pixel_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int h, int w,
                                                            Params p) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const uint8_t* img = in + (size_t)blockIdx.z * h * w * 3;
  uint8_t* dst = out + ((size_t)blockIdx.z * h * w + (size_t)y * w + x) * 3;
  if (p.kind == kBrightness) {
    const uint8_t* px = img + ((size_t)y * w + x) * 3;
    int v[3];
    brightness_px(px[0], px[1], px[2], p.lift, v);
    for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)v[c];
    return;
  }
  for (int c = 0; c < 3; ++c) {
    auto at = [&](int yy, int xx) { return (int)img[((size_t)yy * w + xx) * 3 + c]; };
    dst[c] = (uint8_t)(p.kind == kZoomBlur ? zoom_px(at, h, w, y, x, p.zooms, p.zstep) : pixelate_px(at, h, w, y, x, p.cells));
  }
}

// kind 11: one workgroup per image: the three exact channel sums (lane partials, wave_sum, then the sixteen waves through
// LDS), then the pointwise pass
__global__ __launch_bounds__(1024) void corrupt_contrast_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int h, int w,
                                                                Params p) {
  __shared__ unsigned long long part[3][16];
  const size_t pixels = (size_t)h * w;
  const uint8_t* img = in + (size_t)blockIdx.x * pixels * 3;
  uint8_t* dst = out + (size_t)blockIdx.x * pixels * 3;
  unsigned long long s[3] = {0, 0, 0};
  for (size_t i = threadIdx.x; i < pixels; i += 1024)
    for (int c = 0; c < 3; ++c) s[c] += img[i * 3 + c];
  for (int c = 0; c < 3; ++c) {
    const unsigned long long v = wave_sum(s[c]);
    if ((threadIdx.x & 63) == 0) part[c][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  uint32_t mean8[3];
  for (int c = 0; c < 3; ++c) {
    unsigned long long t = 0;
    for (int k = 0; k < 16; ++k) t += part[c][k];
    mean8[c] = mean_q8(t, pixels);
  }
  for (size_t i = threadIdx.x; i < pixels; i += 1024)
    for (int c = 0; c < 3; ++c) dst[i * 3 + c] = (uint8_t)contrast_px(img[i * 3 + c], mean8[c], p.keep);
}

// The two ends of the stage: y [n,3,h,w] f32 in 0..1 -> bytes [n,h,w,3] (rint(255 y), clamped; NaN -> 0), and bytes -> k / 255
// by the correctly rounded division of the ingest kernel
__global__ __launch_bounds__(256) void unit_to_rgb8_kernel(const float* __restrict__ y, uint8_t* __restrict__ out, size_t pixels, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;       // over n * pixels
  if (i >= total) return;
  const size_t img = i / pixels, at = i - img * pixels;
  for (int c = 0; c < 3; ++c) {
    const float v = rintf(mul_rn(y[(img * 3 + c) * pixels + at], 255.f));
    out[i * 3 + c] = (uint8_t)(v >= 0.f ? (v <= 255.f ? (int)v : 255) : 0);
  }
}

__global__ __launch_bounds__(256) void rgb8_to_unit_kernel(const uint8_t* __restrict__ in, float* __restrict__ y, size_t pixels, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t img = i / pixels, at = i - img * pixels;
  for (int c = 0; c < 3; ++c) y[(img * 3 + c) * pixels + at] = div_rn((float)in[i * 3 + c], 255.f);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct Tables {
  std::vector<uint32_t> shot, fir, motion;
  Tables() : shot((size_t)5 * 256 * kShotMax, 0), fir((size_t)2 * 5 * kMaxTaps * kMaxTaps, 0),
             motion((size_t)5 * kAngles * kMotionSide * kMotionSide, 0) {
    for (int s = 1; s <= 5; ++s) {
      const std::vector<uint32_t> t = shot_table(s);
      std::copy(t.begin(), t.end(), shot.begin() + (size_t)(s - 1) * 256 * kShotMax);
      for (int g = 0; g < 2; ++g) {
        const std::vector<uint32_t> f = fir_table(g ? kGaussianBlur : kDefocusBlur, s, 0);
        std::copy(f.begin(), f.end(), fir.begin() + (size_t)(g * 5 + s - 1) * kMaxTaps * kMaxTaps);
      }
      for (int a = 0; a < kAngles; ++a) {
        const std::vector<uint32_t> m = fir_table(kMotionBlur, s, a - 45);
        std::copy(m.begin(), m.end(), motion.begin() + (size_t)((s - 1) * kAngles + a) * kMotionSide * kMotionSide);
      }
    }
  }
};

static const Tables& tables() {
  static const Tables t;
  return t;
}

// the tables on the current device: copied on the first call there, and complete before anyone is told so
static int upload_tables(hipStream_t stream) {
  static DeviceOnce once;
  static std::mutex lock;
  const unsigned long long bit = DeviceOnce::current_bit();
  if (!once.need(bit)) return DVD_OK;
  std::lock_guard<std::mutex> hold(lock);
  if (!once.need(bit)) return DVD_OK;
  const Tables& t = tables();
  hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_shot), t.shot.data(), t.shot.size() * 4, 0, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_fir), t.fir.data(), t.fir.size() * 4, 0, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_motion), t.motion.data(), t.motion.size() * 4, 0, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    set_error("dvd_corrupt_rgb8: copying the tables to the device: %s", hipGetErrorString(e));
    return DVD_E_LAUNCH;
  }
  once.done(bit);
  return DVD_OK;
}

static int check_kind(const char* who, int kind, int severity) {
  if (kind < 0 || kind >= kKinds) {
    set_error("%s: kind %d is not one of 0..18", who, kind);
    return DVD_E_CORRUPT_KIND;
  }
  if (severity < 1 || severity > 5) {
    set_error("%s: severity %d is not one of 1..5", who, severity);
    return DVD_E_CORRUPT_SEVERITY;
  }
  return DVD_OK;
}

}  // namespace cr
}  // namespace dvd

using namespace dvd;

extern "C" int dvd_corrupt_supported(int kind) { return cr::supported(kind); }

extern "C" int dvd_corrupt_table(int kind, int severity, int angle, uint32_t* out, int cap) {
  if (int rc = cr::check_kind("dvd_corrupt_table", kind, severity)) return rc;
  if (kind != cr::kShotNoise && !cr::is_fir(kind)) {
    set_error("dvd_corrupt_table: kind %d has no table", kind);
    return DVD_E_CORRUPT_KIND;
  }
  DVD_REQUIRE(kind != cr::kMotionBlur || (angle >= -45 && angle <= 45), "dvd_corrupt_table: angle %d is not one of -45..45", angle);
  const std::vector<uint32_t> t = kind == cr::kShotNoise ? cr::shot_table(severity) : cr::fir_table(kind, severity, angle);
  if (out) {
    DVD_REQUIRE(cap >= (int)t.size(), "dvd_corrupt_table: %d entries do not fit cap = %d", (int)t.size(), cap);
    std::copy(t.begin(), t.end(), out);
  }
  return (int)t.size();
}

static int check_planes(const char* who, const void* a, const void* b, int n, int h, int w) {
  DVD_REQUIRE(a && b, "%s: null pointer", who);
  DVD_REQUIRE(n >= 1 && h >= 1 && w >= 1 && (long)n * h * w < (1l << 31) / 3, "%s: n = %d, h = %d, w = %d: 3 n h w must be below 2^31", who, n, h, w);
  return DVD_OK;
}

extern "C" int dvd_unit_to_rgb8(const float* y_nchw, uint8_t* out_nhwc, int n, int h, int w, void* stream) {
  if (int rc = check_planes("dvd_unit_to_rgb8", y_nchw, out_nhwc, n, h, w)) return rc;
  const size_t pixels = (size_t)h * w, total = pixels * n;
  cr::unit_to_rgb8_kernel<<<cdiv((long)total, 256), 256, 0, (hipStream_t)stream>>>(y_nchw, out_nhwc, pixels, total);
  return check_launch("dvd_unit_to_rgb8");
}

extern "C" int dvd_rgb8_to_unit(const uint8_t* in_nhwc, float* y_nchw, int n, int h, int w, void* stream) {
  if (int rc = check_planes("dvd_rgb8_to_unit", in_nhwc, y_nchw, n, h, w)) return rc;
  const size_t pixels = (size_t)h * w, total = pixels * n;
  cr::rgb8_to_unit_kernel<<<cdiv((long)total, 256), 256, 0, (hipStream_t)stream>>>(in_nhwc, y_nchw, pixels, total);
  return check_launch("dvd_rgb8_to_unit");
}

extern "C" int dvd_corrupt_rgb8(const uint8_t* in, uint8_t* out, int n, int h, int w, int kind, int severity, const uint32_t* keys,
                                void* stream) {
  if (int rc = cr::check_kind("dvd_corrupt_rgb8", kind, severity)) return rc;
  if (cr::supported(kind) != 1) {
    set_error(kind == cr::kJpeg ? "dvd_corrupt_rgb8: kind 14 is dvd_jpeg_encode_rgb8 followed by dvd_jpeg_decode_rgb8"
                                : "dvd_corrupt_rgb8: kind %d has no device kernel", kind);
    return DVD_E_CORRUPT_KIND;
  }
  if (h < cr::kMinSide || w < cr::kMinSide || h > cr::kMaxSide || w > cr::kMaxSide) {
    set_error("dvd_corrupt_rgb8: %d x %d: every side must be %d..%d", h, w, cr::kMinSide, cr::kMaxSide);
    return DVD_E_CORRUPT_SIZE;
  }
  DVD_REQUIRE(n >= 1 && n <= 65535, "dvd_corrupt_rgb8: n = %d is not one of 1..65535", n);
  DVD_REQUIRE(in && out && keys, "dvd_corrupt_rgb8: null pointer");
  DVD_REQUIRE(in != out, "dvd_corrupt_rgb8: out must not be in");
  const cr::Params p = cr::params_for(kind, severity);
  hipStream_t s = (hipStream_t)stream;
  const uint32_t n3 = (uint32_t)h * w * 3;                                  // at most 3 * 2^28
  if (kind == cr::kShotNoise || cr::is_fir(kind))
    if (int rc = cr::upload_tables(s)) return rc;
  if (cr::is_fir(kind))
    cr::corrupt_fir_kernel<<<dim3(cdiv(w, cr::kTileW), cdiv(h, cr::kTileH), n), 256, 0, s>>>(in, out, h, w, keys, p);
  else if (kind == cr::kContrast)
    cr::corrupt_contrast_kernel<<<n, 1024, 0, s>>>(in, out, h, w, p);
  else if (kind == cr::kZoomBlur || kind == cr::kBrightness || kind == cr::kPixelate)
    cr::corrupt_pixel_kernel<<<dim3(cdiv(w, 64), cdiv(h, 4), n), 256, 0, s>>>(in, out, h, w, p);
  else
    cr::corrupt_noise_kernel<<<dim3(cdiv(n3, 256 * cr::kNoisePer), n), 256, 0, s>>>(in, out, n3, keys, p);
  return check_launch("dvd_corrupt_rgb8");
}
