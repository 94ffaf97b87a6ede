// Stand-alone CPU restatement of the kernels of corrupt.hip on the shared arithmetic of corrupt_core.h (plain C++, no HIP).
// tests/test_corrupt_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/corrupt_model.py byte for
// byte.
//   corrupt_host_check in.bin out.bin
// in.bin : int32 n, h, w, kind, severity, then keys [n,2] uint32, then the images [n,h,w,3] u8
// out.bin: the corrupted images [n,h,w,3] u8
// stdout : the status dvd_corrupt_rgb8 returns for these arguments; a refusal writes nothing.
#include <string.h>

#include "corrupt_core.h"
#include "host_check_io.hpp"

using namespace dvd::cr;

static void one_image(const uint8_t* in, uint8_t* out, int h, int w, const Params& p, uint32_t k0, uint32_t k1) {
  const size_t pixels = (size_t)h * w;
  const int kind = p.kind;
  if (kind == kGaussianNoise || kind == kSpeckleNoise || kind == kImpulseNoise || kind == kShotNoise) {
    const std::vector<uint32_t> shot = kind == kShotNoise ? shot_table(p.severity) : std::vector<uint32_t>();
    for (size_t e = 0; e < pixels * 3; ++e) {
      const int x = in[e];
      uint32_t u[4];
      philox(k0, k1, (uint32_t)e, 0, (uint32_t)kind, 0, u);
      if (kind == kGaussianNoise) out[e] = (uint8_t)gaussian_px(x, p.gain, irwin_hall(k0, k1, (uint32_t)e));
      if (kind == kSpeckleNoise) out[e] = (uint8_t)speckle_px(x, p.gain, irwin_hall(k0, k1, (uint32_t)e));
      if (kind == kImpulseNoise) out[e] = (uint8_t)impulse_px(x, u[0], p.t_hi, p.t_lo);
      if (kind == kShotNoise) out[e] = (uint8_t)shot_px(u[0], shot.data() + (size_t)x * p.photons, p.photons);
    }
    return;
  }
  if (is_fir(kind)) {
    const std::vector<uint32_t> wt = fir_table(kind, p.severity, kind == kMotionBlur ? motion_angle(k0, k1) : 0);
    const int side = p.side, r = side / 2;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        uint32_t acc[3] = {0, 0, 0};
        for (int dy = 0; dy < side; ++dy)
          for (int dx = 0; dx < side; ++dx) {
            const uint32_t wv = wt[(size_t)dy * side + dx];
            if (!wv) continue;
            const uint8_t* px = in + ((size_t)reflect101(y + dy - r, h) * w + reflect101(x + dx - r, w)) * 3;
            for (int c = 0; c < 3; ++c) acc[c] += wv * px[c];
          }
        for (int c = 0; c < 3; ++c) out[((size_t)y * w + x) * 3 + c] = (uint8_t)((acc[c] + 32768) >> 16);
      }
    return;
  }
  uint32_t mean8[3] = {0, 0, 0};
  if (kind == kContrast)
    for (int c = 0; c < 3; ++c) {
      uint64_t sum = 0;
      for (size_t i = 0; i < pixels; ++i) sum += in[i * 3 + c];
      mean8[c] = mean_q8(sum, pixels);
    }
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t at0 = ((size_t)y * w + x) * 3;
      if (kind == kBrightness) {
        int v[3];
        brightness_px(in[at0], in[at0 + 1], in[at0 + 2], p.lift, v);
        for (int c = 0; c < 3; ++c) out[at0 + c] = (uint8_t)v[c];
        continue;
      }
      for (int c = 0; c < 3; ++c) {
        auto at = [&](int yy, int xx) { return (int)in[((size_t)yy * w + xx) * 3 + c]; };
        if (kind == kContrast) out[at0 + c] = (uint8_t)contrast_px(in[at0 + c], mean8[c], p.keep);
        if (kind == kZoomBlur) out[at0 + c] = (uint8_t)zoom_px(at, h, w, y, x, p.zooms, p.zstep);
        if (kind == kPixelate) out[at0 + c] = (uint8_t)pixelate_px(at, h, w, y, x, p.cells);
      }
    }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: corrupt_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  int32_t head[5];
  if (!read_all(argv[1], file) || file.size() < sizeof(head)) return 2;
  memcpy(head, file.data(), sizeof(head));
  const int n = head[0], h = head[1], w = head[2], kind = head[3], severity = head[4];
  int status = DVD_OK;                                       // the order of dvd_corrupt_rgb8's checks
  if (kind < 0 || kind >= kKinds) status = DVD_E_CORRUPT_KIND;
  else if (severity < 1 || severity > 5) status = DVD_E_CORRUPT_SEVERITY;
  else if (supported(kind) != 1) status = DVD_E_CORRUPT_KIND;
  else if (h < kMinSide || w < kMinSide || h > kMaxSide || w > kMaxSide) status = DVD_E_CORRUPT_SIZE;
  else if (n < 1 || n > 65535) status = DVD_E_ARG;
  if (status) {
    printf("%d\n", status);
    return 0;
  }
  const size_t image = (size_t)h * w * 3, keys_at = sizeof(head), images_at = keys_at + (size_t)n * 8;
  if (file.size() != images_at + n * image) return 2;
  std::vector<uint32_t> keys((size_t)n * 2);
  memcpy(keys.data(), file.data() + keys_at, (size_t)n * 8);
  std::vector<uint8_t> out(n * image);
  const Params p = params_for(kind, severity);
  for (int i = 0; i < n; ++i) one_image(file.data() + images_at + i * image, out.data() + i * image, h, w, p, keys[2 * i], keys[2 * i + 1]);
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
