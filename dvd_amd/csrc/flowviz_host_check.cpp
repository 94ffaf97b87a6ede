// Stand-alone CPU restatement of the kernels of flowviz.hip on the shared arithmetic of flowviz_core.h (plain C++, no HIP).
// tests/test_flowviz_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/flowviz_model.py byte for byte.
//   flowviz_host_check in.bin out.bin
// in.bin : int32 mode, then
//   mode 0 (dvd_flow_to_image_rgb8): int32 n, h, w, norm, bgr, f32 clip, the field [n,h,w,2] f32
//   mode 1 (dvd_flow_radius_max)   : int32 n, h, w, f32 clip, the field
//   mode 2 (dvd_flow_full_uv)      : int32 n, g, h, w, the coarse map [n,2,g,g] f32
//   mode 3 (dvd_flow_picture_rgb8) : int32 n, g, h, w, norm, bgr, the coarse map
// out.bin: modes 0 and 3 the pictures [n,h,w,3] u8, then with norm 'max' the radii [n] f32; mode 1 the radii; mode 2 the field
// stdout : the status the entry point returns for these arguments; a refusal writes nothing.
#include <string.h>

#include "flowviz_core.h"
#include "host_check_io.hpp"

using namespace dvd::fv;

// the largest radius of one image in the kernels' order: lane maxima over kRadPer pixels at stride kBlock, the wave's tree
// (block_ops.h's wave_max as lane 0 sees it), the four waves in order, lane t of 256 over partials t, t + 256, .., a tree
static float largest_radius(const float* field, size_t hw, float clip) {
  const long blocks = (long)((hw + (size_t)kBlock * kRadPer - 1) / ((size_t)kBlock * kRadPer));
  std::vector<float> partials((size_t)blocks);
  for (long blk = 0; blk < blocks; ++blk) {
    float lane[kBlock];
    for (int t = 0; t < kBlock; ++t) {
      lane[t] = 0.f;
      for (int k = 0; k < kRadPer; ++k) {
        const size_t p = ((size_t)blk * kRadPer + k) * kBlock + t;
        if (p < hw) {
          const float r = radius_of(field[2 * p], field[2 * p + 1], clip);
          lane[t] = r > lane[t] ? r : lane[t];
        }
      }
    }
    float red[kBlock / 64];
    for (int w = 0; w < kBlock / 64; ++w) {
      float* v = lane + 64 * w;
      for (int d = 32; d >= 1; d >>= 1)
        for (int i = 0; i < d; ++i) v[i] = v[i + d] > v[i] ? v[i + d] : v[i];
      red[w] = v[0];
    }
    float m = red[0];
    for (int w = 1; w < kBlock / 64; ++w) m = red[w] > m ? red[w] : m;
    partials[(size_t)blk] = m;
  }
  float red[kBlock];
  for (int t = 0; t < kBlock; ++t) {
    red[t] = 0.f;
    for (long i = t; i < blocks; i += kBlock) red[t] = partials[(size_t)i] > red[t] ? partials[(size_t)i] : red[t];
  }
  for (int s = kBlock / 2; s >= 1; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] = red[t + s] > red[t] ? red[t + s] : red[t];
  return red[0];
}

static void full_uv(const float* flow, int g, int h, int w, float* out) {
  const Up up = make_up(g, h, w);
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < w; ++j) {
      float* px = out + 2 * ((size_t)i * w + j);
      full_uv_at(flow, up, i, j, px, px + 1);
    }
}

// pictures and, with norm 'max', radii of n fields
static void pictures(const float* field, int n, int h, int w, int norm, float clip, int bgr, std::vector<uint8_t>& out) {
  const size_t hw = (size_t)h * w;
  std::vector<uint8_t> img((size_t)n * hw * 3);
  std::vector<float> largest((size_t)n);
  for (int d = 0; d < n; ++d) {
    const float* f = field + (size_t)d * hw * 2;
    largest[d] = norm == DVD_FLOW_NORM_MAX ? largest_radius(f, hw, clip) : 0.f;
    const float rad_max = norm == DVD_FLOW_NORM_MAX ? max_rad_max(largest[d]) : diag_rad_max(h, w);
    for (size_t p = 0; p < hw; ++p) {
      int rgb[3];
      pixel_rgb(f[2 * p], f[2 * p + 1], rad_max, clip, rgb);
      uint8_t* px = img.data() + ((size_t)d * hw + p) * 3;
      px[0] = (uint8_t)(bgr ? rgb[2] : rgb[0]);
      px[1] = (uint8_t)rgb[1];
      px[2] = (uint8_t)(bgr ? rgb[0] : rgb[2]);
    }
  }
  append(out, img.data(), img.size());
  if (norm == DVD_FLOW_NORM_MAX) append(out, largest.data(), largest.size() * 4);
}

static int refuse(int status) {
  printf("%d\n", status);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: flowviz_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_all(argv[1], file) || file.size() < 4) return 2;
  int32_t mode;
  memcpy(&mode, file.data(), 4);
  int32_t head[7] = {0, 0, 0, 0, 0, 0, 0};
  const size_t words = mode == 0 ? 6 : (mode == 1 ? 4 : (mode == 2 ? 4 : (mode == 3 ? 6 : 0)));
  if (!words || file.size() < 4 + 4 * words) return 2;
  memcpy(head, file.data() + 4, 4 * words);
  const size_t body_at = 4 + 4 * words, body_floats = (file.size() - body_at) / 4;
  if ((file.size() - body_at) % 4) return 2;
  std::vector<float> body(body_floats);
  if (body_floats) memcpy(body.data(), file.data() + body_at, body_floats * 4);
  std::vector<uint8_t> out;
  if (mode == 0 || mode == 1) {
    const int n = head[0], h = head[1], w = head[2];
    const int norm = mode == 0 ? head[3] : DVD_FLOW_NORM_MAX, bgr = mode == 0 ? head[4] : 0;
    float clip;
    memcpy(&clip, &head[mode == 0 ? 5 : 3], 4);
    if (check_shape(n, h, w) != DVD_OK) return refuse(DVD_E_FLOW_SHAPE);
    if (check_norm(norm) != DVD_OK || check_clip(clip) != DVD_OK) return refuse(DVD_E_ARG);
    const size_t hw = (size_t)h * w;
    if (body_floats != (size_t)n * hw * 2) return 2;
    if (mode == 0) {
      pictures(body.data(), n, h, w, norm, clip, bgr, out);
    } else {
      std::vector<float> largest((size_t)n);
      for (int d = 0; d < n; ++d) largest[d] = largest_radius(body.data() + (size_t)d * hw * 2, hw, clip);
      append(out, largest.data(), largest.size() * 4);
    }
  } else {
    const int n = head[0], g = head[1], h = head[2], w = head[3];
    const int norm = mode == 3 ? head[4] : DVD_FLOW_NORM_DIAG, bgr = mode == 3 ? head[5] : 0;
    if (check_shape(n, h, w) != DVD_OK || check_grid(g) != DVD_OK) return refuse(DVD_E_FLOW_SHAPE);
    if (check_norm(norm) != DVD_OK) return refuse(DVD_E_ARG);
    const size_t hw = (size_t)h * w, gg = (size_t)g * g;
    if (body_floats != (size_t)n * 2 * gg) return 2;
    std::vector<float> field((size_t)n * hw * 2);
    for (int d = 0; d < n; ++d) full_uv(body.data() + (size_t)d * 2 * gg, g, h, w, field.data() + (size_t)d * hw * 2);
    if (mode == 2) append(out, field.data(), field.size() * 4);
    else pictures(field.data(), n, h, w, norm, -1.f, bgr, out);
  }
  const uint8_t none = 0;                                      // an empty batch: an empty file, from a pointer that is not null
  if (!write_all(argv[2], out.empty() ? &none : out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
