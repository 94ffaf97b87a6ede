// Stand-alone CPU restatement of the kernels of noise.hip on the shared arithmetic of noise_core.h (plain C++, no HIP).
// tests/test_noise_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/noise_model.py bit for bit.
//   noise_host_check in.bin out.bin
// in.bin : int32 mode, then
//   mode 0 (dvd_randn_keyed)  : int32 docs, n_hyp, g, uint32 slot, keys [docs,2] uint32
//   mode 1 (dvd_map_deviation): int32 docs, g, then a and b, each [docs,2,g,g] f32
// out.bin: mode 0 the normals [docs*n_hyp,2,g,g] f32; mode 1 the deviations [docs] f64, then the point distances [docs,g*g] f32
// stdout : the status the entry point returns for these arguments; a refusal writes nothing.
#include <string.h>

#include "host_check_io.hpp"
#include "noise_core.h"

using namespace dvd::nz;

// block_ops.h's wave_sum as lane 0 sees it: v += the value 32, 16, .. 1 lanes further down
static double wave_sum0(double* v) {
  for (int d = 32; d >= 1; d >>= 1)
    for (int i = 0; i < d; ++i) v[i] += v[i + d];
  return v[0];
}

static double deviation(const float* a, const float* b, int g, float* dist) {
  const size_t gg = (size_t)g * g;
  for (size_t p = 0; p < gg; ++p) dist[p] = point_distance(a[p], a[gg + p], b[p], b[gg + p]);
  const long blocks = deviation_blocks(g);
  std::vector<double> partials((size_t)blocks);
  for (long blk = 0; blk < blocks; ++blk) {
    double lane[kDevBlock];
    for (int t = 0; t < kDevBlock; ++t) {
      lane[t] = 0.0;
      for (int k = 0; k < kDevPer; ++k) {
        const size_t p = ((size_t)blk * kDevPer + k) * kDevBlock + t;
        if (p < gg) lane[t] += (double)dist[p];
      }
    }
    double red[kDevBlock / 64];
    for (int w = 0; w < kDevBlock / 64; ++w) red[w] = wave_sum0(lane + 64 * w);
    partials[(size_t)blk] = ((red[0] + red[1]) + red[2]) + red[3];
  }
  double red[256];
  for (int t = 0; t < 256; ++t) {
    red[t] = 0.0;
    for (long i = t; i < blocks; i += 256) red[t] += partials[(size_t)i];
  }
  for (int s = 128; s >= 1; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] += red[t + s];
  return kPx * (red[0] / (double)gg);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: noise_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_all(argv[1], file) || file.size() < 4) return 2;
  int32_t mode;
  memcpy(&mode, file.data(), 4);
  std::vector<uint8_t> out;
  if (mode == 0) {
    int32_t head[4];
    if (file.size() < 4 + sizeof(head)) return 2;
    memcpy(head, file.data() + 4, sizeof(head));
    const int docs = head[0], n_hyp = head[1], g = head[2];
    const uint32_t slot = (uint32_t)head[3];
    if (check_randn(docs, n_hyp, g) != DVD_OK) {
      printf("%d\n", DVD_E_ARG);
      return 0;
    }
    const size_t keys_at = 4 + sizeof(head);
    if (file.size() != keys_at + (size_t)docs * 8) return 2;
    std::vector<uint32_t> keys((size_t)docs * 2);
    if (docs) memcpy(keys.data(), file.data() + keys_at, (size_t)docs * 8);
    const uint32_t elems = 2u * g * g, quads = (elems + 3) / 4;
    std::vector<float> z((size_t)docs * n_hyp * elems);
    for (int d = 0; d < docs; ++d)
      for (int h = 0; h < n_hyp; ++h) {
        float* dst = z.data() + ((size_t)d * n_hyp + h) * elems;
        for (uint32_t q = 0; q < quads; ++q) {
          float v[4];
          quad_normals(keys[2 * d], keys[2 * d + 1], q, slot, (uint32_t)h, v);
          for (uint32_t r = 0; r < 4; ++r)
            if (4 * q + r < elems) dst[4 * q + r] = v[r];
        }
      }
    append(out, z.data(), z.size() * 4);
  } else if (mode == 1) {
    int32_t head[2];
    if (file.size() < 4 + sizeof(head)) return 2;
    memcpy(head, file.data() + 4, sizeof(head));
    const int docs = head[0], g = head[1];
    if (check_deviation(docs, g) != DVD_OK) {
      printf("%d\n", DVD_E_ARG);
      return 0;
    }
    const size_t gg = (size_t)g * g, maps = (size_t)docs * 2 * gg;
    if (file.size() != 4 + sizeof(head) + 2 * maps * 4) return 2;
    std::vector<float> a(maps), b(maps), dist((size_t)docs * gg);
    if (maps) {
      memcpy(a.data(), file.data() + 4 + sizeof(head), maps * 4);
      memcpy(b.data(), file.data() + 4 + sizeof(head) + maps * 4, maps * 4);
    }
    std::vector<double> dev((size_t)docs);
    for (int d = 0; d < docs; ++d) dev[d] = deviation(a.data() + (size_t)d * 2 * gg, b.data() + (size_t)d * 2 * gg, g, dist.data() + (size_t)d * gg);
    append(out, dev.data(), dev.size() * 8);
    append(out, dist.data(), dist.size() * 4);
  } else {
    return 2;
  }
  const uint8_t none = 0;                                      // an empty batch: an empty file, from a pointer that is not null
  if (!write_all(argv[2], out.empty() ? &none : out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
