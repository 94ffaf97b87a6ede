// Stand-alone CPU restatement of the kernels of sized.hip on the shared arithmetic of sized_core.h (plain C++, no HIP).
// tests/test_sized_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/sized_model.py.
//   sized_host_check in.bin out.bin
// in.bin : int32 g, hs, ws, hp, wp, max_radius, alias; f32 scale; then flow [2,g,g] f32 and src [hs,ws,3] u8.  alias != 0 asks
//          what the entry point answers when the page is written over the photograph.
// out.bin: the page [hp,wp,3] u8, the radii [hp,wp] u16 and the three counts as u64.  Every buffer is allocated at its exact
//          size: a read or write past one is a sanitizer report.
// stdout : the status the entry points return for these arguments; a refusal writes nothing.
#include <string.h>

#include "sized_core.h"
#include "host_check_io.hpp"

using namespace dvd;
using namespace dvd::sz;

// a pixel's neighbourhood in the plane of positions; off the page: kNone
struct PlaneAt {
  const Pos* pos;
  int h, w, y, x;
  Pos operator()(int dy, int dx) const {
    const int yy = y + dy, xx = x + dx;
    Pos none;
    none.x = kNone;
    none.y = 0;
    return yy < 0 || yy >= h || xx < 0 || xx >= w ? none : pos[(size_t)yy * w + xx];
  }
};

static int refuse(int status) {
  printf("%d\n", status);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: sized_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_all(argv[1], file) || file.size() < 32) return 2;
  int32_t head[7];
  float scale;
  memcpy(head, file.data(), 28);
  memcpy(&scale, file.data() + 28, 4);
  const int g = head[0], hs = head[1], ws = head[2], hp = head[3], wp = head[4], max_radius = head[5], alias = head[6];
  if (check_shape(g, hs, ws, hp, wp) != DVD_OK) return refuse(DVD_E_SIZED_SHAPE);
  if (check_params(scale, max_radius) != DVD_OK) return refuse(DVD_E_SIZED_PARAM);
  const size_t n = (size_t)hp * wp, ns = (size_t)hs * ws, nf = (size_t)2 * g * g;
  if (file.size() != 32 + 4 * nf + 3 * ns) return 2;
  std::vector<float> flow(nf);
  std::vector<uint8_t> src(3 * ns), page(3 * n);
  memcpy(flow.data(), file.data() + 32, 4 * nf);
  memcpy(src.data(), file.data() + 32 + 4 * nf, 3 * ns);
  if (int e = check_pointers(flow.data(), src.data(), alias ? src.data() + 1 : page.data(), hs, ws, hp, wp)) return refuse(e);

  // stage_tile: flow_grid_at is flow_grid_from on the axis terms of the pixel's row and column
  const UpParams up = make_up(g, hp, wp, scale);
  std::vector<Pos> pos(n);
  for (int y = 0; y < hp; ++y)
    for (int x = 0; x < wp; ++x) {
      float gx, gy;
      flow_grid_at(flow.data(), up, y, x, gx, gy);
      pos[(size_t)y * wp + x] = pos_of(gx, gy, hs, ws);
    }
  // unwarp_tile, sized_footprint_kernel
  std::vector<uint16_t> radii(n);
  Counts cnt;
  cnt.capped = cnt.outside = cnt.invalid = 0;
  for (int y = 0; y < hp; ++y)
    for (int x = 0; x < wp; ++x) {
      const size_t p = (size_t)y * wp + x;
      PlaneAt at;
      at.pos = pos.data();
      at.h = hp;
      at.w = wp;
      at.y = y;
      at.x = x;
      uint32_t rgb[3];
      pixel_at(src.data(), hs, ws, at, max_radius, rgb, cnt);
      for (int q = 0; q < 3; ++q) page[3 * p + q] = (uint8_t)rgb[q];
      radii[p] = radii_at(at, max_radius);
    }
  const unsigned long long stats[DVD_SIZED_STATS] = {cnt.capped, cnt.outside, cnt.invalid};
  std::vector<uint8_t> out;
  append(out, page.data(), 3 * n);
  append(out, radii.data(), 2 * n);
  append(out, stats, sizeof(stats));
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
