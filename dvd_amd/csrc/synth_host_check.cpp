// Stand-alone CPU restatement of the kernels of synth.hip on the shared arithmetic of synth_core.h (plain C++, no HIP).
// tests/test_synth_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/synth_model.py.
//   synth_host_check in.bin out.bin
// in.bin : int32 hs, ws, h, w, has_bg; uint32 bg_color; f32 l0, lgx, lgy, k, a_ref; then scan [hs,ws,3] u8, fwd [h,w,2] f32 and,
//          with has_bg, bg [h,w,3] u8
// out.bin: the photograph [h,w,3] u8 and the radii [h,w,2] u8.  Every buffer is allocated at its exact size: a read or write
//          past one is a sanitizer report.
// stdout : the status the entry points return for these arguments; a refusal writes nothing.
#include <string.h>

#include "synth_core.h"
#include "host_check_io.hpp"

using namespace dvd;
using namespace dvd::sy;

// a pixel's neighbourhood in the plane of positions; off the image: uncovered
struct PlaneAt {
  const Pos* pos;
  int h, w, y, x;
  Pos operator()(int dy, int dx) const {
    const int yy = y + dy, xx = x + dx;
    Pos none;
    none.x = kUncovered;
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
    fprintf(stderr, "usage: synth_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_all(argv[1], file) || file.size() < 44) return 2;
  int32_t head[5];
  uint32_t bg_color;
  Params prm;
  memcpy(head, file.data(), 20);
  memcpy(&bg_color, file.data() + 20, 4);
  memcpy(&prm, file.data() + 24, 20);
  const int hs = head[0], ws = head[1], h = head[2], w = head[3], has_bg = head[4];
  if (check_size(hs, ws, h, w) != DVD_OK) return refuse(DVD_E_SYNTH_SHAPE);
  if (check_params(prm) != DVD_OK) return refuse(DVD_E_SYNTH_PARAM);
  const size_t n = (size_t)h * w, ns = (size_t)hs * ws;
  if (file.size() != 44 + 3 * ns + 8 * n + (has_bg ? 3 * n : 0)) return 2;
  std::vector<uint8_t> scan(3 * ns), bg(has_bg ? 3 * n : 0);
  std::vector<float> fwd(2 * n);
  memcpy(scan.data(), file.data() + 44, 3 * ns);
  memcpy(fwd.data(), file.data() + 44 + 3 * ns, 8 * n);
  if (has_bg) memcpy(bg.data(), file.data() + 44 + 3 * ns + 8 * n, 3 * n);

  // stage_tile
  const float kx = axis_scale(ws, w), ky = axis_scale(hs, h);
  std::vector<Pos> pos(n);
  for (size_t p = 0; p < n; ++p) pos[p] = pos_of(fwd[2 * p], fwd[2 * p + 1], kx, ky, hs, ws);
  // render_kernel, footprint_kernel
  const bool shade_on = shading_on(prm);
  std::vector<uint8_t> photo(3 * n), radii(2 * n);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t p = (size_t)y * w + x;
      PlaneAt at;
      at.pos = pos.data();
      at.h = h;
      at.w = w;
      at.y = y;
      at.x = x;
      uint32_t back[3] = {bg_color & 255, (bg_color >> 8) & 255, (bg_color >> 16) & 255};
      if (has_bg)
        for (int q = 0; q < 3; ++q) back[q] = bg[3 * p + q];
      uint32_t rgb[3];
      pixel_at(scan.data(), hs, ws, at, x, y, h, w, back, prm, shade_on, rgb);
      for (int q = 0; q < 3; ++q) photo[3 * p + q] = (uint8_t)rgb[q];
      radii[2 * p] = radii[2 * p + 1] = 0;
      if (at(0, 0).x >= 0) {
        const Foot f = foot_at(at);
        radii[2 * p] = (uint8_t)f.rx;
        radii[2 * p + 1] = (uint8_t)f.ry;
      }
    }
  std::vector<uint8_t> out;
  append(out, photo.data(), 3 * n);
  append(out, radii.data(), 2 * n);
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
