// Stand-alone CPU restatement of the kernels of mapinv.hip on the shared arithmetic of mapinv_core.h (plain C++, no HIP).
// tests/test_mapinv_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/mapinv_model.py.
//   mapinv_host_check in.bin out.bin
// in.bin : int32 g, h, w, step, lines, thickness, dim, n_photo, n_page; uint32 color, outline; f32 scale; then flow [2,g,g] f32,
//          n_photo points (x, y) f32 on the photograph, n_page points (u, v) f32 on the page, and src [h,w,3] u8
// out.bin: the lattice's vertices [rows cols] (int32 x, y) and validity bytes, fwd [h,w,2] f32, the six u64 of dvd_map_invert,
//          the three 8-byte words of dvd_map_cycle_error, the picture [h,w,3] u8, the transferred points [n_photo,2] f32 and the
//          mapped points [n_page,2] f32.  Every buffer is allocated at its exact size: a write past one is a sanitizer report.
// stdout : the status the entry points return for these arguments; a refusal writes nothing.
#include <string.h>

#include "mapinv_core.h"
#include "host_check_io.hpp"

using namespace dvd;
using namespace dvd::mi;

static int refuse(int status) {
  printf("%d\n", status);
  return 0;
}

// an f64 sum in the order of cycle_kernel and cycle_finalize_kernel
static double wave_sum64(const double* lane) {
  double v[64];
  memcpy(v, lane, sizeof v);
  for (int d = 32; d >= 1; d >>= 1)
    for (int i = 0; i < d; ++i) v[i] += v[i + d];
  return v[0];
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: mapinv_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_all(argv[1], file) || file.size() < 48) return 2;
  int32_t head[9];
  uint32_t colors[2];
  float scale;
  memcpy(head, file.data(), 36);
  memcpy(colors, file.data() + 36, 8);
  memcpy(&scale, file.data() + 44, 4);
  const int g = head[0], h = head[1], w = head[2], step = head[3], lines = head[4], thickness = head[5], dim = head[6];
  const long n_photo = head[7], n_page = head[8];
  if (check_size(h, w) != DVD_OK || check_grid(g) != DVD_OK) return refuse(DVD_E_INV_SHAPE);
  if (check_step(step) != DVD_OK) return refuse(DVD_E_INV_STEP);
  if (check_overlay(lines, thickness) != DVD_OK) return refuse(DVD_E_INV_LINES);
  if (n_photo < 0 || n_page < 0) return refuse(DVD_E_INV_POINTS);
  const size_t n = (size_t)h * w, gg = (size_t)2 * g * g;
  if (file.size() != 48 + 4 * gg + 8 * (size_t)(n_photo + n_page) + 3 * n) return 2;
  std::vector<float> flow(gg), photo(2 * n_photo), page(2 * n_page);
  std::vector<uint8_t> src(3 * n);
  const uint8_t* at = file.data() + 48;
  memcpy(flow.data(), at, 4 * gg);
  at += 4 * gg;
  if (n_photo) memcpy(photo.data(), at, 8 * n_photo);
  at += 8 * n_photo;
  if (n_page) memcpy(page.data(), at, 8 * n_page);
  at += 8 * n_page;
  memcpy(src.data(), at, 3 * n);

  const Mesh m = make_mesh(h, w, step);
  const UpParams up = make_up(g, h, w, scale);
  const long nv = (long)m.rows * m.cols, tris = mesh_tris(m);
  // lattice_kernel
  std::vector<Vertex> verts(nv);
  std::vector<uint8_t> valid(nv);
  for (long k = 0; k < nv; ++k) {
    const int r = (int)(k / m.cols), c = (int)(k - (long)r * m.cols);
    valid[k] = vertex_at(flow.data(), up, lattice_at(r, m.h, m.step), lattice_at(c, m.w, m.step), &verts[k]) ? 1 : 0;
  }
  // fill_kernel, raster_kernel
  std::vector<uint32_t> winner(n, kInvalid);
  std::vector<uint8_t> multi(n, 0);
  unsigned long long stats[kStats] = {0, 0, 0, 0, 0, (unsigned long long)tris};
  for (long id = 0; id < tris; ++id) {
    const Tri t = make_tri(m, verts.data(), valid.data(), id);
    stats[2] += t.kind == kFlipped;
    stats[3] += t.kind == kDegenerate;
    stats[4] += t.kind == kSkipped;
    for (int y = t.ymin; y <= t.ymax; ++y)
      for (int x = t.xmin; x <= t.xmax; ++x) {
        long long e[3];
        if (!tri_covers(t, x, y, e)) continue;
        uint32_t& slot = winner.at((size_t)y * w + x);
        if (slot != kInvalid) multi[(size_t)y * w + x] = 1;
        if ((uint32_t)id < slot) slot = (uint32_t)id;
      }
  }
  // resolve_kernel
  std::vector<float> fwd(2 * n);
  for (size_t p = 0; p < n; ++p) {
    float u = float_of(kInvalid), v = float_of(kInvalid);
    if (winner[p] != kInvalid) {
      const Tri t = make_tri(m, verts.data(), valid.data(), (long)winner[p]);
      long long e[3];
      tri_covers(t, (int)(p % w), (int)(p / w), e);
      tri_page(t, e, &u, &v);
      stats[0] += 1;
      stats[1] += multi[p];
    }
    fwd[2 * p] = u;
    fwd[2 * p + 1] = v;
  }
  // cycle_kernel, cycle_finalize_kernel
  const long blocks = pixel_blocks((long)n);
  std::vector<double> part(blocks, 0.0);
  unsigned long long cyc_n = 0;
  uint32_t top = 0;
  for (long b = 0; b < blocks; ++b) {
    double lane[kBlock];
    for (int t = 0; t < kBlock; ++t) {
      lane[t] = 0.0;
      for (int k = 0; k < kPer; ++k) {
        const size_t p = ((size_t)b * kPer + k) * kBlock + t;
        if (p >= n || bits_of(fwd[2 * p]) == kInvalid) continue;
        bool ok;
        const float d = cycle_at(flow.data(), up, fwd[2 * p], fwd[2 * p + 1], (int)(p % w), (int)(p / w), &ok);
        if (!ok) continue;
        cyc_n += 1;
        lane[t] += (double)d;
        top = bits_of(d) > top ? bits_of(d) : top;
      }
    }
    part[b] = ((wave_sum64(lane) + wave_sum64(lane + 64)) + wave_sum64(lane + 128)) + wave_sum64(lane + 192);
  }
  double lane[kBlock];
  for (int t = 0; t < kBlock; ++t) {
    lane[t] = 0.0;
    for (long b = t; b < blocks; b += kBlock) lane[t] += part[b];
  }
  for (int st = kBlock / 2; st >= 1; st >>= 1)
    for (int t = 0; t < st; ++t) lane[t] += lane[t + st];
  unsigned long long cycle[kCycleWords] = {cyc_n, 0, top};
  memcpy(&cycle[1], &lane[0], 8);
  // overlay_kernel
  Overlay o;
  o.h = h;
  o.w = w;
  o.lines = lines;
  o.thickness = thickness;
  o.dim = dim != 0;
  o.color = colors[0];
  o.outline = colors[1];
  std::vector<uint8_t> picture(3 * n);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) overlay_at(src.data(), fwd.data(), o, y, x, &picture[3 * ((size_t)y * w + x)]);
  // the point kernels
  std::vector<float> to_page(2 * n_photo), to_photo(2 * n_page);
  for (long i = 0; i < n_photo; ++i) {
    float u = 0.f, v = 0.f;
    const bool ok = transfer_at(fwd.data(), h, w, photo[2 * i], photo[2 * i + 1], &u, &v);
    to_page[2 * i] = ok ? u : float_of(kInvalid);
    to_page[2 * i + 1] = ok ? v : float_of(kInvalid);
  }
  for (long i = 0; i < n_page; ++i) {
    float x = 0.f, y = 0.f;
    const bool ok = backward_at(flow.data(), up, page[2 * i], page[2 * i + 1], &x, &y);
    to_photo[2 * i] = ok ? x : float_of(kInvalid);
    to_photo[2 * i + 1] = ok ? y : float_of(kInvalid);
  }
  std::vector<uint8_t> out;
  append(out, verts.data(), 8 * (size_t)nv);
  append(out, valid.data(), (size_t)nv);
  append(out, fwd.data(), 8 * n);
  append(out, stats, sizeof stats);
  append(out, cycle, sizeof cycle);
  append(out, picture.data(), 3 * n);
  append(out, to_page.data(), 8 * (size_t)n_photo);
  append(out, to_photo.data(), 8 * (size_t)n_page);
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
