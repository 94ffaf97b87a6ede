// Stand-alone CPU restatement of the kernels of clean.hip on the shared arithmetic of clean_core.h (plain C++, no HIP).
// tests/test_clean_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/clean_model.py.
//   clean_host_check in.bin out.bin
// in.bin : int32 h, w, cell, close, smooth, neutral, white, radius, kq; then img [h,w,3] u8.
// out.bin: the background [3,hc,wc] u8, the flattened page [h,w,3] u8, the Sauvola plane [h,w] u8 of the flattened page and
//          the one of img, and four counts as u64: saturated, floored, ink of the flattened page, ink of img.  Every buffer is
//          allocated at its exact size: a read or write past one is a sanitizer report.
// stdout : the status the entry points return for these arguments; a refusal writes nothing.
#include <string.h>

#include "clean_core.h"
#include "host_check_io.hpp"

using namespace dvd;
using namespace dvd::cl;

static int refuse(int status) {
  printf("%d\n", status);
  return 0;
}

// page_binarize_kernel: the plane and the ink count of g [h,w]
static unsigned long long binarize(const std::vector<uint8_t>& g, int h, int w, int r, int kq, std::vector<uint8_t>& out) {
  unsigned long long ink = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      uint32_t s1 = 0, s2 = 0;
      for (int yy = clip_lo(y, r); yy <= clip_hi(y, r, h); ++yy)
        for (int xx = clip_lo(x, r); xx <= clip_hi(x, r, w); ++xx) {
          const uint32_t v = g[(size_t)yy * w + xx];
          s1 += v;
          s2 += v * v;
        }
      const bool is_ink = sauvola_ink(g[(size_t)y * w + x], (uint32_t)(win_count(y, h, r) * win_count(x, w, r)), s1, s2, kq);
      out[(size_t)y * w + x] = is_ink ? 0 : 255;
      ink += is_ink;
    }
  return ink;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: clean_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_all(argv[1], file) || file.size() < 36) return 2;
  int32_t head[9];
  memcpy(head, file.data(), 36);
  const int h = head[0], w = head[1], s = head[2], close = head[3], smooth = head[4], neutral = head[5], white = head[6], radius = head[7],
            kq = head[8];
  if (check_page(h, w) != DVD_OK) return refuse(DVD_E_CLEAN_SHAPE);
  if (check_background(s, close, smooth) != DVD_OK || check_flatten(s, white) != DVD_OK || check_binarize(radius, kq) != DVD_OK)
    return refuse(DVD_E_CLEAN_PARAM);
  const size_t n = (size_t)h * w;
  if (file.size() != 36 + 3 * n) return 2;
  std::vector<uint8_t> img(file.begin() + 36, file.end());
  const int hc = coarse(h, s), wc = coarse(w, s);
  const size_t nc = (size_t)hc * wc;

  // page_cellmax_kernel
  std::vector<uint8_t> cmax(3 * nc, 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) {
        uint8_t& m = cmax[(c * (size_t)hc + y / s) * wc + x / s];
        const uint8_t v = img[3 * ((size_t)y * w + x) + c];
        m = m > v ? m : v;
      }
  // page_bg_kernel: maximum, minimum, tent - every window clipped to the plane
  std::vector<uint8_t> grown(3 * nc), closed(3 * nc), bg(3 * nc);
  for (int pass = 0; pass < 2; ++pass) {
    const std::vector<uint8_t>& src = pass ? grown : cmax;
    std::vector<uint8_t>& dst = pass ? closed : grown;
    for (int c = 0; c < 3; ++c)
      for (int y = 0; y < hc; ++y)
        for (int x = 0; x < wc; ++x) {
          int v = pass ? 255 : 0;
          for (int yy = clip_lo(y, close); yy <= clip_hi(y, close, hc); ++yy)
            for (int xx = clip_lo(x, close); xx <= clip_hi(x, close, wc); ++xx) {
              const int q = src[(c * (size_t)hc + yy) * wc + xx];
              v = pass ? (v < q ? v : q) : (v > q ? v : q);
            }
          dst[(c * (size_t)hc + y) * wc + x] = (uint8_t)v;
        }
  }
  for (int c = 0; c < 3; ++c)
    for (int y = 0; y < hc; ++y)
      for (int x = 0; x < wc; ++x) {
        uint32_t num = 0;
        for (int yy = clip_lo(y, smooth); yy <= clip_hi(y, smooth, hc); ++yy)
          for (int xx = clip_lo(x, smooth); xx <= clip_hi(x, smooth, wc); ++xx)
            num += tent_w(yy - y, smooth) * tent_w(xx - x, smooth) * closed[(c * (size_t)hc + yy) * wc + xx];
        bg[(c * (size_t)hc + y) * wc + x] = (uint8_t)bg_round(num, tent_den(x, wc, smooth) * tent_den(y, hc, smooth));
      }
  if (!neutral)
    for (size_t i = 0; i < nc; ++i) bg[i] = bg[nc + i] = bg[2 * nc + i] = (uint8_t)gray_of(bg[i], bg[nc + i], bg[2 * nc + i]);

  // page_flatten_kernel
  std::vector<uint8_t> page(3 * n), gray(n), gray_img(n), plane(n), plane_img(n);
  Counts cnt;
  cnt.saturated = cnt.floored = cnt.ink = 0;
  for (int y = 0; y < h; ++y) {
    const Axis ay = flat_axis(y, s, hc);
    for (int x = 0; x < w; ++x) {
      const Axis ax = flat_axis(x, s, wc);
      const size_t p = (size_t)y * w + x;
      for (int c = 0; c < 3; ++c) {
        const uint8_t* b = bg.data() + c * nc;
        const uint32_t q = bgq_of(b[(size_t)ay.i0 * wc + ax.i0], b[(size_t)ay.i0 * wc + ax.i1], b[(size_t)ay.i1 * wc + ax.i0],
                                  b[(size_t)ay.i1 * wc + ax.i1], ax.f, ay.f, s);
        page[3 * p + c] = (uint8_t)flatten_sample(img[3 * p + c], (uint32_t)white, s, q, cnt);
      }
      gray[p] = (uint8_t)gray_of(page[3 * p], page[3 * p + 1], page[3 * p + 2]);
      gray_img[p] = (uint8_t)gray_of(img[3 * p], img[3 * p + 1], img[3 * p + 2]);
    }
  }
  const unsigned long long ink = binarize(gray, h, w, radius, kq, plane), ink_img = binarize(gray_img, h, w, radius, kq, plane_img);
  const unsigned long long stats[4] = {cnt.saturated, cnt.floored, ink, ink_img};
  std::vector<uint8_t> out;
  append(out, bg.data(), 3 * nc);
  append(out, page.data(), 3 * n);
  append(out, plane.data(), n);
  append(out, plane_img.data(), n);
  append(out, stats, sizeof(stats));
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
