// The arithmetic of the map inverse: the page's triangle mesh rasterised on the photograph, the forward
// map photograph pixel -> page position, its cycle error, the mesh picture and the point transfers.  Shared by the kernels of
// mapinv.hip and by the stand-alone CPU restatement mapinv_host_check.cpp (plain C++, no HIP); tests/mapinv_model.py is its
// NumPy statement and the definition.  Vertices are Q8 integers and the edge functions exact int64; every f32 operation is
// rounded on its own (noise_core.h's helpers); the vertex positions are flowgrid_core.h's, the unwarp tail's own.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dvd_hip.h"

#include "flowgrid_core.h"
#include "hd.h"
#include "noise_core.h"

namespace dvd {
namespace mi {

using nz::bits_of;
using nz::fadd;
using nz::fdiv;
using nz::float_of;
using nz::fmul;
using nz::fsqrt;
using nz::fsub;

constexpr int kMaxSide = 16384, kMinGrid = 2, kMaxGrid = 8192;
constexpr int kBlock = 256, kPer = 4;                  // threads of a workgroup; pixels of a thread in the per-pixel passes
constexpr uint32_t kInvalid = 0xffffffffu;             // the winner of an uncovered pixel, and both components of fwd there
constexpr float kCoordCap = 4194304.f;                 // 2^22: a vertex further out is invalid; its Q8 integer stays below 2^31
constexpr int kStats = 6;                              // covered, fold_px, flipped_tris, degenerate_tris, skipped_tris, tris
constexpr int kCycleWords = 3;                         // n, the bits of the f64 sum, the bits of the f32 maximum
enum Kind { kPlain = 0, kFlipped = 1, kDegenerate = 2, kSkipped = 3 };

struct Vertex {
  int32_t x, y;      // Q8 photograph position
};

// The lattice of a page of h x w: rows 0, step, 2 step, .. and h - 1 appended when it is no multiple of step; columns likewise.
struct Mesh {
  int h, w, step, rows, cols;
  long budget;       // the most pixels a triangle's clipped box may hold
};
DVD_HD int lattice_count(int n, int step) { return (n - 1) / step + 1 + ((n - 1) % step != 0); }
DVD_HD int lattice_at(int k, int n, int step) {
  const long p = (long)k * step;
  return p < n - 1 ? (int)p : n - 1;
}
inline Mesh make_mesh(int h, int w, int step) {
  Mesh m;
  m.h = h;
  m.w = w;
  m.step = step;
  m.rows = lattice_count(h, step);
  m.cols = lattice_count(w, step);
  const long b = 64l * step * step;
  m.budget = b > 1024 ? b : 1024;
  return m;
}
DVD_HD long mesh_tris(const Mesh& m) { return 2l * (m.rows - 1) * (m.cols - 1); }

DVD_HD bool finite1(float x) { return (bits_of(x) & 0x7f800000u) != 0x7f800000u; }

// The photograph position the unwarp tail samples for page pixel (i, j): flow_grid_at, un-normalised as
// grid_sample(align_corners=True) does.
DVD_HD void position_at(const float* flow, const UpParams& up, int i, int j, float* x, float* y) {
  float gx, gy;
  flow_grid_at(flow, up, i, j, gx, gy);
  *x = fmul(fmul(fadd(gx, 1.f), 0.5f), (float)(up.w - 1));
  *y = fmul(fmul(fadd(gy, 1.f), 0.5f), (float)(up.h - 1));
}
// ... quantised: rint(256 x).  Returns whether the vertex is valid; an invalid one is (0, 0).
DVD_HD bool vertex_at(const float* flow, const UpParams& up, int i, int j, Vertex* v) {
  float x, y;
  position_at(flow, up, i, j, &x, &y);
  const bool ok = finite1(x) && finite1(y) && fabsf(x) <= kCoordCap && fabsf(y) <= kCoordCap;
  v->x = ok ? (int32_t)rintf(fmul(x, 256.f)) : 0;
  v->y = ok ? (int32_t)rintf(fmul(y, 256.f)) : 0;
  return ok;
}

// ---- triangles ----------------------------------------------------------------------------------------------------------------
DVD_HD long long edge_fn(long long ax, long long ay, long long bx, long long by, long long px, long long py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
// whether a pixel exactly on the edge a -> b belongs to the triangle (positive area, y down): the edge runs upward, or it is
// horizontal and runs to the right
DVD_HD bool top_left(const Vertex& a, const Vertex& b) { return b.y < a.y || (b.y == a.y && b.x > a.x); }

struct Tri {
  Vertex v[3];           // after the swap of a flipped triangle: positive area
  int pu[3], pv[3];      // the page pixels of the vertices
  long long area;
  int kind;
  int xmin, xmax, ymin, ymax;      // the clipped box; empty when xmin > xmax or ymin > ymax
};
DVD_HD int imin3(int a, int b, int c) {
  const int m = a < b ? a : b;
  return m < c ? m : c;
}
DVD_HD int imax3(int a, int b, int c) {
  const int m = a > b ? a : b;
  return m > c ? m : c;
}
// Triangle `id` = 2 cell + {0, 1} of the mesh, cells in row-major order: (a, b, c) and (c, b, d), a upper left, b upper right,
// c lower left, d lower right.
DVD_HD Tri make_tri(const Mesh& m, const Vertex* verts, const uint8_t* valid, long id) {
  const long cell = id >> 1;
  const int r = (int)(cell / (m.cols - 1)), c = (int)(cell - (long)r * (m.cols - 1));
  int rr[3], cc[3];
  if (id & 1) {
    rr[0] = r + 1; cc[0] = c; rr[1] = r; cc[1] = c + 1; rr[2] = r + 1; cc[2] = c + 1;
  } else {
    rr[0] = r; cc[0] = c; rr[1] = r; cc[1] = c + 1; rr[2] = r + 1; cc[2] = c;
  }
  Tri t;
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const long at = (long)rr[k] * m.cols + cc[k];
    t.v[k] = verts[at];
    ok = ok && valid[at] != 0;
    t.pu[k] = lattice_at(cc[k], m.w, m.step);
    t.pv[k] = lattice_at(rr[k], m.h, m.step);
  }
  t.area = edge_fn(t.v[0].x, t.v[0].y, t.v[1].x, t.v[1].y, t.v[2].x, t.v[2].y);
  const bool flip = ok && t.area < 0;
  if (flip) {
    const Vertex v = t.v[1];
    t.v[1] = t.v[2];
    t.v[2] = v;
    int s = t.pu[1];
    t.pu[1] = t.pu[2];
    t.pu[2] = s;
    s = t.pv[1];
    t.pv[1] = t.pv[2];
    t.pv[2] = s;
    t.area = -t.area;
  }
  const int x0 = (imin3(t.v[0].x, t.v[1].x, t.v[2].x) + 255) >> 8, x1 = imax3(t.v[0].x, t.v[1].x, t.v[2].x) >> 8;
  const int y0 = (imin3(t.v[0].y, t.v[1].y, t.v[2].y) + 255) >> 8, y1 = imax3(t.v[0].y, t.v[1].y, t.v[2].y) >> 8;
  t.xmin = x0 > 0 ? x0 : 0;
  t.xmax = x1 < m.w - 1 ? x1 : m.w - 1;
  t.ymin = y0 > 0 ? y0 : 0;
  t.ymax = y1 < m.h - 1 ? y1 : m.h - 1;
  const long bw = t.xmax >= t.xmin ? t.xmax - t.xmin + 1 : 0, bh = t.ymax >= t.ymin ? t.ymax - t.ymin + 1 : 0;
  t.kind = !ok ? kSkipped : (t.area == 0 ? kDegenerate : (bw * bh > m.budget ? kSkipped : (flip ? kFlipped : kPlain)));
  if (t.kind >= kDegenerate) t.xmax = t.xmin - 1;        // covers nothing
  return t;
}
// The three edge values of pixel (px, py): e[0] of edge v0 -> v1 (the weight of v2), e[1] of v1 -> v2 (of v0), e[2] of v2 -> v0
// (of v1).  Returns whether the triangle covers the pixel.
DVD_HD bool tri_covers(const Tri& t, int px, int py, long long* e) {
  const long long X = 256ll * px, Y = 256ll * py;
  bool in = true;
  for (int k = 0; k < 3; ++k) {
    const Vertex& a = t.v[k];
    const Vertex& b = t.v[k == 2 ? 0 : k + 1];
    e[k] = edge_fn(a.x, a.y, b.x, b.y, X, Y);
    in = in && (e[k] > 0 || (e[k] == 0 && top_left(a, b)));
  }
  return in;
}
// the page position of a covered pixel from the winner's edge values
DVD_HD void tri_page(const Tri& t, const long long* e, float* u, float* v) {
  const float area = (float)t.area;
  const float wb = fdiv((float)e[2], area), wc = fdiv((float)e[0], area);
  *u = fadd((float)t.pu[0], fadd(fmul(wb, (float)(t.pu[1] - t.pu[0])), fmul(wc, (float)(t.pu[2] - t.pu[0]))));
  *v = fadd((float)t.pv[0], fadd(fmul(wb, (float)(t.pv[1] - t.pv[0])), fmul(wc, (float)(t.pv[2] - t.pv[0]))));
}

// ---- the backward map at a fractional page position ---------------------------------------------------------------------------
DVD_HD void axis_taps(float u, int n, int* i0, int* i1, float* l0, float* l1) {
  const float uc = fminf(fmaxf(u, 0.f), (float)(n - 1));
  const int f = (int)uc;
  *i0 = f < n - 1 ? f : n - 1;
  *i1 = *i0 + 1 < n - 1 ? *i0 + 1 : n - 1;
  *l1 = fsub(uc, (float)*i0);
  *l0 = fsub(1.f, *l1);
}
DVD_HD float blend4(float p00, float p01, float p10, float p11, float lx0, float lx1, float ly0, float ly1) {
  const float t0 = fadd(fmul(p00, lx0), fmul(p01, lx1)), t1 = fadd(fmul(p10, lx0), fmul(p11, lx1));
  return fadd(fmul(t0, ly0), fmul(t1, ly1));
}
// Bilinear over the four surrounding page pixels' photograph positions; a position outside the page is clamped to it.
// Returns false (and leaves x, y alone) when u or v is not finite.
DVD_HD bool backward_at(const float* flow, const UpParams& up, float u, float v, float* x, float* y) {
  if (!finite1(u) || !finite1(v)) return false;
  int i0, i1, j0, j1;
  float lx0, lx1, ly0, ly1, px[4], py[4];
  axis_taps(u, up.w, &j0, &j1, &lx0, &lx1);
  axis_taps(v, up.h, &i0, &i1, &ly0, &ly1);
  position_at(flow, up, i0, j0, &px[0], &py[0]);
  position_at(flow, up, i0, j1, &px[1], &py[1]);
  position_at(flow, up, i1, j0, &px[2], &py[2]);
  position_at(flow, up, i1, j1, &px[3], &py[3]);
  *x = blend4(px[0], px[1], px[2], px[3], lx0, lx1, ly0, ly1);
  *y = blend4(py[0], py[1], py[2], py[3], lx0, lx1, ly0, ly1);
  return true;
}
// |backward(fwd(p)) - p| of a covered pixel; *ok = it is finite
DVD_HD float cycle_at(const float* flow, const UpParams& up, float u, float v, int px, int py, bool* ok) {
  float x = 0.f, y = 0.f;
  backward_at(flow, up, u, v, &x, &y);
  const float dx = fsub(x, (float)px), dy = fsub(y, (float)py);
  const float d = fsqrt(fadd(fmul(dx, dx), fmul(dy, dy)));
  *ok = finite1(d);
  return d;
}

// ---- fwd as the other passes read it --------------------------------------------------------------------------------------------
DVD_HD bool covered_at(const float* fwd, int w, int y, int x) { return bits_of(fwd[2 * ((size_t)y * w + x)]) != kInvalid; }

// photograph position -> page position: fwd sampled bilinearly.  False where the point is outside the photograph, not finite,
// or a tap is uncovered.
DVD_HD bool transfer_at(const float* fwd, int h, int w, float x, float y, float* u, float* v) {
  if (!(x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1))) return false;
  int i0, i1, j0, j1;
  float lx0, lx1, ly0, ly1;
  axis_taps(x, w, &j0, &j1, &lx0, &lx1);
  axis_taps(y, h, &i0, &i1, &ly0, &ly1);
  if (!covered_at(fwd, w, i0, j0) || !covered_at(fwd, w, i0, j1) || !covered_at(fwd, w, i1, j0) || !covered_at(fwd, w, i1, j1)) return false;
  const float* a = fwd + 2 * ((size_t)i0 * w + j0);
  const float* b = fwd + 2 * ((size_t)i0 * w + j1);
  const float* c = fwd + 2 * ((size_t)i1 * w + j0);
  const float* d = fwd + 2 * ((size_t)i1 * w + j1);
  *u = blend4(a[0], b[0], c[0], d[0], lx0, lx1, ly0, ly1);
  *v = blend4(a[1], b[1], c[1], d[1], lx0, lx1, ly0, ly1);
  return true;
}

// ---- the mesh picture -----------------------------------------------------------------------------------------------------------
struct Overlay {
  int h, w, lines, thickness, dim;
  uint32_t color, outline;          // 0x00BBGGRR
};
DVD_HD void line_index(const float* fwd, const Overlay& o, int y, int x, int* ku, int* kv) {
  const float* p = fwd + 2 * ((size_t)y * o.w + x);
  *ku = (int)floorf(fdiv(fmul(p[0], (float)(o.lines - 1)), (float)(o.w > 1 ? o.w - 1 : 1)));
  *kv = (int)floorf(fdiv(fmul(p[1], (float)(o.lines - 1)), (float)(o.h > 1 ? o.h - 1 : 1)));
}
// bit 0: (y, x) is on a grid line - its line index differs from its covered right or lower neighbour's; bit 1: it is on the
// outline - covered with a 4-neighbour that is uncovered or off the image
DVD_HD int base_marks(const float* fwd, const Overlay& o, int y, int x) {
  if (!covered_at(fwd, o.w, y, x)) return 0;
  int ku, kv, nu, nv, marks = 0;
  line_index(fwd, o, y, x, &ku, &kv);
  const bool right = x + 1 < o.w && covered_at(fwd, o.w, y, x + 1), down = y + 1 < o.h && covered_at(fwd, o.w, y + 1, x);
  if (right) {
    line_index(fwd, o, y, x + 1, &nu, &nv);
    if (nu != ku || nv != kv) marks |= 1;
  }
  if (down) {
    line_index(fwd, o, y + 1, x, &nu, &nv);
    if (nu != ku || nv != kv) marks |= 1;
  }
  const bool left = x > 0 && covered_at(fwd, o.w, y, x - 1), up = y > 0 && covered_at(fwd, o.w, y - 1, x);
  if (!(right && down && left && up)) marks |= 2;
  return marks;
}
// the three bytes of output pixel (y, x): the window rows and columns p - (t - 1) / 2 .. p + t / 2
DVD_HD void overlay_at(const uint8_t* src, const float* fwd, const Overlay& o, int y, int x, uint8_t* rgb) {
  const int lo = (o.thickness - 1) / 2, hi = o.thickness / 2;
  int marks = 0;
  for (int dy = -lo; dy <= hi; ++dy)
    for (int dx = -lo; dx <= hi; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if (yy >= 0 && yy < o.h && xx >= 0 && xx < o.w) marks |= base_marks(fwd, o, yy, xx);
    }
  const uint8_t* s = src + 3 * ((size_t)y * o.w + x);
  const int shift = o.dim && !covered_at(fwd, o.w, y, x) ? 1 : 0;
  for (int ch = 0; ch < 3; ++ch) {
    uint8_t b = (uint8_t)(s[ch] >> shift);
    if (marks & 1) b = (uint8_t)(o.color >> (8 * ch));
    if (marks & 2) b = (uint8_t)(o.outline >> (8 * ch));
    rgb[ch] = b;
  }
}

// ---- the workspace: byte offsets of its parts (every part 256-byte aligned) ------------------------------------------------------
struct Layout {
  long verts, valid, winner, multi, tri_part, px_part, cycle_part, total;
};
inline long up256(long x) { return (x + 255) & ~255l; }
inline long pixel_blocks(long n) { return (n + kBlock * kPer - 1) / (kBlock * kPer); }
inline long tri_blocks(long tris) { return tris > 0 ? (tris + kBlock - 1) / kBlock : 1; }
inline Layout layout(const Mesh& m) {
  const long nv = (long)m.rows * m.cols, n = (long)m.h * m.w;
  Layout l;
  l.cycle_part = 0;                  // first, and a function of h w alone: dvd_map_cycle_error takes the workspace of any step
  l.px_part = up256(l.cycle_part + pixel_blocks(n) * kCycleWords * 8);
  l.winner = up256(l.px_part + pixel_blocks(n) * 2 * 8);
  l.multi = up256(l.winner + 4 * n);
  l.verts = up256(l.multi + n);
  l.valid = up256(l.verts + 8 * nv);
  l.tri_part = up256(l.valid + nv);
  l.total = up256(l.tri_part + tri_blocks(mesh_tris(m)) * 3 * 8);
  return l;
}

// ---- the argument checks of the entry points (no pointers), shared with the restatement ----------------------------------------
inline int check_size(int h, int w) { return h < 1 || w < 1 || h > kMaxSide || w > kMaxSide ? DVD_E_INV_SHAPE : DVD_OK; }
inline int check_grid(int g) { return g < kMinGrid || g > kMaxGrid ? DVD_E_INV_SHAPE : DVD_OK; }
inline int check_step(int step) { return step < 1 || step > kMaxSide ? DVD_E_INV_STEP : DVD_OK; }
inline int check_overlay(int lines, int thickness) { return lines < 2 || lines > kMaxSide || thickness < 1 || thickness > 3 ? DVD_E_INV_LINES : DVD_OK; }

}  // namespace mi
}  // namespace dvd
