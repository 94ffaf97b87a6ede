// The local-distortion chain of sflow.hip as plain CPU loops on the shared arithmetic of sflow_core.h (no HIP): the functions of
// the stand-alone restatements sflow_host_check.cpp and adist_host_check.cpp, which the tests build under ASan/UBSan.
#pragma once
#include <stdio.h>
#include <string.h>

#include <vector>

#include "host_check_io.hpp"
#include "sflow_core.h"

using namespace dvd::sf;

typedef std::vector<uint8_t> Bytes;

// in.bin of both programs: int32 h, w, the ten int32 fields of dvd_sflow_params in their order, plane A, plane B.  Returns 0,
// 2 for a file that cannot be read or is too short, DVD_E_ARG for a refused shape or parameter (said on stderr).
static int read_pair(const char* path, int& h, int& w, dvd_sflow_params& pr, Bytes& a, Bytes& b) {
  Bytes in;
  int32_t head[12];
  if (!read_all(path, in) || in.size() < sizeof(head)) return 2;
  memcpy(head, in.data(), sizeof(head));
  h = head[0];
  w = head[1];
  memcpy(&pr, head + 2, sizeof(pr));
  static_assert(sizeof(dvd_sflow_params) == 10 * sizeof(int32_t), "ten int fields");
  const char* why = check_params(pr);
  if (!why) why = check_shape(h, w, pr);
  if (why) {
    fprintf(stderr, "refused: %s\n", why);
    return DVD_E_ARG;
  }
  const size_t hw = (size_t)h * w;
  if (in.size() - sizeof(head) < 2 * hw) return 2;
  a.assign(in.begin() + sizeof(head), in.begin() + sizeof(head) + hw);
  b.assign(in.begin() + sizeof(head) + hw, in.begin() + sizeof(head) + 2 * hw);
  return 0;
}

static Bytes dsift(const Bytes& img, int h, int w, int eps) {
  std::vector<int> r((size_t)h * w * 8), c((size_t)h * w * 8);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      int gx, gy;
      gradient(img.data(), h, w, y, x, &gx, &gy);
      for (int o = 0; o < 8; ++o) r[((size_t)y * w + x) * 8 + o] = response(gx, gy, o);
    }
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int o = 0; o < 8; ++o) {
        int s = 0;
        for (int a = -1; a <= 1; ++a)
          for (int b = -1; b <= 1; ++b) s += r[((size_t)clampi(y + a, h) * w + clampi(x + b, w)) * 8 + o];
        c[((size_t)y * w + x) * 8 + o] = s;
      }
  Bytes out((size_t)h * w * kDesc);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      int hist[kDesc];
      uint64_t ss = 0;
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
          for (int o = 0; o < 8; ++o) {
            const int v = c[((size_t)cell_at(y, i, h) * w + cell_at(x, j, w)) * 8 + o];
            hist[(4 * i + j) * 8 + o] = v;
            ss += (uint64_t)v * (uint64_t)v;
          }
      const uint32_t norm = isqrt64(ss);
      for (int k = 0; k < kDesc; ++k) out[((size_t)y * w + x) * kDesc + k] = (uint8_t)quantise(hist[k], norm, eps);
    }
  return out;
}

static Bytes reduce2(const Bytes& img, int h, int w) {
  const int oh = (h + 1) / 2, ow = (w + 1) / 2;
  Bytes out((size_t)oh * ow);
  for (int i = 0; i < oh; ++i)
    for (int j = 0; j < ow; ++j) out[(size_t)i * ow + j] = (uint8_t)reduce2_at(img.data(), h, w, i, j);
  return out;
}

static std::vector<uint16_t> cost_volume(const Bytes& da, const Bytes& db, const std::vector<int16_t>& off, int h, int w, int win,
                                         const dvd_sflow_params& pr) {
  const int n = 2 * win + 1, L = n * n;
  const size_t hw = (size_t)h * w;
  std::vector<uint16_t> cost(hw * L);
  for (size_t p = 0; p < hw; ++p) {
    const int y = (int)(p / w), x = (int)(p % w);
    uint32_t a[32];
    memcpy(a, &da[p * kDesc], kDesc);
    for (int lv = 0; lv < n; ++lv)
      for (int lu = 0; lu < n; ++lu) {
        const int fu = off[p] + lu - win, fv = off[hw + p] + lv - win, qx = x + fu, qy = y + fv;
        const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
        uint32_t s = 0;
        if (inside) {
          uint32_t b[32];
          memcpy(b, &db[((size_t)qy * w + qx) * kDesc], kDesc);
          s = sad128(a, b);
        }
        cost[p * L + (size_t)lv * n + lu] = (uint16_t)data_cost(inside, s, fu, fv, pr.gamma, pr.T);
      }
  }
  return cost;
}

// `iters` synchronous iterations, sender-side like the kernels; returns the buffer the last iteration wrote
static std::vector<uint16_t> propagate(const std::vector<uint16_t>& cost, const std::vector<int16_t>& off, int h, int w, int win,
                                       int iters, const dvd_sflow_params& pr) {
  const int n = 2 * win + 1, L = n * n;
  const size_t hw = (size_t)h * w;
  std::vector<uint16_t> msg[2] = {std::vector<uint16_t>(4 * hw * L, 0), std::vector<uint16_t>(4 * hw * L, 0)};
  std::vector<int> tot(L), hq(L), t(L), o(L);
  for (int it = 0; it < iters; ++it) {
    const std::vector<uint16_t>& in = msg[it & 1];
    std::vector<uint16_t>& out = msg[(it + 1) & 1];
    for (size_t q = 0; q < hw; ++q) {
      const int y = (int)(q / w), x = (int)(q % w);
      for (int i = 0; i < L; ++i) {
        tot[i] = cost[q * L + i];
        for (int k = 0; k < 4; ++k) tot[i] += in[((size_t)k * hw + q) * L + i];
      }
      for (int k = 0; k < 4; ++k) {
        int dy, dx, slot, excl;
        direction(k, &dy, &dx, &slot, &excl);
        const int py = y + dy, px = x + dx;
        if (py < 0 || py >= h || px < 0 || px >= w) continue;
        const size_t p = (size_t)py * w + px;
        const int du0 = off[p] - off[q], dv0 = off[hw + p] - off[hw + q];
        for (int i = 0; i < L; ++i) hq[i] = tot[i] - in[((size_t)excl * hw + q) * L + i];
        for (int i = 0; i < L; ++i) t[i] = minconv_u(hq, n, i / n, i % n, du0, pr.alpha, pr.d);
        int mn = 0x7fffffff;
        for (int i = 0; i < L; ++i) {
          o[i] = minconv_v(t, n, i / n, i % n, dv0, pr.alpha, pr.d);
          mn = mini(mn, o[i]);
        }
        for (int i = 0; i < L; ++i) out[((size_t)slot * hw + p) * L + i] = (uint16_t)(o[i] - mn);
      }
    }
  }
  return msg[iters & 1];
}

// the sum of blocks * 256 terms (padded with zeros) in the kernels' fixed order; the terms are used up
static double ordered_sum(std::vector<double>& len, size_t blocks) {
  std::vector<double> partials(blocks);
  for (size_t b = 0; b < blocks; ++b) {                 // per wave a butterfly tree, then the four waves in order
    double wave[kSelBlock / 64];
    for (int wv = 0; wv < kSelBlock / 64; ++wv) {
      double* v = &len[b * kSelBlock + (size_t)wv * 64];
      for (int s = 32; s >= 1; s >>= 1)
        for (int i = 0; i < s; ++i) v[i] += v[i + s];
      wave[wv] = v[0];
    }
    partials[b] = ((wave[0] + wave[1]) + wave[2]) + wave[3];
  }
  double red[kFinThreads];                               // lane t: partials t, t + 256, ... in order; then a tree
  for (int t = 0; t < kFinThreads; ++t) {
    double a = 0.0;
    for (size_t i = t; i < blocks; i += kFinThreads) a += partials[i];
    red[t] = a;
  }
  for (int s = kFinThreads / 2; s >= 1; s >>= 1)
    for (int i = 0; i < s; ++i) red[i] += red[i + s];
  return red[0];
}

// the belief's argmin (the smallest label index on ties) as the absolute flow; returns the LD sum in the kernels' order
static double select_flow(const std::vector<uint16_t>& cost, const std::vector<uint16_t>& msg, const std::vector<int16_t>& off,
                          int h, int w, int win, std::vector<int16_t>& flow) {
  const int n = 2 * win + 1, L = n * n;
  const size_t hw = (size_t)h * w;
  const size_t blocks = (hw + kSelBlock - 1) / kSelBlock;
  std::vector<double> len(blocks * kSelBlock, 0.0);
  flow.assign(2 * hw, 0);
  for (size_t p = 0; p < hw; ++p) {
    int best = 0x7fffffff, arg = 0;
    for (int i = 0; i < L; ++i) {
      int b = cost[p * L + i];
      for (int k = 0; k < 4; ++k) b += msg[((size_t)k * hw + p) * L + i];
      if (b < best) { best = b; arg = i; }
    }
    const int fu = off[p] + arg % n - win, fv = off[hw + p] + arg / n - win;
    flow[p] = (int16_t)fu;
    flow[hw + p] = (int16_t)fv;
    len[p] = flow_length(fu, fv);
  }
  return ordered_sum(len, blocks) / (double)hw;
}

// The whole chain for one pair of u8 planes (parameters and shape already checked): the flow [2,h,w] and LD; on request the
// descriptors of A on level 0 and the top level's cost volume.
static double chain(const Bytes& a, const Bytes& b, int h, int w, const dvd_sflow_params& pr, std::vector<int16_t>& flow,
                    Bytes* da0 = nullptr, std::vector<uint16_t>* top_cost = nullptr) {
  std::vector<Bytes> pa(pr.levels), pb(pr.levels);
  pa[0] = a;
  pb[0] = b;
  const LevelDims dm = level_dims(h, w, pr.levels);
  for (int l = 1; l < pr.levels; ++l) {
    pa[l] = reduce2(pa[l - 1], dm.h[l - 1], dm.w[l - 1]);
    pb[l] = reduce2(pb[l - 1], dm.h[l - 1], dm.w[l - 1]);
  }
  std::vector<int16_t> coarse;
  double ld = 0.0;
  for (int l = pr.levels - 1; l >= 0; --l) {
    const int lh = dm.h[l], lw = dm.w[l], win = level_win(pr, l);
    const size_t lhw = (size_t)lh * lw;
    const Bytes da = dsift(pa[l], lh, lw, pr.eps), db = dsift(pb[l], lh, lw, pr.eps);
    std::vector<int16_t> off(2 * lhw, 0);
    if (l != pr.levels - 1) {
      const size_t chw = (size_t)dm.h[l + 1] * dm.w[l + 1];
      for (int y = 0; y < lh; ++y)
        for (int x = 0; x < lw; ++x) {
          const size_t q = (size_t)(y >> 1) * dm.w[l + 1] + (x >> 1);
          off[(size_t)y * lw + x] = (int16_t)(2 * coarse[q]);
          off[lhw + (size_t)y * lw + x] = (int16_t)(2 * coarse[chw + q]);
        }
    }
    const std::vector<uint16_t> cost = cost_volume(da, db, off, lh, lw, win, pr);
    const std::vector<uint16_t> msg = propagate(cost, off, lh, lw, win, level_iters(pr, l), pr);
    ld = select_flow(cost, msg, off, lh, lw, win, flow);
    coarse = flow;
    if (l == pr.levels - 1 && top_cost) *top_cost = cost;
    if (l == 0 && da0) *da0 = da;
  }
  return ld;
}
