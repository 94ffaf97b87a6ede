// Stand-alone CPU restatement of the kernels of mapscore.hip on the shared arithmetic of mapscore_core.h (plain C++, no HIP).
// tests/test_mapscore_cpu.py builds it with -fsanitize=address,undefined and holds its output to tests/mapscore_model.py.
//   mapscore_host_check in.bin out.bin
// in.bin : int32 mode, then
//   mode 0 (a document)     : int32 g, gt_g, n_hyp, h, w; flow [2,g,g] f32 or, g = 0, [h,w,2]; the ground truth, [h,w,2] f32 (gt_g = 0) or
//                             [2,gt_g,gt_g]; with n_hyp >= 2 the hypotheses [n_hyp,2,g,g]
//   mode 1 (dvd_select_u32) : int32 n, k; ranks [k] u32; keys [n] u32
// out.bin: mode 0 the planes e [h w] and sigma [h w] u32, the seven 8-byte words of dvd_map_metrics and, with a valid pixel,
//          for key = sigma and then key = e: the 50 thresholds u32 and the bins [51][4] u64; mode 1 the k selected keys
// stdout : the status the entry point returns for these arguments; a refusal writes nothing.
#include <string.h>

#include <algorithm>

#include "mapscore_core.h"
#include "host_check_io.hpp"

using namespace dvd::ms;

// dvd_select_u32 as the two kernels do it: four levels; per level the histograms of the live slots, then every rank's digit
static void select_u32(const uint32_t* keys, long n, const uint32_t* ranks, int k, uint32_t* out) {
  SelState st;
  memset(&st, 0, sizeof st);
  std::vector<uint32_t> hist((size_t)kMaxRanks * 256);
  for (int level = 0; level < 4; ++level) {
    const uint32_t* prefix = st.prefix[level & 1];
    uint32_t table[kMaxRanks];
    int unused = 0;
    const int nslots = level ? sel_slots(prefix, k, 0, table, &unused) : 1;
    std::fill(hist.begin(), hist.end(), 0u);
    for (long p = 0; p < n; ++p) {
      const int slot = level ? sel_slot(table, nslots, sel_prefix(keys[p], level)) : 0;
      if (slot >= 0) hist[(size_t)slot * 256 + sel_digit(keys[p], level)] += 1;
    }
    for (int r = 0; r < k; ++r) {
      int slot = 0;
      if (level) sel_slots(prefix, k, r, table, &slot);
      uint32_t rem = level ? st.rem[level & 1][r] : ranks[r];
      const uint32_t now = ((level ? prefix[r] : 0u) << 8) | sel_walk(hist.data() + (size_t)slot * 256, &rem);
      st.prefix[(level + 1) & 1][r] = now;
      st.rem[(level + 1) & 1][r] = rem;
    }
  }
  for (int r = 0; r < k; ++r) out[r] = st.prefix[0][r];
}

static int refuse(int status) {
  printf("%d\n", status);
  return 0;
}

// the thresholds of one key plane (descending ranks hi of the valid keys = ascending ranks n_valid - 1 - hi) and its bins
static void sparsify(const std::vector<uint32_t>& e, const std::vector<uint32_t>& key, unsigned long long n_valid,
                     std::vector<uint8_t>& out) {
  uint32_t asc[kMaxRanks], sel[kMaxRanks], thr[kMaxRanks];
  for (int t = 0; t < kMaxRanks; ++t) {
    const unsigned long long hi = (2ull * t * (n_valid - 1) + 99) / 100;
    asc[kMaxRanks - 1 - t] = (uint32_t)(n_valid - 1 - hi);
  }
  select_u32(key.data(), (long)key.size(), asc, kMaxRanks, sel);
  for (int t = 0; t < kMaxRanks; ++t) thr[t] = sel[kMaxRanks - 1 - t];
  unsigned long long bins[(kMaxRanks + 1) * kBinWords];
  memset(bins, 0, sizeof bins);
  for (size_t p = 0; p < e.size(); ++p) {
    if (e[p] == kInvalid) continue;
    const float ev = float_of(e[p]);
    unsigned long long* b = bins + bin_of(thr, kMaxRanks, key[p]) * kBinWords;
    b[0] += 1;
    b[1] += ev <= 1.f;
    b[2] += ev <= 5.f;
    b[3] += fixed_of(ev);
  }
  append(out, thr, sizeof thr);
  append(out, bins, sizeof bins);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: mapscore_host_check in.bin out.bin\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_all(argv[1], file) || file.size() < 4) return 2;
  int32_t mode;
  memcpy(&mode, file.data(), 4);
  const size_t words = mode == 0 ? 5 : (mode == 1 ? 2 : 0);
  if (!words || file.size() < 4 + 4 * words || (file.size() - 4 - 4 * words) % 4) return 2;
  int32_t head[5] = {0, 0, 0, 0, 0};
  memcpy(head, file.data() + 4, 4 * words);
  const size_t body_words = (file.size() - 4 - 4 * words) / 4;
  std::vector<uint32_t> body(body_words);
  if (body_words) memcpy(body.data(), file.data() + 4 + 4 * words, body_words * 4);
  std::vector<uint8_t> out;
  if (mode == 1) {
    const long n = head[0];
    const int k = head[1];
    if (check_plane(n) != DVD_OK) return refuse(DVD_E_MAP_SHAPE);
    if (k < 1 || k > kMaxRanks || body_words < (size_t)k) return refuse(DVD_E_MAP_RANKS);
    if (check_ranks(body.data(), k, n) != DVD_OK) return refuse(DVD_E_MAP_RANKS);
    if (body_words != (size_t)k + (size_t)n) return 2;
    uint32_t sel[kMaxRanks];
    select_u32(body.data() + k, n, body.data(), k, sel);
    append(out, sel, 4 * (size_t)k);
  } else {
    const int g = head[0], gt_g = head[1], n_hyp = head[2], h = head[3], w = head[4];
    if (check_errors(g, gt_g, n_hyp, h, w) != DVD_OK) return refuse(DVD_E_MAP_SHAPE);
    const size_t n = (size_t)h * w, gg = g ? (size_t)2 * g * g : 2 * n, gt_words = gt_g ? (size_t)2 * gt_g * gt_g : 2 * n;
    if (body_words != gg + gt_words + (n_hyp >= 2 ? (size_t)n_hyp * gg : 0)) return 2;
    std::vector<float> fl(body_words);
    memcpy(fl.data(), body.data(), body_words * 4);
    const float* flow = fl.data();
    const float* gt = flow + gg;
    const float* hyps = gt + gt_words;
    const Up up = dvd::fv::make_up(g ? g : 2, h, w), up_gt = dvd::fv::make_up(gt_g ? gt_g : 2, h, w);
    std::vector<uint32_t> e(n), sigma(n);
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    double se = 0.0, se2 = 0.0;
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j) {
        const size_t p = (size_t)i * w + j;
        float pu, pv, gu, gv, ev = 0.f, m = 0.f, s = 0.f;
        if (g) {
          full_uv_at(flow, up, i, j, &pu, &pv);
        } else {
          pu = flow[2 * p];
          pv = flow[2 * p + 1];
        }
        if (gt_g) {
          full_uv_at(gt, up_gt, i, j, &gu, &gv);
        } else {
          gu = gt[2 * p];
          gv = gt[2 * p + 1];
        }
        bool sigma_ok = true;
        if (n_hyp >= 2) s = spread_at(hyps, n_hyp, up, i, j, &sigma_ok);
        const bool valid = pixel_error(pu, pv, gu, gv, sigma_ok, &ev, &m);
        e[p] = valid ? bits_of(ev) : kInvalid;
        sigma[p] = valid ? bits_of(s) : kInvalid;
        if (valid) {
          cnt[0] += 1;
          cnt[1] += ev <= 1.f;
          cnt[2] += ev <= 3.f;
          cnt[3] += ev <= 5.f;
          cnt[4] += fl_outlier(ev, m);
          se += (double)ev;
          se2 += (double)ev * (double)ev;
        }
      }
    append(out, e.data(), 4 * n);
    append(out, sigma.data(), 4 * n);
    append(out, cnt, sizeof cnt);
    append(out, &se, 8);
    append(out, &se2, 8);
    if (cnt[0]) {
      sparsify(e, sigma, cnt[0], out);
      sparsify(e, e, cnt[0], out);
    }
  }
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
