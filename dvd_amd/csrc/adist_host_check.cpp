// Stand-alone CPU restatement of the aligned-distortion chain of sflow.hip on the shared arithmetic of adist_core.h and
// sflow_core.h (plain C++, no HIP): flow 1, the fit, the resampled page, flow 2 and the weighted mean.
// tests/test_adist_cpu.py builds it with -fsanitize=address,undefined and holds every output to tests/adist_model.py: the
// integers byte for byte, LD and AD bit for bit.
//   adist_host_check in.bin out.bin
// in.bin : int32 h, w, then the ten int32 fields of dvd_sflow_params in their order, then plane A and plane B, h*w bytes each
// out.bin: flow 1 [2,h,w] int16, sums [4] int64, coefficients [4] int32, B' [h,w] u8, flow 2 [2,h,w] int16, then LD (of flow 1),
//          LD of flow 2 and AD as f64
// stdout : "status"; a refused shape or parameter prints its status (DVD_E_ARG) and writes nothing.
// Two stages alone, on planes of any size 1..8192 per side:
//   adist_host_check fit in.bin out.bin      in: int32 h, w, flow [2,h,w] int16            out: sums [4] int64, coefficients [4] int32
//   adist_host_check align in.bin out.bin    in: int32 h, w, coefficients [4] int32, B u8   out: B' [h,w] u8
#include "adist_core.h"
#include "sflow_host_chain.hpp"

using namespace dvd;

static void fit(const std::vector<int16_t>& flow, int h, int w, int64_t* sums, int32_t* coef) {
  const size_t hw = (size_t)h * w;
  for (int k = 0; k < 4; ++k) sums[k] = 0;                  // exact integer sums, in any order
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int fu = flow[(size_t)y * w + x], fv = flow[hw + (size_t)y * w + x];
      sums[0] += fu;
      sums[1] += (int64_t)ad::centred(x, w) * fu;
      sums[2] += fv;
      sums[3] += (int64_t)ad::centred(y, h) * fv;
    }
  ad::fit_coefs(sums, h, w, coef);
}

static Bytes align(const Bytes& b, int h, int w, const int32_t* coef) {
  Bytes bp((size_t)h * w);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) bp[(size_t)y * w + x] = (uint8_t)ad::aligned_at(b.data(), h, w, y, x, coef);
  return bp;
}

// one stage alone
static int stage(const char* which, const char* in, const char* out) {
  const bool is_fit = strcmp(which, "fit") == 0;
  if (!is_fit && strcmp(which, "align") != 0) return 2;
  Bytes file, res;
  int32_t head[6];
  const size_t nhead = (is_fit ? 2 : 6) * sizeof(int32_t);
  if (!read_all(in, file) || file.size() < nhead) return 2;
  memcpy(head, file.data(), nhead);
  const int h = head[0], w = head[1];
  if (h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) {
    printf("%d\n", DVD_E_ARG);
    return 0;
  }
  const size_t hw = (size_t)h * w;
  if (file.size() - nhead < (is_fit ? 4 * hw : hw)) return 2;
  if (is_fit) {
    std::vector<int16_t> flow(2 * hw);
    memcpy(flow.data(), file.data() + nhead, 4 * hw);
    int64_t sums[4];
    int32_t coef[4];
    fit(flow, h, w, sums, coef);
    append(res, sums, sizeof(sums));
    append(res, coef, sizeof(coef));
  } else {
    res = align(Bytes(file.begin() + nhead, file.begin() + nhead + hw), h, w, head + 2);
  }
  if (!write_all(out, res.data(), res.size())) return 2;
  printf("0\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4) return stage(argv[1], argv[2], argv[3]);
  if (argc != 3) {
    fprintf(stderr, "usage: adist_host_check in.bin out.bin\n");
    return 2;
  }
  int h, w;
  dvd_sflow_params pr;
  Bytes a, b;
  const int rc = read_pair(argv[1], h, w, pr, a, b);
  if (rc == DVD_E_ARG) printf("%d\n", DVD_E_ARG);
  if (rc) return rc == DVD_E_ARG ? 0 : rc;
  const size_t hw = (size_t)h * w;

  std::vector<int16_t> flow1, flow2;
  const double ld = chain(a, b, h, w, pr, flow1);

  int64_t sums[4];
  int32_t coef[4];
  fit(flow1, h, w, sums, coef);
  const Bytes bp = align(b, h, w, coef);
  const double ld2 = chain(a, bp, h, w, pr, flow2);

  const size_t blocks = (hw + kSelBlock - 1) / kSelBlock;   // the weighted mean, its f64 sums in the kernels' order
  std::vector<double> term(blocks * kSelBlock, 0.0), len(blocks * kSelBlock, 0.0);
  int64_t gsum = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t p = (size_t)y * w + x;
      const int g = ad::weight_at(a.data(), h, w, y, x);
      len[p] = ad::flow_len(flow2[p], flow2[hw + p]);
      term[p] = ad::weighted_term(g, len[p]);
      gsum += g;
    }
  const double wsum = ordered_sum(term, blocks), lsum = ordered_sum(len, blocks);
  const double adv = ad::ad_value(wsum, lsum, gsum, (int64_t)hw);

  Bytes out;
  append(out, flow1.data(), flow1.size() * sizeof(int16_t));
  append(out, sums, sizeof(sums));
  append(out, coef, sizeof(coef));
  append(out, bp.data(), bp.size());
  append(out, flow2.data(), flow2.size() * sizeof(int16_t));
  append(out, &ld, sizeof(double));
  append(out, &ld2, sizeof(double));
  append(out, &adv, sizeof(double));
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  printf("0\n");
  return 0;
}
