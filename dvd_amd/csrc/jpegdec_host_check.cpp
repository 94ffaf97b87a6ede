// Stand-alone CPU restatement of the JPEG decoder of jpegdec.hip on the shared arithmetic of jpegdec_core.h: the same header
// parser, the same walk per subsequence iterated to the fixpoint (every lane of an iteration reads the states of the iteration
// before), count, scan, write, DC sums, IDCT, upsampling, colour and orientation, with the lanes as plain loops and every
// buffer of exactly the size the layout gives it.  Plain C++ (no HIP), so it can be built with -fsanitize=address,undefined:
//     g++ -O1 -g -fsanitize=address,undefined jpegdec_host_check.cpp -o jpegdec_host_check
//     jpegdec_host_check in.jpg out.rgb [max_iters]
// prints "status iterations out_h out_w" and writes out.rgb (out_h * out_w * 3 bytes) when status is 0.  Its exit status is 0
// whenever it could print that line - a refusal, NOSYNC or DATA is a normal outcome - and 2 for a bad command line.
// It is not part of libdvd_hip.so; tests/test_jpegdec_cpu.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host_check_io.hpp"
#include "jpegdec_core.h"

using namespace dvd::jpegdec;

static int finish(int status, int iters, int oh, int ow) {
  printf("%d %d %d %d\n", status, iters, oh, ow);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    fprintf(stderr, "usage: %s in.jpg out.rgb [max_iters]\n", argv[0]);
    return 2;
  }
  const int max_iters = argc == 4 ? atoi(argv[3]) : kDefaultMaxIters;
  std::vector<uint8_t> file;
  if (max_iters < 1 || !read_all(argv[1], file) || file.empty()) return 2;
  const long n = (long)file.size();

  Plan P;
  const char* why = "";
  const int rc = parse(file.data(), n, &P, &why);
  if (rc) {
    fprintf(stderr, "refused: %s\n", why);
    return finish(rc, 0, 0, 0);
  }
  if (P.nsub == 0) return finish(DVD_E_JPEG_DATA, 0, P.out_h, P.out_w);
  // the scan in a buffer of its own, so that a read outside it is the sanitizer's to find
  const std::vector<uint8_t> scan(file.begin() + P.scan_off, file.begin() + P.scan_off + P.scan_len);
  const uint8_t* d = scan.data();
  HuffDec tabs[4];
  memcpy(tabs, P.huff, sizeof tabs);
  auto stop_of = [](long j) { return (j + 1) * (long)kSubseq * 8; };

  // the fixpoint
  std::vector<unsigned long long> E((size_t)P.nsub + 1), En;
  std::vector<uint8_t> chg((size_t)P.nsub + 1, 0), chg_next;
  for (long j = 0; j <= P.nsub; ++j) {
    E[j] = guess_state(j);
    chg[j] = j < P.nsub;
  }
  int it = 0, stamp = 0;
  bool synced = false;
  while (it < max_iters && !synced) {
    En = E;
    chg_next.assign((size_t)P.nsub + 1, 0);
    for (long j = 0; j < P.nsub; ++j) {
      if (!chg[j]) continue;
      NullSink sink;
      const unsigned long long s = walk(tabs, P.dc_mask, P.ac_mask, P.bpm, d, P.scan_len, E[j], stop_of(j), sink);
      if (j + 1 < P.nsub && s != E[j + 1]) {
        En[j + 1] = s;
        chg_next[j + 1] = 1;
        stamp = it + 1;
      }
    }
    E.swap(En);
    chg.swap(chg_next);
    ++it;
    if (stamp < it) {
      synced = true;
      it = stamp + 1;
    }
  }
  if (!synced) return finish(DVD_E_JPEG_NOSYNC, it, P.out_h, P.out_w);

  // count, scan
  std::vector<long> first((size_t)P.nsub);
  long total = 0;
  for (long j = 0; j < P.nsub; ++j) {
    CountSink sink{0};
    walk(tabs, P.dc_mask, P.ac_mask, P.bpm, d, P.scan_len, E[j], stop_of(j), sink);
    first[j] = total;
    total += sink.n;
  }
  if (total != P.nblocks) return finish(DVD_E_JPEG_DATA, it, P.out_h, P.out_w);

  // write
  const Layout l = layout_of(P);
  const long mcus = (long)P.mcus_x * P.mcus_y;
  std::vector<int16_t> coef((size_t)P.nblocks * 64, 0);
  std::vector<uint8_t> flags((size_t)mcus, 0);
  for (long j = 0; j < P.nsub; ++j) {
    WriteSink sink{coef.data(), flags.data(), P.nblocks, first[j], P.bpm};
    walk(tabs, P.dc_mask, P.ac_mask, P.bpm, d, P.scan_len, E[j], stop_of(j), sink);
  }

  // DC differences -> DC values, per component, restarted at flagged MCUs (wrapping sums: garbage cannot overflow)
  uint32_t run[3] = {0, 0, 0};
  for (long m = 0; m < mcus; ++m) {
    if (flags[m]) run[0] = run[1] = run[2] = 0;
    for (int s = 0; s < P.bpm; ++s) {
      int16_t* dc = coef.data() + (m * P.bpm + s) * 64;
      uint32_t& r = run[comp_of_slot(s, P.bpm, P.ncomp)];
      r += (uint32_t)(int32_t)*dc;
      *dc = (int16_t)(uint16_t)r;
    }
  }

  // IDCT into planes of exactly the layout's size
  uint8_t izz[64];
  for (int k = 0; k < 64; ++k) izz[kZigzag[k]] = (uint8_t)k;
  std::vector<uint8_t> plane[3];
  for (int c = 0; c < P.ncomp; ++c) plane[c].assign((size_t)l.pitch[c] * l.rows[c], 0);
  for (long b = 0; b < P.nblocks; ++b) {
    const int slot = (int)(b % P.bpm), comp = comp_of_slot(slot, P.bpm, P.ncomp);
    const long m = b / P.bpm;
    const int mx = (int)(m % P.mcus_x), my = (int)(m / P.mcus_x);
    const int bx = comp == 0 ? mx * P.hs + slot % P.hs : mx, by = comp == 0 ? my * P.vs + slot / P.hs : my;
    int32_t ws[8][8], out[8];
    uint32_t in[8];
    for (int c = 0; c < 8; ++c) {
      for (int r = 0; r < 8; ++r) {
        const int kk = izz[r * 8 + c];
        in[r] = (uint32_t)(int32_t)coef[(size_t)b * 64 + kk] * (uint32_t)P.q[comp][kk];
      }
      idct_1d(in, out, 11);
      for (int r = 0; r < 8; ++r) ws[r][c] = out[r];
    }
    for (int r = 0; r < 8; ++r) {
      for (int x = 0; x < 8; ++x) in[x] = (uint32_t)ws[r][x];
      idct_1d(in, out, 18);
      for (int x = 0; x < 8; ++x) plane[comp].at(((size_t)by * 8 + r) * l.pitch[comp] + (size_t)bx * 8 + x) = (uint8_t)sample_of(out[x]);
    }
  }
  // the kernels may read the cropped planes only: give the final pass exactly those
  const int cw = (P.w + P.hs - 1) / P.hs, ch = (P.h + P.vs - 1) / P.vs;
  std::vector<uint8_t> crop[3];
  for (int c = 0; c < P.ncomp; ++c) {
    const int pw = c == 0 ? P.w : cw, ph = c == 0 ? P.h : ch;
    crop[c].resize((size_t)pw * ph);
    for (int y = 0; y < ph; ++y) memcpy(crop[c].data() + (size_t)y * pw, plane[c].data() + (size_t)y * l.pitch[c], (size_t)pw);
  }
  std::vector<uint8_t> rgb((size_t)P.h * P.w * 3);
  for (int y = 0; y < P.h; ++y)
    for (int x = 0; x < P.w; ++x) {
      int r, g, b;
      r = g = b = crop[0][(size_t)y * P.w + x];
      if (P.ncomp == 3) {
        const int cb = chroma_at(crop[1].data(), cw, P.hs, P.vs, ch, cw, y, x);
        const int cr = chroma_at(crop[2].data(), cw, P.hs, P.vs, ch, cw, y, x);
        ycc_rgb(r, cb, cr, &r, &g, &b);
      }
      int yo, xo;
      oriented(P.orientation, P.h, P.w, y, x, &yo, &xo);
      uint8_t* dst = &rgb.at(((size_t)yo * P.out_w + xo) * 3);
      dst[0] = (uint8_t)r;
      dst[1] = (uint8_t)g;
      dst[2] = (uint8_t)b;
    }
  if (!write_all(argv[2], rgb.data(), rgb.size())) return 2;
  return finish(0, it, P.out_h, P.out_w);
}
