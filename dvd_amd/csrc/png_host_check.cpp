// Stand-alone CPU restatement of the PNG encoder of png.hip on the shared arithmetic of png_core.h: the same filter choice,
// segment compressor, bit writer, Adler-32 folding, chunk layout and CRC-32 tree, with the lanes of a wave and the threads of
// a workgroup as plain loops.  Plain C++ (no HIP), so it can be built with -fsanitize=address,undefined and run anywhere:
//     g++ -O1 -g -fsanitize=address,undefined png_host_check.cpp -o png_host_check
//     png_host_check H W in.rgb out.png            in.rgb = H*W*3 raw bytes; DVD_PNG_HUFFMAN_FIXED
//     png_host_check H W in.rgb out.png dynamic    DVD_PNG_HUFFMAN_DYNAMIC: png_compress_dyn_kernel's steps, its 64 lanes a loop
//     png_host_check --code-lengths LIMIT f0 f1 ...    the lengths build_code_lengths gives the histogram f0 f1 ...
// It is not part of libdvd_hip.so; tests/test_png_cpu.py and tests/test_png_dyn_cpu.py build and run it and decode what it
// writes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host_check_io.hpp"
#include "png_core.h"

using namespace dvd::png;

struct HostOps {
  static uint32_t uniform(uint32_t v) { return v; }
  static int match_len(const uint8_t* seg, int cand, int pos, int maxlen) {
    int len = 0;
    while (len < maxlen && seg[cand + len] == seg[pos + len]) ++len;
    return len;
  }
  static void store32(uint32_t* p, uint32_t v) { *p = v; }
  static void store16(uint16_t* p, uint16_t v) { *p = v; }
  static void store_tok(uint16_t* p, uint16_t v) { *p = v; }
  static int lane() { return 0; }
  static int lanes() { return 1; }
  static void count(uint32_t* p) { ++*p; }
};

// png_compress_dyn_kernel's steps after the segment is staged.  tok: exactly n entries; st on the heap with the staging
// dwords as its last member, so that a staging index past them is the sanitizer's to find.
static int compress_segment_dynamic(const uint8_t* seg, int n, uint16_t* table, uint16_t* tok, DynState& st, uint32_t* out,
                                    bool first, bool last) {
  const int kLanes = 64;
  TokenSink<HostOps> sink{tok, 0};
  tokenise<HostOps>(seg, n, table, sink);
  const int m = sink.count;
  memset(&st, 0, sizeof(st));
  st.ll_freq[256] = 1;
  count_tokens<HostOps>(tok, m, st);
  plan_block(st);
  BitWriter<HostOps> bw{0, 0, out, 0};
  put_block_header(bw, st, first);
  int words = bw.words, cnt = bw.cnt;
  st.stage[0] = (uint32_t)bw.buf;
  for (int i0 = 0; i0 < m; i0 += kLanes) {
    int off = cnt;
    for (int lane = 0; lane < kLanes && i0 + lane < m; ++lane) {
      const uint32_t e = tok[i0 + lane];
      if (e & kDistFlag) continue;
      int nb = 0;
      const uint64_t bits = token_bits(st, e, e >= 256 ? (uint32_t)tok[i0 + lane + 1] : 0u, nb);
      if (nb) {
        const int w = off >> 5, sh = off & 31;
        const uint64_t lo = bits << sh;
        const uint32_t hi = sh ? (uint32_t)(bits >> (64 - sh)) : 0u;
        st.stage[w] |= (uint32_t)lo;
        if ((uint32_t)(lo >> 32)) st.stage[w + 1] |= (uint32_t)(lo >> 32);
        if (hi) st.stage[w + 2] |= hi;
      }
      off += nb;
    }
    const int full = off >> 5;
    const uint32_t carry = st.stage[full];
    for (int k = 0; k < full; ++k) out[words + k] = st.stage[k];
    for (int k = 0; k <= full; ++k) st.stage[k] = k == 0 ? carry : 0u;
    words += full;
    cnt = off & 31;
  }
  bw.words = words;
  bw.cnt = cnt;
  bw.buf = st.stage[0];
  bw.put(st.ll_code[256], st.ll_len[256]);
  return finish_segment(bw, last);
}

static int code_lengths_mode(int argc, char** argv) {
  const int limit = atoi(argv[2]), n = argc - 3;
  if (limit < 1 || limit > 15 || n < 1 || n > 288 || n > (1 << limit)) return 2;
  std::vector<uint32_t> freq((size_t)n), work(2 * 288);
  std::vector<uint8_t> len((size_t)n);
  for (int s = 0; s < n; ++s) {
    const long v = atol(argv[3 + s]);
    if (v < 0 || v >= (1L << 23)) return 2;
    freq[s] = (uint32_t)v;
  }
  build_code_lengths(freq.data(), n, limit, len.data(), work.data());
  for (int s = 0; s < n; ++s) printf(s ? " %d" : "%d", (int)len[s]);
  printf("\n");
  return 0;
}

static void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "--code-lengths")) return code_lengths_mode(argc, argv);
  if (argc != 5 && !(argc == 6 && !strcmp(argv[5], "dynamic"))) {
    fprintf(stderr, "usage: %s H W in.rgb out.png [dynamic] | %s --code-lengths LIMIT f0 f1 ...\n", argv[0], argv[0]);
    return 2;
  }
  const bool dynamic = argc == 6;
  const int h = atoi(argv[1]), w = atoi(argv[2]);
  if (h < 1 || w < 1 || 3L * w + 1 > ((1L << 31) - 1) / h) return 2;
  const long rb = 3L * w, stream = stream_bytes(h, w);
  std::vector<uint8_t> img;
  if (!read_all(argv[3], img) || img.size() < (size_t)h * rb) return 2;
  img.resize((size_t)h * rb);

  // filter: exactly the stream's bytes, so that any access past it is the sanitizer's to find
  std::vector<uint8_t> filt((size_t)stream);
  for (long y = 0; y < h; ++y) {
    const uint8_t* cur = img.data() + y * rb;
    const uint8_t* up = y ? cur - rb : cur;
    unsigned long long cost[5] = {0, 0, 0, 0, 0};
    for (int pass = 0, best = 0; pass < 2; ++pass) {
      for (long i = 0; i < rb; ++i) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y ? up[i] : 0, c = (y && i >= 3) ? up[i - 3] : 0;
        if (pass == 0)
          for (int k = 0; k < 5; ++k) cost[k] += residual_cost(filter_byte(k, x, a, b, c));
        else
          filt[y * (rb + 1) + 1 + i] = filter_byte(best, x, a, b, c);
      }
      if (pass == 0) filt[y * (rb + 1)] = (uint8_t)(best = pick_filter(cost));
    }
  }

  // segments: slot, length, Adler partials
  const int nseg = (int)segments(stream);
  std::vector<std::vector<uint32_t>> slots(nseg);
  std::vector<uint32_t> len(nseg), pa(nseg), pb(nseg);
  for (int s = 0; s < nseg; ++s) {
    const long base = (long)s * kSeg;
    const int n = (int)(stream - base < kSeg ? stream - base : kSeg);
    std::vector<uint8_t> seg(filt.begin() + base, filt.begin() + base + n);   // exactly n bytes
    std::vector<uint16_t> table(kHashSize, (uint16_t)kEmpty);
    // exactly the words a segment of n bytes may take (the device slot is sized for a full segment)
    slots[s].assign((size_t)(seg_data_max(n) + 2 + 2 + 3) / 4, 0xDEADBEEFu);
    if (dynamic) {
      std::vector<uint16_t> tok((size_t)n);                                   // at most one entry per stream byte
      std::vector<DynState> st(1);
      len[s] = (uint32_t)compress_segment_dynamic(seg.data(), n, table.data(), tok.data(), st[0], slots[s].data(), s == 0,
                                                  s == nseg - 1);
    } else {
      len[s] = (uint32_t)compress_segment<HostOps>(seg.data(), n, table.data(), slots[s].data(), s == 0, s == nseg - 1);
    }
    if ((long)len[s] > seg_data_max(n) + (s == 0 ? 2 : 0) + (s == nseg - 1 ? 2 : 0)) {
      fprintf(stderr, "segment %d: %u bytes above the bound\n", s, len[s]);
      return 1;
    }
    unsigned long long a = 0, b = 0;
    for (int k = 0; k < n; ++k) {
      a += seg[k];
      b += (unsigned long long)(n - k) * seg[k];
    }
    pa[s] = (uint32_t)(a % kAdlerMod);
    pb[s] = (uint32_t)(b % kAdlerMod);
  }

  // layout
  std::vector<unsigned long long> offs(nseg);
  unsigned long long pos = 33;
  for (int s = 0; s < nseg; ++s) {
    offs[s] = pos;
    pos += 12ull + len[s] + (s == nseg - 1 ? 4u : 0u);
  }
  const unsigned long long total = pos + 12;
  if ((long)total > file_bound(stream)) {
    fprintf(stderr, "file of %llu bytes above the bound %ld\n", total, file_bound(stream));
    return 1;
  }
  std::vector<uint8_t> out((size_t)total);
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  memcpy(out.data(), sig, 8);
  uint8_t* ih = out.data() + 8;
  put_be32(ih, 13);
  memcpy(ih + 4, "IHDR", 4);
  put_be32(ih + 8, (uint32_t)w);
  put_be32(ih + 12, (uint32_t)h);
  ih[16] = 8; ih[17] = 2; ih[18] = 0; ih[19] = 0; ih[20] = 0;
  put_be32(ih + 21, ~crc_bytes(0xFFFFFFFFu, ih + 4, 17));
  uint32_t A = 1, B = 0;
  for (int s = 0; s < nseg; ++s) {
    const long left = stream - (long)s * kSeg;
    adler_fold(A, B, (uint32_t)(left < kSeg ? left : kSeg), pa[s], pb[s]);
  }
  const uint32_t adler = (B << 16) | A;
  const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
  memcpy(out.data() + pos, iend, 12);

  // gather: the 256 threads of a workgroup as a loop
  for (int s = 0; s < nseg; ++s) {
    const uint8_t* src = (const uint8_t*)slots[s].data();
    const int extra = s == nseg - 1 ? 4 : 0, N = (int)len[s] + extra;
    uint8_t tail[4];
    put_be32(tail, adler);
    uint8_t* dst = out.data() + offs[s];
    for (int i = 0; i < N; ++i) dst[8 + i] = i < (int)len[s] ? src[i] : tail[i - len[s]];
    const int c = (N + 255) / 256, shift = 256 * c - N;
    uint32_t part[256];
    for (int t = 0; t < 256; ++t) {
      uint32_t r = 0;
      for (int j = 0; j < c; ++j) {
        const int i = t * c + j - shift;
        if (i >= 0) r = crc_byte(r, i < (int)len[s] ? src[i] : tail[i - len[s]]);
      }
      part[t] = r;
    }
    uint32_t fac = crc_xpow8((unsigned long long)c);
    for (int d = 1; d < 256; d <<= 1) {
      for (int t = 0; t < 256; t += 2 * d) part[t] = crc_mul(part[t], fac) ^ part[t + d];
      fac = crc_mul(fac, fac);
    }
    put_be32(dst, (uint32_t)N);
    memcpy(dst + 4, "IDAT", 4);
    const uint32_t head = crc_bytes(0xFFFFFFFFu, dst + 4, 4);
    put_be32(dst + 8 + N, ~(crc_mul(head, crc_xpow8((unsigned long long)N)) ^ part[0]));
  }

  if (!write_all(argv[4], out.data(), out.size())) return 2;
  printf("%llu\n", total);
  return 0;
}
