// The JPEG encoder's format arithmetic, shared by the kernels of jpeg.hip and by the stand-alone CPU restatement
// jpeg_host_check.cpp (plain C++, no HIP): geometry, the quality rule, colour conversion, the 8 x 8 forward DCT, quantisation,
// the Huffman coder of one block, the bit emitter, byte stuffing, the header and the size bounds.  DESIGN.md section 4.5 holds
// the format.  Everything is integer arithmetic and a pure function of its arguments; how the threads of a workgroup share a
// bitstream is the caller's `Ops`:
//   Ops::store32(ptr, v)   a word that one block owns entirely
//   Ops::or32(ptr, v)      a word that two blocks may share (an LDS atomic on the device, a plain |= on the host)
#pragma once
#include <stdint.h>

#include "../../include/dvd_hip.h"

#include "hd.h"

namespace dvd {
namespace jpeg {

// ---------------------------------------------------------------- tables (ITU-T T.81 Annex K) -------------------------------
// position in the zig-zag sequence -> natural index 8 v + u (T.81 figure 5)
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// K.1: luminance, chrominance, natural order
constexpr uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// K.3: BITS (codes of length 1..16) and HUFFVAL of the four tables; table 0 = luminance, 1 = chrominance
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// symbol -> (length << 16) | code, built by the procedure of T.81 Annex C; 0 for a symbol the table does not hold
struct HuffEnc {
  uint32_t dc[12];
  uint32_t ac[256];
};
constexpr HuffEnc make_enc(int t) {
  HuffEnc e{};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < kDcBits[t][len - 1]; ++i) e.dc[kDcVals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
  code = 0;
  k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < kAcBits[t][len - 1]; ++i) e.ac[kAcVals[t][k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
  return e;
}
constexpr int max_len(const HuffEnc& e, bool dc) {
  int m = 0;
  for (int i = 0; i < (dc ? 12 : 256); ++i) {
    const int l = (int)((dc ? e.dc[i] : e.ac[i]) >> 16);
    m = l > m ? l : m;
  }
  return m;
}
constexpr HuffEnc kEncLum = make_enc(0), kEncChr = make_enc(1);
constexpr int kMaxDcLen = max_len(kEncLum, true) > max_len(kEncChr, true) ? max_len(kEncLum, true) : max_len(kEncChr, true);
constexpr int kMaxAcLen = max_len(kEncLum, false) > max_len(kEncChr, false) ? max_len(kEncLum, false) : max_len(kEncChr, false);
static_assert(kMaxDcLen == 11 && kMaxAcLen == 16, "Annex K.3: the longest DC code has 11 bits, the longest AC code 16");

// ---------------------------------------------------------------- sizes -----------------------------------------------------
// Most bits one block can take: a DC code and 63 AC codes at their longest, each followed by 11 magnitude bits (the DC
// difference has at most 11; an AC coefficient of 8-bit samples at most 10).  ZRL and EOB only replace coefficients.
constexpr int kMagBits = 11;
constexpr int kBlockBitsMax = (kMaxDcLen + kMagBits) + 63 * (kMaxAcLen + kMagBits);   // 1723
// SOI 2, APP0 18, DQT 134, SOF0 19, DHT 420, DRI 6, SOS 14
constexpr int kHeaderBytes = 2 + 18 + (4 + 2 * 65) + 19 + (4 + 2 * (17 + 12) + 2 * (17 + 162)) + 6 + 14;
static_assert(kHeaderBytes == 613, "");
constexpr int kTile = 256;                   // blocks whose bits a workgroup joins in LDS at a time, one per thread
// words of a tile's bitstream: up to 31 bits carried over from the tile before, kTile blocks, one word of slack for the
// emitter's last partial word
constexpr int kTileWords = (31 + kTile * kBlockBitsMax + 31) / 32 + 1;

struct Geom {
  int ss;            // DVD_JPEG_420 or DVD_JPEG_444
  int mw, mh;        // pixels per MCU
  int mcus_x, mcus_y;
  int bpm;           // blocks per MCU: 6 (Y Y Y Y Cb Cr) or 3 (Y Cb Cr)
  long row_blocks;   // blocks of one restart interval = one MCU row
};
DVD_HD Geom geom_of(int h, int w, int ss) {
  Geom g;
  g.ss = ss;
  g.mw = g.mh = ss == DVD_JPEG_420 ? 16 : 8;
  g.mcus_x = (w + g.mw - 1) / g.mw;
  g.mcus_y = (h + g.mh - 1) / g.mh;
  g.bpm = ss == DVD_JPEG_420 ? 6 : 3;
  g.row_blocks = (long)g.mcus_x * g.bpm;
  return g;
}
// h and w fit SOF0's 16 bits, and the padded planes stay below 2^31 bytes (no product here leaves 64 bits)
DVD_HD bool shape_ok(int h, int w) {
  if (h < 1 || w < 1 || h > 65535 || w > 65535) return false;
  return 3L * ((h + 15) / 16 * 16) * ((w + 15) / 16 * 16) < (1L << 31);
}
// most bytes of one interval before stuffing, a multiple of 4; after stuffing and padding at most twice that
DVD_HD long interval_raw_max(long row_blocks) { return (row_blocks * kBlockBitsMax + 31) / 32 * 4; }
DVD_HD long interval_slot(long row_blocks) { return (2 * interval_raw_max(row_blocks) + 15) / 16 * 16; }
// header, per interval its stuffed bytes and a marker (RSTn, or EOI after the last)
DVD_HD long file_bound(const Geom& g) { return kHeaderBytes + (long)g.mcus_y * (2 * interval_raw_max(g.row_blocks) + 2); }

// ---------------------------------------------------------------- quality -> tables -----------------------------------------
// natural order; t = 0 luminance, 1 chrominance
struct QuantTables { uint16_t q[2][64]; };
inline QuantTables quant_tables(int quality) {
  QuantTables t;
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) {
      const int v = (kBaseQuant[c][i] * s + 50) / 100;
      t.q[c][i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
  return t;
}

// ---------------------------------------------------------------- colour ----------------------------------------------------
// JFIF's RGB -> YCbCr in 16-bit fixed point, rounded half up (the weights of each row sum to 65536 or to 0); all in 0..255
DVD_HD int rgb_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
DVD_HD int rgb_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
DVD_HD int rgb_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }
// 4:2:0: the 2 x 2 box average, rounded half up
DVD_HD int box4(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }

// ---------------------------------------------------------------- forward DCT -----------------------------------------------
// The 8-point DCT-II of T.81 A.3.3, out[u] = C(u)/2 sum_x in[x] cos((2x+1) u pi / 16), as the integer matrix
// M[u][x] = round(2^13 C(u)/2 cos(...)): seven distinct magnitudes.  x and 7 - x share a magnitude (equal signs for even u,
// opposite for odd u), so the sums s and differences d halve the products; integer arithmetic makes that exact.
constexpr int kC4 = 2896, kC1 = 4017, kC3 = 3406, kC5 = 2276, kC7 = 799, kC2 = 3784, kC6 = 1567;
DVD_HD void dct8(const int in[8], int out[8]) {
  const int s0 = in[0] + in[7], s1 = in[1] + in[6], s2 = in[2] + in[5], s3 = in[3] + in[4];
  const int d0 = in[0] - in[7], d1 = in[1] - in[6], d2 = in[2] - in[5], d3 = in[3] - in[4];
  out[0] = kC4 * (s0 + s1 + s2 + s3);
  out[4] = kC4 * (s0 - s1 - s2 + s3);
  out[2] = kC2 * (s0 - s3) + kC6 * (s1 - s2);
  out[6] = kC6 * (s0 - s3) - kC2 * (s1 - s2);
  out[1] = kC1 * d0 + kC3 * d1 + kC5 * d2 + kC7 * d3;
  out[3] = kC3 * d0 - kC7 * d1 - kC1 * d2 - kC5 * d3;
  out[5] = kC5 * d0 - kC1 * d1 + kC7 * d2 + kC3 * d3;
  out[7] = kC7 * d0 - kC5 * d1 + kC3 * d2 - kC1 * d3;
}
// Rows first: level-shifted samples (-128..127) -> the row's DCT with 2 fraction bits (|.| <= 1449).  Then columns: those
// -> the coefficient with 3 fraction bits, rounded half up (|.| <= 8 * 1024 + rounding), so that quantisation is the only
// rounding that costs precision.  >> of a negative int is the arithmetic shift (floor).
constexpr int kCoefFractionBits = 3;
DVD_HD void dct8_rows(const int in[8], int out[8]) {
  dct8(in, out);
  for (int u = 0; u < 8; ++u) out[u] = (out[u] + (1 << 10)) >> 11;
}
DVD_HD void dct8_cols(const int in[8], int out[8]) {
  dct8(in, out);
  for (int v = 0; v < 8; ++v) out[v] = (out[v] + (1 << 11)) >> 12;
}
// c = the coefficient with kCoefFractionBits fraction bits, q = the table's entry: c / (8 q), rounded half away from zero
DVD_HD int quantize(int c, int q) {
  const int d = q << kCoefFractionBits, a = c < 0 ? -c : c, r = (a + (d >> 1)) / d;
  return c < 0 ? -r : r;
}

// ---------------------------------------------------------------- Huffman coding of one block -------------------------------
DVD_HD int bit_size(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }   // a >= 0: bits of a
// (magnitude bits, their count) of v (T.81 F.1.2.1): v itself if positive, v - 1 in `size` bits if negative
DVD_HD uint32_t mag_bits(int v, int size) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u); }

// The block in MCU order before `b` that holds the same component, as a distance; 0 for the first of the interval
// (its predictor is 0).  4:2:0 MCU: Y00 Y01 Y10 Y11 Cb Cr.
DVD_HD int pred_distance(long b, int bpm) {
  const int k = (int)(b % bpm);
  if (bpm == 3) return b >= 3 ? 3 : 0;
  if (k >= 1 && k <= 3) return 1;
  if (k == 0) return b >= 6 ? 3 : 0;
  return b >= 6 ? 6 : 0;
}
DVD_HD bool is_chroma(long b, int bpm) { return (int)(b % bpm) >= bpm - 2; }

// zz: the block's 64 quantised coefficients in zig-zag order; pred: the DC of the previous block of the component.
// Sink::put(code, nbits) takes nbits <= 27.
template <class Sink>
DVD_HD void encode_block(const int16_t* zz, int pred, const HuffEnc& enc, Sink& sink) {
  const int diff = zz[0] - pred;
  const int ds = bit_size(diff < 0 ? -diff : diff);
  const uint32_t dc = enc.dc[ds];
  sink.put(((dc & 0xFFFFu) << ds) | mag_bits(diff, ds), (int)(dc >> 16) + ds);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = zz[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run >= 16) {                                           // ZRL: sixteen zeros
      const uint32_t z = enc.ac[0xF0];
      sink.put(z & 0xFFFFu, (int)(z >> 16));
      run -= 16;
    }
    const int size = bit_size(v < 0 ? -v : v);
    const uint32_t c = enc.ac[(run << 4) | size];
    sink.put(((c & 0xFFFFu) << size) | mag_bits(v, size), (int)(c >> 16) + size);
    run = 0;
  }
  if (run) {                                                      // EOB: the rest is zero
    const uint32_t e = enc.ac[0x00];
    sink.put(e & 0xFFFFu, (int)(e >> 16));
  }
}

struct CountSink {
  int bits;
  DVD_HD void put(uint32_t, int nbits) { bits += nbits; }
};

// Writes a block's bits at a bit offset of a stream of 32-bit words; the stream's first bit is the top bit of word 0 (byte
// j is bits 31-8(j%4) .. 24-8(j%4) of word j/4).  The words must be zero where other blocks have not written.  The first
// word (shared with the block before unless the offset is a multiple of 32) and the last, partial one are OR-ed in.
template <class Ops>
struct EmitSink {
  uint32_t* words;
  long wi;
  uint64_t acc;
  int cnt;           // bits of acc not yet written, < 32 between calls (in the first word: the bits in front count)
  bool shared;
  DVD_HD EmitSink(uint32_t* w, long bit_offset) : words(w), wi(bit_offset >> 5), acc(0), cnt((int)(bit_offset & 31)), shared(true) {}
  DVD_HD void put(uint32_t v, int nbits) {
    acc = (acc << nbits) | v;
    cnt += nbits;
    if (cnt >= 32) {
      cnt -= 32;
      const uint32_t word = (uint32_t)(acc >> cnt);
      if (shared) Ops::or32(words + wi, word);
      else Ops::store32(words + wi, word);
      shared = false;
      ++wi;
      acc &= (1ull << cnt) - 1ull;
    }
  }
  DVD_HD void finish() {
    if (cnt > 0) Ops::or32(words + wi, (uint32_t)(acc << (32 - cnt)));
  }
};

DVD_HD uint8_t stream_byte(const uint32_t* words, long j) { return (uint8_t)(words[j >> 2] >> (24 - 8 * (int)(j & 3))); }

// ---------------------------------------------------------------- header ----------------------------------------------------
// SOI, APP0 (JFIF 1.01, density 1:1, no thumbnail), DQT (both tables, zig-zag order), SOF0, DHT (the four tables), DRI (one
// MCU row), SOS: kHeaderBytes bytes.  Host only: the kernels receive the result.
struct Header { uint8_t b[kHeaderBytes + 3]; };
inline Header make_header(int h, int w, const Geom& g, const QuantTables& qt) {
  Header hd{};
  uint8_t* p = hd.b;
  auto put = [&p](int v) { *p++ = (uint8_t)v; };
  auto put16 = [&put](int v) { put(v >> 8); put(v & 255); };
  put16(0xFFD8);
  put16(0xFFE0); put16(16);
  put('J'); put('F'); put('I'); put('F'); put(0);
  put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
  put16(0xFFDB); put16(2 + 2 * 65);
  for (int t = 0; t < 2; ++t) {
    put(t);                                                       // 8-bit entries, table t
    for (int k = 0; k < 64; ++k) put(qt.q[t][kZigzag[k]]);
  }
  put16(0xFFC0); put16(17); put(8); put16(h); put16(w); put(3);
  const int ys = g.ss == DVD_JPEG_420 ? 0x22 : 0x11;
  put(1); put(ys); put(0);
  put(2); put(0x11); put(1);
  put(3); put(0x11); put(1);
  put16(0xFFC4); put16(2 + 2 * (17 + 12) + 2 * (17 + 162));
  for (int t = 0; t < 2; ++t) {
    put(0x00 | t);
    for (int i = 0; i < 16; ++i) put(kDcBits[t][i]);
    for (int i = 0; i < 12; ++i) put(kDcVals[i]);
    put(0x10 | t);
    for (int i = 0; i < 16; ++i) put(kAcBits[t][i]);
    for (int i = 0; i < 162; ++i) put(kAcVals[t][i]);
  }
  put16(0xFFDD); put16(4); put16(g.mcus_x);
  put16(0xFFDA); put16(12); put(3);
  put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
  put(0); put(63); put(0);
  return hd;
}

}  // namespace jpeg
}  // namespace dvd
