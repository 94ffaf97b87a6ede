// Stand-alone CPU restatement of the JPEG encoder of jpeg.hip on the shared arithmetic of jpeg_core.h: the same strips, sample
// blocks, row and column passes, tiles of kTile blocks joined in a word buffer, carry between tiles, stuffing runs, layout and
// gather, with the threads of a workgroup as plain loops.  Plain C++ (no HIP), so it can be built with
// -fsanitize=address,undefined and run anywhere:
//     g++ -O1 -g -fsanitize=address,undefined jpeg_host_check.cpp -o jpeg_host_check
//     jpeg_host_check H W QUALITY 420|444 in.rgb out.jpg        in.rgb = H*W*3 raw bytes
// It is not part of libdvd_hip.so; tests/test_jpeg_cpu.py builds and runs it and compares its files with the model's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host_check_io.hpp"
#include "jpeg_core.h"

using namespace dvd::jpeg;

struct HostOps {
  static void store32(uint32_t* p, uint32_t v) { *p = v; }
  static void or32(uint32_t* p, uint32_t v) { *p |= v; }
};

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: %s H W QUALITY 420|444 in.rgb out.jpg\n", argv[0]);
    return 2;
  }
  const int h = atoi(argv[1]), w = atoi(argv[2]), quality = atoi(argv[3]);
  const int ss = !strcmp(argv[4], "420") ? DVD_JPEG_420 : !strcmp(argv[4], "444") ? DVD_JPEG_444 : -1;
  if (!shape_ok(h, w) || quality < 1 || quality > 100 || ss < 0) return 2;
  std::vector<uint8_t> img;
  if (!read_all(argv[5], img) || img.size() < (size_t)h * w * 3) return 2;
  img.resize((size_t)h * w * 3);
  const Geom g = geom_of(h, w, ss);
  const QuantTables qt = quant_tables(quality);
  const Header hd = make_header(h, w, g, qt);
  uint8_t izz[64];
  for (int k = 0; k < 64; ++k) izz[kZigzag[k]] = (uint8_t)k;

  // transform: exactly the blocks of the image's MCUs, so that any access past them is the sanitizer's to find
  const int M = g.mw;
  std::vector<int16_t> coef((size_t)g.mcus_y * g.row_blocks * 64);
  for (int my = 0; my < g.mcus_y; ++my)
    for (int mx = 0; mx < g.mcus_x; ++mx) {
      int16_t blk[6][64];
      const int rows = h - my * M < M ? h - my * M : M, cols_left = w - mx * M;   // the strip's clamp, per MCU
      auto pixel = [&](int py, int px) {
        const int y = my * M + (py < rows ? py : rows - 1), x = mx * M + (px < cols_left ? px : cols_left - 1);
        return img.data() + ((size_t)y * w + x) * 3;
      };
      if (ss == DVD_JPEG_420) {
        for (int qy = 0; qy < 8; ++qy)
          for (int qx = 0; qx < 8; ++qx) {
            int cb[4], cr[4];
            for (int d = 0; d < 4; ++d) {
              const int py = 2 * qy + (d >> 1), px = 2 * qx + (d & 1);
              const uint8_t* p = pixel(py, px);
              blk[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = (int16_t)(rgb_y(p[0], p[1], p[2]) - 128);
              cb[d] = rgb_cb(p[0], p[1], p[2]);
              cr[d] = rgb_cr(p[0], p[1], p[2]);
            }
            blk[4][qy * 8 + qx] = (int16_t)(box4(cb[0], cb[1], cb[2], cb[3]) - 128);
            blk[5][qy * 8 + qx] = (int16_t)(box4(cr[0], cr[1], cr[2], cr[3]) - 128);
          }
      } else {
        for (int py = 0; py < 8; ++py)
          for (int px = 0; px < 8; ++px) {
            const uint8_t* p = pixel(py, px);
            blk[0][py * 8 + px] = (int16_t)(rgb_y(p[0], p[1], p[2]) - 128);
            blk[1][py * 8 + px] = (int16_t)(rgb_cb(p[0], p[1], p[2]) - 128);
            blk[2][py * 8 + px] = (int16_t)(rgb_cr(p[0], p[1], p[2]) - 128);
          }
      }
      for (int k = 0; k < g.bpm; ++k) {
        int tmp[8][8], in[8], out[8];
        for (int r = 0; r < 8; ++r) {
          for (int x = 0; x < 8; ++x) in[x] = blk[k][r * 8 + x];
          dct8_rows(in, tmp[r]);
        }
        int16_t* dst = coef.data() + (((size_t)my * g.mcus_x + mx) * g.bpm + k) * 64;
        const uint16_t* qq = qt.q[k >= g.bpm - 2];
        for (int c = 0; c < 8; ++c) {
          for (int y = 0; y < 8; ++y) in[y] = tmp[y][c];
          dct8_cols(in, out);
          for (int v = 0; v < 8; ++v) dst[izz[v * 8 + c]] = (int16_t)quantize(out[v], qq[v * 8 + c]);
        }
      }
    }

  // entropy coding: per interval, tiles of kTile blocks in a word buffer of exactly the words the tile's bits take
  std::vector<std::vector<uint8_t>> slots(g.mcus_y);
  for (int iv = 0; iv < g.mcus_y; ++iv) {
    const int16_t* base = coef.data() + (size_t)iv * g.row_blocks * 64;
    std::vector<uint8_t>& out = slots[iv];
    uint32_t carry = 0, rest = 0;
    for (long t0 = 0; t0 < g.row_blocks; t0 += kTile) {
      const long nb = g.row_blocks - t0 < kTile ? g.row_blocks - t0 : kTile;
      const bool last = t0 + kTile >= g.row_blocks;
      uint32_t bits[kTile], total = 0;
      int pred[kTile];
      for (long t = 0; t < nb; ++t) {
        const long b = t0 + t;
        const int d = pred_distance(b, g.bpm);
        pred[t] = d ? base[(b - d) * 64] : 0;
        CountSink cs{0};
        encode_block(base + b * 64, pred[t], is_chroma(b, g.bpm) ? kEncChr : kEncLum, cs);
        if (cs.bits > kBlockBitsMax) {
          fprintf(stderr, "interval %d block %ld: %d bits above the bound\n", iv, b, cs.bits);
          return 1;
        }
        bits[t] = (uint32_t)cs.bits;
        total += bits[t];
      }
      const uint32_t end = carry + total;
      std::vector<uint32_t> words((end >> 5) + ((end & 31) ? 1 : 0), 0u);
      if (carry) words[0] = rest;
      uint32_t off = carry;
      for (long t = 0; t < nb; ++t) {
        const long b = t0 + t;
        EmitSink<HostOps> es(words.data(), (long)off);
        encode_block(base + b * 64, pred[t], is_chroma(b, g.bpm) ? kEncChr : kEncLum, es);
        es.finish();
        off += bits[t];
      }
      uint32_t nbytes = (end >> 5) * 4;
      if (last) {
        const uint32_t pad = (8 - (end & 7)) & 7;
        if (pad) words[end >> 5] |= ((1u << pad) - 1u) << (32 - (end & 31) - pad);
        nbytes = (end + 7) >> 3;
      }
      if (!last && (end & 31)) rest = words[end >> 5];
      // stuffing: 256 runs; count, scan, write
      const uint32_t per = (nbytes + 255) / 256;
      uint32_t start[257];
      start[0] = 0;
      for (uint32_t t = 0; t < 256; ++t) {
        const uint32_t lo = t * per < nbytes ? t * per : nbytes, hi = lo + per < nbytes ? lo + per : nbytes;
        uint32_t ff = 0;
        for (uint32_t i = lo; i < hi; ++i) ff += stream_byte(words.data(), i) == 0xFF;
        start[t + 1] = start[t] + ff;
      }
      const size_t outpos = out.size();
      out.resize(outpos + nbytes + start[256]);                    // exactly the tile's stuffed bytes
      for (uint32_t t = 0; t < 256; ++t) {
        const uint32_t lo = t * per < nbytes ? t * per : nbytes, hi = lo + per < nbytes ? lo + per : nbytes;
        uint8_t* dst = out.data() + outpos + lo + start[t];
        for (uint32_t i = lo; i < hi; ++i) {
          const uint8_t v = stream_byte(words.data(), i);
          *dst++ = v;
          if (v == 0xFF) *dst++ = 0;
        }
      }
      carry = end & 31;
    }
    if ((long)out.size() > 2 * interval_raw_max(g.row_blocks)) {
      fprintf(stderr, "interval %d: %zu bytes above the bound\n", iv, out.size());
      return 1;
    }
  }

  // layout and gather
  std::vector<unsigned long long> offs(g.mcus_y);
  unsigned long long pos = kHeaderBytes;
  for (int iv = 0; iv < g.mcus_y; ++iv) {
    offs[iv] = pos;
    pos += 2ull + slots[iv].size();
  }
  if ((long)pos > file_bound(g)) {
    fprintf(stderr, "file of %llu bytes above the bound %ld\n", pos, file_bound(g));
    return 1;
  }
  std::vector<uint8_t> file((size_t)pos);
  memcpy(file.data(), hd.b, kHeaderBytes);
  for (int iv = 0; iv < g.mcus_y; ++iv) {
    uint8_t* dst = file.data() + offs[iv];
    const size_t len = slots[iv].size();
    if (len) memcpy(dst, slots[iv].data(), len);
    dst[len] = 0xFF;
    dst[len + 1] = iv == g.mcus_y - 1 ? 0xD9 : (uint8_t)(0xD0 + (iv & 7));
  }
  if (!write_all(argv[6], file.data(), file.size())) return 2;
  printf("%llu\n", pos);
  return 0;
}
