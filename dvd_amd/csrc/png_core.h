// The PNG encoder's format arithmetic, shared by the kernels of png.hip and by the stand-alone CPU restatement
// png_host_check.cpp (plain C++, no HIP): filter residuals, the fixed-Huffman token writer, the segment compressor, CRC-32
// and Adler-32 pieces, and the size bounds.  DESIGN.md section 4.4 holds the format.
// Everything here is a pure function of its arguments; how a wave shares the work is the caller's `Ops`:
//   Ops::uniform(v)                 the value as a wave-uniform one (identity on the host)
//   Ops::match_len(seg, c, p, max)  the number of equal bytes of seg[c..] and seg[p..], at most max
//   Ops::store32(ptr, v)            one 32-bit store to the output slot (one lane only on the device)
//   Ops::store16(ptr, v)            one hash-table store
#pragma once
#include <stdint.h>

#include "../../include/dvd_hip.h"

#if defined(__HIPCC__)
#define DVD_HD __host__ __device__ __forceinline__
#else
#define DVD_HD inline
#endif

namespace dvd {
namespace png {

constexpr int kSeg = DVD_PNG_SEGMENT;        // bytes of the filtered stream per segment = per IDAT chunk
static_assert(kSeg >= 64 && kSeg <= 32768 && kSeg % 16 == 0, "a position must fit 15 bits (distance <= 32768, 0xFFFF = empty)");
constexpr int kHashBits = 12;                // 4096 most recent positions, one candidate per 3-byte hash
constexpr int kHashSize = 1 << kHashBits;
constexpr unsigned kEmpty = 0xFFFFu;
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr int kInsertMax = 8;                // positions inside a match enter the hash table only for matches this short
constexpr uint32_t kAdlerMod = 65521u;
constexpr uint32_t kCrcPoly = 0xEDB88320u;   // reflected CRC-32 polynomial

// Most bytes the deflate data of a segment of n stream bytes can take.  Every token costs at most 9 bits per byte it covers:
// a literal 8 or 9 bits; a match of 3 at most 7 + 5 + 13 = 25 <= 27 bits, a longer one at most 8 + 5 + 5 + 13 = 31 <= 36.
// So the fixed block is at most 3 (header) + 9 n + 7 (end of block) bits; the empty stored block adds its 3 header bits, the
// padding to a byte and 00 00 FF FF: ceil((13 + 9 n) / 8) + 4 <= ceil((10 + 9 n) / 8) + 5 bytes.
DVD_HD long seg_data_max(long n) { return (10 + 9 * n + 7) / 8 + 5; }
// A segment's slot in the scratch buffer: the above for a full segment, the zlib header (2, first segment), the final empty
// fixed block (2, last segment), up to 3 bytes that the last 32-bit flush writes past the length; a multiple of 16.
constexpr long kSlot = ((10 + 9L * kSeg + 7) / 8 + 5 + 2 + 2 + 3 + 15) / 16 * 16;

DVD_HD long stream_bytes(int h, int w) { return (long)h * (3L * w + 1); }
DVD_HD long segments(long stream) { return (stream + kSeg - 1) / kSeg; }
// signature 8, IHDR 25, per segment an IDAT frame of 12 around its data, zlib header 2, final block 2, Adler-32 4, IEND 12
DVD_HD long file_bound(long stream) {
  const long ns = segments(stream);
  return 8 + 25 + 12 * ns + (ns - 1) * seg_data_max(kSeg) + seg_data_max(stream - (ns - 1) * kSeg) + 2 + 2 + 4 + 12;
}

// ---------------------------------------------------------------- filters ---------------------------------------------------
DVD_HD int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// x = the byte, a = left (3 bytes back), b = up, c = up-left; absent neighbours are 0
DVD_HD uint8_t filter_byte(int f, int x, int a, int b, int c) {
  const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (uint8_t)(x - pred);
}
DVD_HD unsigned residual_cost(uint8_t r) { return r < 128 ? r : 256u - r; }   // |r as a signed byte|
// lowest filter number among the minima
template <class T>
DVD_HD int pick_filter(const T cost[5]) {
  int best = 0;
  for (int f = 1; f < 5; ++f)
    if (cost[f] < cost[best]) best = f;
  return best;
}

// ---------------------------------------------------------------- CRC-32 ----------------------------------------------------
// raw register arithmetic (no initial / final inversion): the state after `byte` from state `crc`
DVD_HD uint32_t crc_byte(uint32_t crc, uint32_t byte) {
  crc ^= byte;
  for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (kCrcPoly & (0u - (crc & 1u)));
  return crc;
}
DVD_HD uint32_t crc_bytes(uint32_t crc, const uint8_t* p, long n) {
  for (long i = 0; i < n; ++i) crc = crc_byte(crc, p[i]);
  return crc;
}
// a * b mod P in the reflected representation (x^0 = 0x80000000)
DVD_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; ++k) {
    p ^= b & (0u - ((a >> (31 - k)) & 1u));
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 n) mod P: the factor that carries a register state across n bytes (state' = crc_mul(state, f) ^ raw(bytes, 0))
DVD_HD uint32_t crc_xpow8(unsigned long long n) {
  uint32_t p = 0x80000000u, sq = 0x00800000u;   // 1, x^8
  while (n) {
    if (n & 1) p = crc_mul(sq, p);
    sq = crc_mul(sq, sq);
    n >>= 1;
  }
  return p;
}

// ---------------------------------------------------------------- Adler-32 --------------------------------------------------
// A segment's partial is (a, b) = (sum d_k, sum (n - k) d_k) mod 65521, k = 0 .. n-1: what it adds to (A, B) from A = 0.
// Folding a segment of n bytes into the running pair, exactly: B += n A + b, A += a.
DVD_HD void adler_fold(uint32_t& A, uint32_t& B, uint32_t n, uint32_t a, uint32_t b) {
  B = (uint32_t)((B + (unsigned long long)(n % kAdlerMod) * A + b) % kAdlerMod);
  A = (A + a) % kAdlerMod;
}

// ---------------------------------------------------------------- deflate, fixed Huffman -----------------------------------
DVD_HD uint32_t bit_reverse(uint32_t v, int nbits) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
  v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32 - nbits);
}

template <class Ops>
struct BitWriter {
  uint64_t buf;
  int cnt;          // bits held, < 32 between calls
  uint32_t* out;
  int words;
  DVD_HD void put(uint32_t v, int nbits) {   // nbits <= 32, v < 2^nbits
    buf |= (uint64_t)v << cnt;
    cnt += nbits;
    if (cnt >= 32) {
      Ops::store32(out + words, (uint32_t)buf);
      ++words;
      buf >>= 32;
      cnt -= 32;
    }
  }
  DVD_HD void pad_to_byte() { cnt = (cnt + 7) & ~7; if (cnt == 32) put(0, 0); }
  DVD_HD int finish() {                      // bytes written; the last store may carry up to 3 bytes of zero padding
    pad_to_byte();
    const int bytes = words * 4 + cnt / 8;
    if (cnt > 0) Ops::store32(out + words, (uint32_t)buf);
    return bytes;
  }
  DVD_HD void literal(uint32_t v) {
    if (v < 144) put(bit_reverse(0x30 + v, 8), 8);
    else put(bit_reverse(0x190 + (v - 144), 9), 9);
  }
  DVD_HD void match(int len, int dist) {     // 3 <= len <= 258, 1 <= dist <= 32768
    uint32_t code, eb = 0, ev = 0;
    const uint32_t l = (uint32_t)(len - 3);
    if (len == kMaxMatch) code = 285;
    else if (l < 8) code = 257 + l;
    else {
      eb = (uint32_t)(31 - __builtin_clz(l)) - 2;
      code = 261 + 4 * eb + ((l >> eb) & 3);
      ev = l & ((1u << eb) - 1);
    }
    if (code < 280) put(bit_reverse(code - 256, 7), 7);
    else put(bit_reverse(0xC0 + (code - 280), 8), 8);
    if (eb) put(ev, (int)eb);
    const uint32_t d = (uint32_t)(dist - 1);
    uint32_t dcode = d, deb = 0, dev = 0;
    if (d >= 4) {
      deb = (uint32_t)(31 - __builtin_clz(d)) - 1;
      dcode = 2 * deb + 2 + ((d >> deb) & 1);
      dev = d & ((1u << deb) - 1);
    }
    put(bit_reverse(dcode, 5), 5);
    if (deb) put(dev, (int)deb);
  }
};

DVD_HD uint32_t hash3(const uint8_t* p) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

// One segment: greedy LZ77 with one candidate per hash (the most recent position with that hash, inside the segment only),
// one fixed-Huffman block, the empty stored block; `first` puts the zlib header 78 01 in front, `last` the final empty fixed
// block 03 00 behind.  table: kHashSize entries, all kEmpty on entry.  Returns the bytes written to out (<= kSlot - 3).
template <class Ops>
DVD_HD int compress_segment(const uint8_t* seg, int n, uint16_t* table, uint32_t* out, bool first, bool last) {
  BitWriter<Ops> bw{0, 0, out, 0};
  if (first) bw.put(0x0178, 16);
  bw.put(2, 3);                               // BFINAL = 0, BTYPE = 01
  int pos = 0;
  while (pos < n) {
    int len = 0, dist = 0;
    if (pos + kMinMatch <= n) {
      const uint32_t h = Ops::uniform(hash3(seg + pos));
      const unsigned cand = Ops::uniform((unsigned)table[h]);
      Ops::store16(table + h, (uint16_t)pos);
      if (cand != kEmpty) {                   // cand < pos: never before the segment's first byte
        const int room = n - pos;             // a match stops at the segment's last byte
        len = Ops::match_len(seg, (int)cand, pos, room < kMaxMatch ? room : kMaxMatch);
        dist = pos - (int)cand;
      }
    }
    if (len >= kMinMatch) {
      bw.match(len, dist);
      if (len <= kInsertMax)
        for (int k = 1; k < len; ++k)
          if (pos + k + kMinMatch <= n) Ops::store16(table + Ops::uniform(hash3(seg + pos + k)), (uint16_t)(pos + k));
      pos += len;
    } else {
      bw.literal(Ops::uniform((uint32_t)seg[pos]));
      ++pos;
    }
  }
  bw.put(0, 7);                               // end of block (code 256)
  bw.put(0, 3);                               // empty stored block: BFINAL = 0, BTYPE = 00, pad, LEN = 0, NLEN = FFFF
  bw.pad_to_byte();
  bw.put(0x0000, 16);
  bw.put(0xFFFF, 16);
  if (last) bw.put(3, 10);                    // BFINAL = 1, BTYPE = 01, end of block: the bytes 03 00
  return bw.finish();
}

}  // namespace png
}  // namespace dvd
