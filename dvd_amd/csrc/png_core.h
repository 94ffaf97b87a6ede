// The PNG encoder's format arithmetic, shared by the kernels of png.hip and by the stand-alone CPU restatement
// png_host_check.cpp (plain C++, no HIP): filter residuals, the fixed-Huffman token writer, the token loop and the segment
// compressor, the dynamic route's code builder, header and pricing, CRC-32 and Adler-32 pieces, and the size bounds.
// DESIGN.md section 4.4 holds the format.
// Everything here is a pure function of its arguments; how a wave shares the work is the caller's `Ops`:
//   Ops::uniform(v)                 the value as a wave-uniform one (identity on the host)
//   Ops::match_len(seg, c, p, max)  the number of equal bytes of seg[c..] and seg[p..], at most max
//   Ops::store32(ptr, v)            one 32-bit store to the output slot (one lane only on the device)
//   Ops::store16(ptr, v)            one hash-table store
//   Ops::store_tok(ptr, v)          one 16-bit token store (one lane only on the device)
//   Ops::lane(), Ops::lanes()       this lane's number and the lanes that share a loop (0 and 1 on the host)
//   Ops::count(ptr)                 ++*ptr on a histogram cell that other lanes count into as well
#pragma once
#include <stdint.h>

#include "../../include/dvd_hip.h"

#include "hd.h"

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

// The length symbol 257..285 of a match of l + 3 bytes and the distance symbol 0..29 of a distance of d + 1, each with the
// number and the value of its extra bits (RFC 1951 section 3.2.5).
DVD_HD uint32_t len_symbol(uint32_t l, uint32_t& eb, uint32_t& ev) {
  eb = 0;
  ev = 0;
  if (l == (uint32_t)(kMaxMatch - 3)) return 285;
  if (l < 8) return 257 + l;
  eb = (uint32_t)(31 - __builtin_clz(l)) - 2;
  ev = l & ((1u << eb) - 1);
  return 261 + 4 * eb + ((l >> eb) & 3);
}
DVD_HD uint32_t dist_symbol(uint32_t d, uint32_t& deb, uint32_t& dev) {
  deb = 0;
  dev = 0;
  if (d < 4) return d;
  deb = (uint32_t)(31 - __builtin_clz(d)) - 1;
  dev = d & ((1u << deb) - 1);
  return 2 * deb + 2 + ((d >> deb) & 1);
}
DVD_HD uint32_t len_extra_bits(uint32_t sym) { return (sym < 265 || sym == 285) ? 0u : (sym - 261) / 4; }
DVD_HD uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0u : sym / 2 - 1; }

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
    uint32_t eb, ev, deb, dev;
    const uint32_t code = len_symbol((uint32_t)(len - 3), eb, ev);
    if (code < 280) put(bit_reverse(code - 256, 7), 7);
    else put(bit_reverse(0xC0 + (code - 280), 8), 8);
    if (eb) put(ev, (int)eb);
    const uint32_t dcode = dist_symbol((uint32_t)(dist - 1), deb, dev);
    put(bit_reverse(dcode, 5), 5);
    if (deb) put(dev, (int)deb);
  }
};

DVD_HD uint32_t hash3(const uint8_t* p) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

// The token loop of one segment: greedy LZ77 with one candidate per hash (the most recent position with that hash, inside the
// segment only).  table: kHashSize entries, all kEmpty on entry.  Every token goes to `sink` (literal(v) / match(len, dist)):
// the fixed route's sink writes its bits at once, the dynamic route's keeps the tokens.
template <class Ops, class Sink>
DVD_HD void tokenise(const uint8_t* seg, int n, uint16_t* table, Sink& sink) {
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
      sink.match(len, dist);
      if (len <= kInsertMax)
        for (int k = 1; k < len; ++k)
          if (pos + k + kMinMatch <= n) Ops::store16(table + Ops::uniform(hash3(seg + pos + k)), (uint16_t)(pos + k));
      pos += len;
    } else {
      sink.literal(Ops::uniform((uint32_t)seg[pos]));
      ++pos;
    }
  }
}

template <class Ops>
struct FixedSink {
  BitWriter<Ops>& bw;
  DVD_HD void literal(uint32_t v) { bw.literal(v); }
  DVD_HD void match(int len, int dist) { bw.match(len, dist); }
};

// What follows a segment's block: the empty stored block (BFINAL = 0, BTYPE = 00, pad, LEN = 0, NLEN = FFFF) and, behind the
// last segment, the final empty fixed block (BFINAL = 1, BTYPE = 01, end of block: the bytes 03 00).  Returns the bytes written.
template <class Ops>
DVD_HD int finish_segment(BitWriter<Ops>& bw, bool last) {
  bw.put(0, 3);
  bw.pad_to_byte();
  bw.put(0x0000, 16);
  bw.put(0xFFFF, 16);
  if (last) bw.put(3, 10);
  return bw.finish();
}

// One segment of the fixed route: the token loop into ONE fixed-Huffman block, then the empty stored block; `first` puts the
// zlib header 78 01 in front, `last` the final empty fixed block 03 00 behind.  Returns the bytes written to out (<= kSlot - 3).
template <class Ops>
DVD_HD int compress_segment(const uint8_t* seg, int n, uint16_t* table, uint32_t* out, bool first, bool last) {
  BitWriter<Ops> bw{0, 0, out, 0};
  if (first) bw.put(0x0178, 16);
  bw.put(2, 3);                               // BFINAL = 0, BTYPE = 01
  FixedSink<Ops> sink{bw};
  tokenise<Ops>(seg, n, table, sink);
  bw.put(0, 7);                               // end of block (code 256)
  return finish_segment(bw, last);
}

// ---------------------------------------------------------------- deflate, dynamic Huffman ---------------------------------
// The dynamic route keeps a segment's tokens as 16-bit entries: a literal is 0..255; a match is its head 256 + (len - 3)
// followed by kDistFlag | (dist - 1).  At most one entry per stream byte (a match covers >= 3 bytes with 2 entries), and a scan
// from any entry tells heads (bit 15 clear) from distance words (bit 15 set).
constexpr int kNumLL = 286, kNumD = 30, kNumCL = 19;
constexpr int kLimitLL = 15, kLimitCL = 7;
constexpr unsigned kDistFlag = 0x8000u;
constexpr int kStageWords = 104;             // 64 tokens of at most 48 bits behind at most 31 pending bits: 97 dwords + spare

template <class Ops>
struct TokenSink {
  uint16_t* tok;
  int count;
  DVD_HD void literal(uint32_t v) {
    Ops::store_tok(tok + count, (uint16_t)v);
    ++count;
  }
  DVD_HD void match(int len, int dist) {
    Ops::store_tok(tok + count, (uint16_t)(256 + (len - 3)));
    Ops::store_tok(tok + count + 1, (uint16_t)(kDistFlag | (unsigned)(dist - 1)));
    count += 2;
  }
};

// Everything the dynamic route keeps per segment between the token loop and the last bit; every array lives here (LDS on the
// device), so no function below needs a private array.
struct DynState {
  uint32_t ll_freq[288], d_freq[32], cl_freq[20];   // histograms: literal/length (one end-of-block included), distance, header
  uint8_t ll_len[288], d_len[32], cl_len[20];       // code lengths, 0 = unused
  uint16_t ll_code[288], d_code[32], cl_code[20];   // canonical codes, bit-reversed for the LSB-first writer
  uint32_t work[2 * 288];                           // build_code_lengths: sort keys, then weights / depths
  uint32_t count[16], next[16];                     // canonical_codes
  uint16_t rle[kNumLL + kNumD + 2];                 // the header's code-length symbols: symbol | extra value << 8
  int nrle, hlit, hdist, hclen;
  uint32_t dyn_bits, fix_bits, dynamic;             // the two block types priced; dynamic = 1 if dyn_bits < fix_bits
  uint32_t stage[kStageWords];                      // the parallel emitter's staging dwords
};

// Code lengths of a length-limited prefix code for freq[0 .. n), a pure function of the histogram:
//   1. the used symbols sorted by (frequency, symbol), ascending - the keys are distinct, so the order is total;
//   2. Huffman depths by the in-place two-queue construction on that order (Moffat and Katajainen), which takes a leaf
//      before an internal node of the same weight;
//   3. if the deepest leaf is beyond `limit`: every depth clamped to the limit; while the Kraft sum is above 1, the rarest
//      symbol among those of the greatest depth below the limit goes one level down; then, while the sum is below 1, pass
//      over the symbols from the most frequent to the rarest and lift by one level each whose gain still fits.  Every pass
//      lifts at least one symbol (the lowest set bit of the deficit is a level some symbol stands on or below), so the code
//      ends complete.
// No used symbol: all lengths 0.  One used symbol: length 1 (an incomplete code; the callers deal with it).
// Needs freq < 2^23, n <= 288, n <= 2^limit, limit <= 15; work: 2 * 288 words.
DVD_HD void build_code_lengths(const uint32_t* freq, int n, int limit, uint8_t* len, uint32_t* work) {
  uint32_t* key = work;
  uint32_t* A = work + 288;
  int m = 0;
  for (int s = 0; s < n; ++s) {
    len[s] = 0;
    if (freq[s]) key[m++] = (freq[s] << 9) | (uint32_t)s;
  }
  if (m == 0) return;
  if (m == 1) {
    len[key[0] & 511u] = 1;
    return;
  }
  for (int gap = 121; gap >= 1; gap /= 3)      // Shell sort, gaps 121 40 13 4 1
    for (int i = gap; i < m; ++i) {
      const uint32_t v = key[i];
      int j = i;
      while (j >= gap && key[j - gap] > v) {
        key[j] = key[j - gap];
        j -= gap;
      }
      key[j] = v;
    }
  for (int i = 0; i < m; ++i) A[i] = key[i] >> 9;
  // first pass, left to right: internal node `next` takes the two least of the remaining leaves and internal nodes
  A[0] += A[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < m - 1; ++next) {
    if (leaf >= m || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] = A[leaf++];
    }
    if (leaf >= m || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] += A[leaf++];
    }
  }
  // second pass, right to left: parent pointers to depths of the internal nodes
  A[m - 2] = 0;
  for (int next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
  // third pass, right to left: depths of the leaves
  int avbl = 1, used = 0, dpth = 0, next = m - 1;
  root = m - 2;
  while (avbl > 0) {
    while (root >= 0 && (int)A[root] == dpth) {
      ++used;
      --root;
    }
    while (avbl > used) {
      A[next--] = (uint32_t)dpth;
      --avbl;
    }
    avbl = 2 * used;
    ++dpth;
    used = 0;
  }
  if ((int)A[0] > limit) {                     // A is non-increasing: the rarest symbol is the deepest
    const uint32_t full = 1u << limit;
    uint32_t kraft = 0;
    for (int i = 0; i < m; ++i) {
      if ((int)A[i] > limit) A[i] = (uint32_t)limit;
      kraft += 1u << (limit - (int)A[i]);
    }
    int i = 0;
    while (kraft > full) {
      while ((int)A[i] >= limit) ++i;          // m <= 2^limit: the sum is at most 1 before i runs out
      kraft -= 1u << (limit - (int)A[i] - 1);
      ++A[i];
    }
    uint32_t deficit = full - kraft;
    while (deficit)
      for (int j = m - 1; j >= 0 && deficit; --j) {
        const uint32_t gain = 1u << (limit - (int)A[j]);
        if (gain <= deficit && A[j] > 1) {
          --A[j];
          deficit -= gain;
        }
      }
  }
  for (int i = 0; i < m; ++i) len[key[i] & 511u] = (uint8_t)A[i];
}

// Canonical codes of RFC 1951 section 3.2.2 for len[0 .. n), bit-reversed.  count / next: 16 words each.
DVD_HD void canonical_codes(const uint8_t* len, int n, uint16_t* code, uint32_t* count, uint32_t* next) {
  for (int b = 0; b < 16; ++b) count[b] = 0;
  for (int s = 0; s < n; ++s) ++count[len[s]];
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) {
    c = (c + count[b - 1]) << 1;
    next[b] = c;
  }
  for (int s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)bit_reverse(next[len[s]]++, len[s]) : (uint16_t)0;
}

// position k of the code-length alphabet's permuted order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (5 bits each)
DVD_HD int cl_order(int k) {
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                      10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (int)((k < 12 ? lo >> (5 * k) : hi >> (5 * (k - 12))) & 31u);
}
DVD_HD uint32_t cl_extra_bits(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }
DVD_HD uint32_t fixed_ll_len(int s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

DVD_HD void rle_put(DynState& st, uint32_t sym, uint32_t extra) {
  st.rle[st.nrle++] = (uint16_t)(sym | extra << 8);
  ++st.cl_freq[sym];
}

// From the histograms to the block that will be written, serial (one lane on the device): the two length-limited codes, the
// header (HLIT / HDIST trimmed of trailing zeros, the concatenated lengths run-length coded greedily - a zero run as 18s of up
// to 138, then one 17 for 3..10, then single zeros; another length once, then 16s of up to 6 copies, then single lengths -,
// its own 7-bit code, HCLEN trimmed in the permuted order), the exact bits of the dynamic and of the fixed block.  If the
// dynamic block is not strictly smaller, the code tables are replaced by the fixed code's, so that one emitter serves both.
DVD_HD void plan_block(DynState& st) {
  build_code_lengths(st.ll_freq, kNumLL, kLimitLL, st.ll_len, st.work);
  build_code_lengths(st.d_freq, kNumD, kLimitLL, st.d_len, st.work);
  int hlit = kNumLL, hdist = kNumD;
  while (hlit > 257 && st.ll_len[hlit - 1] == 0) --hlit;
  while (hdist > 1 && st.d_len[hdist - 1] == 0) --hdist;
  st.hlit = hlit;
  st.hdist = hdist;
  st.nrle = 0;
  for (int s = 0; s < 20; ++s) st.cl_freq[s] = 0;
  const int total = hlit + hdist;              // runs stay inside the concatenated sequence, and may cross its seam
  int i = 0;
  while (i < total) {
    const uint32_t v = i < hlit ? st.ll_len[i] : st.d_len[i - hlit];
    int run = 1;
    while (i + run < total && (i + run < hlit ? st.ll_len[i + run] : st.d_len[i + run - hlit]) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int c = run < 138 ? run : 138;
        rle_put(st, 18, (uint32_t)(c - 11));
        run -= c;
      }
      if (run >= 3) {
        rle_put(st, 17, (uint32_t)(run - 3));
        run = 0;
      }
    } else {
      rle_put(st, v, 0);
      --run;
      while (run >= 3) {
        const int c = run < 6 ? run : 6;
        rle_put(st, 16, (uint32_t)(c - 3));
        run -= c;
      }
    }
    for (; run > 0; --run) rle_put(st, v, 0);
  }
  build_code_lengths(st.cl_freq, kNumCL, kLimitCL, st.cl_len, st.work);
  int used = 0, only = 0;
  for (int s = 0; s < kNumCL; ++s)
    if (st.cl_len[s]) {
      ++used;
      only = s;
    }
  if (used == 1) st.cl_len[only == 0 ? 18 : 0] = 1;   // zlib refuses an incomplete code-length code: a second symbol completes it
  int hclen = kNumCL;
  while (hclen > 4 && st.cl_len[cl_order(hclen - 1)] == 0) --hclen;
  st.hclen = hclen;
  uint32_t dyn = 3 + 14 + 3 * (uint32_t)hclen, fix = 3;
  for (int k = 0; k < st.nrle; ++k) {
    const uint32_t sym = st.rle[k] & 255u;
    dyn += st.cl_len[sym] + cl_extra_bits(sym);
  }
  for (int s = 0; s < kNumLL; ++s) {
    const uint32_t extra = s > 256 ? len_extra_bits((uint32_t)s) : 0u;
    dyn += st.ll_freq[s] * (st.ll_len[s] + extra);
    fix += st.ll_freq[s] * (fixed_ll_len(s) + extra);
  }
  for (int s = 0; s < kNumD; ++s) {
    dyn += st.d_freq[s] * (st.d_len[s] + dist_extra_bits((uint32_t)s));
    fix += st.d_freq[s] * (5 + dist_extra_bits((uint32_t)s));
  }
  st.dyn_bits = dyn;
  st.fix_bits = fix;
  st.dynamic = dyn < fix ? 1u : 0u;
  if (st.dynamic) {
    canonical_codes(st.ll_len, kNumLL, st.ll_code, st.count, st.next);
    canonical_codes(st.d_len, kNumD, st.d_code, st.count, st.next);
    canonical_codes(st.cl_len, kNumCL, st.cl_code, st.count, st.next);
  } else {
    for (int s = 0; s < kNumLL; ++s) {
      st.ll_len[s] = (uint8_t)fixed_ll_len(s);
      const uint32_t c = s < 144 ? 0x30u + s : s < 256 ? 0x190u + (s - 144) : s < 280 ? (uint32_t)(s - 256) : 0xC0u + (s - 280);
      st.ll_code[s] = (uint16_t)bit_reverse(c, st.ll_len[s]);
    }
    for (int s = 0; s < kNumD; ++s) {
      st.d_len[s] = 5;
      st.d_code[s] = (uint16_t)bit_reverse((uint32_t)s, 5);
    }
  }
}

// The histograms of the entries tok[0 .. m): the lanes share the loop and count into the same cells.
template <class Ops>
DVD_HD void count_tokens(const uint16_t* tok, int m, DynState& st) {
  for (int i = Ops::lane(); i < m; i += Ops::lanes()) {
    const uint32_t e = tok[i];
    uint32_t eb, ev;
    if (e & kDistFlag) Ops::count(st.d_freq + dist_symbol(e & 0x7FFFu, eb, ev));
    else Ops::count(st.ll_freq + (e < 256 ? e : len_symbol(e - 256, eb, ev)));
  }
}

// The bits of the token whose head entry is e (next = the entry behind it, read for a match only), LSB first: at most
// 15 + 5 + 15 + 13 = 48.
DVD_HD uint64_t token_bits(const DynState& st, uint32_t e, uint32_t next, int& nbits) {
  if (e < 256) {
    nbits = st.ll_len[e];
    return st.ll_code[e];
  }
  uint32_t eb, ev, deb, dev;
  const uint32_t sym = len_symbol(e - 256, eb, ev);
  uint64_t bits = st.ll_code[sym];
  int nb = st.ll_len[sym];
  bits |= (uint64_t)ev << nb;
  nb += (int)eb;
  const uint32_t dsym = dist_symbol(next & 0x7FFFu, deb, dev);
  bits |= (uint64_t)st.d_code[dsym] << nb;
  nb += st.d_len[dsym];
  bits |= (uint64_t)dev << nb;
  nbits = nb + (int)deb;
  return bits;
}

// What stands in front of a segment's tokens: 78 01 on the first segment, BFINAL = 0 with the block type, and for a dynamic
// block HLIT, HDIST, HCLEN, the code-length code's lengths in the permuted order and the run-length coded lengths.
template <class Ops>
DVD_HD void put_block_header(BitWriter<Ops>& bw, const DynState& st, bool first) {
  if (first) bw.put(0x0178, 16);
  if (!Ops::uniform(st.dynamic)) {
    bw.put(2, 3);                             // BFINAL = 0, BTYPE = 01
    return;
  }
  bw.put(4, 3);                               // BFINAL = 0, BTYPE = 10
  const int hclen = (int)Ops::uniform((uint32_t)st.hclen), nrle = (int)Ops::uniform((uint32_t)st.nrle);
  bw.put(Ops::uniform((uint32_t)st.hlit) - 257, 5);
  bw.put(Ops::uniform((uint32_t)st.hdist) - 1, 5);
  bw.put((uint32_t)hclen - 4, 4);
  for (int k = 0; k < hclen; ++k) bw.put(Ops::uniform(st.cl_len[cl_order(k)]), 3);
  for (int k = 0; k < nrle; ++k) {
    const uint32_t r = Ops::uniform(st.rle[k]), sym = r & 255u;
    bw.put(Ops::uniform(st.cl_code[sym]), (int)Ops::uniform(st.cl_len[sym]));
    if (sym >= 16) bw.put(r >> 8, (int)cl_extra_bits(sym));
  }
}

}  // namespace png
}  // namespace dvd
