// The JPEG decoder's arithmetic, shared by the kernels of jpegdec.hip and by the stand-alone CPU restatement
// jpegdec_host_check.cpp (plain C++, no HIP): the header parser (host only), the Huffman decode tables, the byte reader that
// steps over stuffing and meets restart markers, the self-synchronising walk over one subsequence of the scan, libjpeg's
// accurate integer IDCT, its triangle chroma upsampling, its colour conversion and the EXIF orientation.  DESIGN.md section
// 4.6 holds the definition.  Everything is integer arithmetic and a pure function of its arguments; no read leaves
// [scan, scan + scan_len) and every loop is bounded by a constant or by the bits of the subsequence.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hd.h"
#include "jpeg_core.h"   // kZigzag
#include "workspace.h"

namespace dvd {
namespace jpegdec {

using jpeg::kZigzag;

constexpr int kSubseq = DVD_JPEGDEC_SUBSEQ;   // bytes of the scan, stuffing included, per lane
constexpr int kDefaultMaxIters = 1024;
constexpr int kGroup = 16;                    // fixpoint iterations launched between two read-backs
constexpr int kDcChunk = 64;                  // MCUs per lane of the DC prefix sum

// Canonical Huffman decoding (T.81 F.2.2.3): a code of length l is valid if it is <= maxcode[l] (-1: no code of that length);
// its symbol is vals[valoff[l] + code].  Index 0 is unused.
struct HuffDec {
  int32_t maxcode[17];
  int32_t valoff[17];
  uint8_t vals[256];
};
constexpr int kHuffWords = (int)(sizeof(HuffDec) / 4);
static_assert(sizeof(HuffDec) == 4 * kHuffWords, "");

// What the kernels need of the header; passed by value.  huff: DC table 0, DC 1, AC 0, AC 1 as words (copied to LDS).
struct Plan {
  int h, w, out_h, out_w;
  int ncomp, hs, vs;         // luma sampling; chroma is 1 x 1
  int mcus_x, mcus_y, bpm;   // blocks per MCU: hs vs + 2, or 1
  int ri, orientation;
  unsigned dc_mask, ac_mask; // bit s: block slot s of the MCU uses DC / AC table 1
  long scan_off, scan_len, nblocks, nsub;
  uint8_t q[3][64];          // per component, zig-zag order as in DQT
  uint32_t huff[4 * kHuffWords];
};

// ---------------------------------------------------------------- header (host only) ----------------------------------------
inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// BITS / HUFFVAL -> decode table; false for a table libjpeg refuses too (a code that does not fit its length; this also
// means that no code is all ones, so the 1-bits that pad a restart interval never decode to a symbol)
inline bool build_huff(const uint8_t bits[16], const uint8_t* vals, int nvals, HuffDec* t) {
  memset(t, 0, sizeof *t);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = bits[l - 1];
    t->maxcode[l] = -1;
    if (cnt) {
      t->valoff[l] = k - code;
      code += cnt;
      k += cnt;
      t->maxcode[l] = code - 1;
    }
    if (code >= (1 << l)) return false;
    code <<= 1;
  }
  if (k != nvals || k > 256) return false;
  memcpy(t->vals, vals, (size_t)k);
  return true;
}

// Orientation tag 0x0112 of IFD0 of an APP1 payload `s` ("Exif\0\0" + TIFF): 0 = no such tag, else its value.
inline int exif_orientation(const uint8_t* s, long sl) {
  if (sl < 14 || memcmp(s, "Exif\0\0", 6) != 0) return 0;
  const uint8_t* t = s + 6;
  const long tl = sl - 6;
  const bool le = t[0] == 'I' && t[1] == 'I';
  if (!le && !(t[0] == 'M' && t[1] == 'M')) return 0;
  auto r16 = [&](long o) -> long { return le ? (t[o] | (t[o + 1] << 8)) : ((t[o] << 8) | t[o + 1]); };
  auto r32 = [&](long o) -> long {
    return le ? ((long)t[o] | ((long)t[o + 1] << 8) | ((long)t[o + 2] << 16) | ((long)t[o + 3] << 24))
              : (((long)t[o] << 24) | ((long)t[o + 1] << 16) | ((long)t[o + 2] << 8) | (long)t[o + 3]);
  };
  if (r16(2) != 42) return 0;
  const long off = r32(4);
  if (off < 8 || off + 2 > tl) return 0;
  const long cnt = r16(off);
  for (long e = 0; e < cnt; ++e) {
    const long p = off + 2 + 12 * e;
    if (p + 12 > tl) break;
    if (r16(p) != 0x0112) continue;
    const long type = r16(p + 2);
    const long v = type == 3 ? r16(p + 8) : type == 4 ? r32(p + 8) : type == 1 ? t[p + 8] : -1;
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 0;
}

inline bool contains(const uint8_t* s, long sl, const char* needle) {
  const long nl = (long)strlen(needle);
  for (long i = 0; i + nl <= sl; ++i)
    if (memcmp(s + i, needle, (size_t)nl) == 0) return true;
  return false;
}

// The file's header -> *P; 0, or the refusal code with *why naming the reason.
inline int parse(const uint8_t* f, long n, Plan* P, const char** why) {
  memset(P, 0, sizeof *P);
#define DVD_JPEGDEC_REFUSE(code, text) \
  do {                                 \
    *why = text;                       \
    return code;                       \
  } while (0)
  if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "no SOI marker");
  uint8_t qt[4][64];
  bool qt_ok[4] = {false, false, false, false};
  HuffDec hd[2][2];
  bool hd_ok[2][2] = {{false, false}, {false, false}};
  int cid[3] = {0, 0, 0}, chs[3] = {0, 0, 0}, cvs[3] = {0, 0, 0}, ctq[3] = {0, 0, 0}, ctd[3] = {0, 0, 0}, cta[3] = {0, 0, 0};
  bool have_sof = false, jfif = false, adobe = false, xmp_orientation = false;
  int adobe_transform = -1, orientation = 0, ri = 0;
  long i = 2, scan_off = -1;
  while (scan_off < 0) {
    if (i + 2 > n) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "truncated header");
    if (f[i] != 0xFF) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "a marker was expected");
    while (i < n && f[i] == 0xFF) ++i;                     // fill bytes
    if (i >= n) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "truncated header");
    const int m = f[i++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // markers without a segment
    if (m == 0xD9) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "EOI before SOS");
    if (i + 2 > n) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "truncated header");
    const long len = rd16(f + i);
    if (len < 2 || i + len > n) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "truncated header");
    const uint8_t* s = f + i + 2;
    const long sl = len - 2;
    if (m == 0xC0) {
      if (have_sof || sl < 6) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad SOF0");
      if (s[0] != 8) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_PRECISION, "samples of other than 8 bits");
      P->h = rd16(s + 1);
      P->w = rd16(s + 3);
      P->ncomp = s[5];
      if (P->ncomp != 1 && P->ncomp != 3) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_COMPONENTS, "neither 1 nor 3 components");
      if (sl != 6 + 3 * P->ncomp || P->h < 1 || P->w < 1) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad SOF0");
      for (int c = 0; c < P->ncomp; ++c) {
        cid[c] = s[6 + 3 * c];
        chs[c] = s[7 + 3 * c] >> 4;
        cvs[c] = s[7 + 3 * c] & 15;
        ctq[c] = s[8 + 3 * c];
      }
      have_sof = true;
    } else if (m == 0xC1) {
      DVD_JPEGDEC_REFUSE(DVD_E_JPEG_EXTENDED, "extended sequential DCT (SOF1)");
    } else if (m == 0xC2) {
      DVD_JPEGDEC_REFUSE(DVD_E_JPEG_PROGRESSIVE, "progressive DCT (SOF2)");
    } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7)) {
      DVD_JPEGDEC_REFUSE(DVD_E_JPEG_LOSSLESS, "lossless or hierarchical coding");
    } else if (m == 0xC8) {
      DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "reserved marker JPG");
    } else if ((m >= 0xC9 && m <= 0xCF)) {
      DVD_JPEGDEC_REFUSE(DVD_E_JPEG_ARITHMETIC, "arithmetic coding");
    } else if (m == 0xC4) {                                // DHT: any number of tables per segment, redefinition allowed
      long p = 0;
      while (p < sl) {
        if (p + 17 > sl) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad DHT");
        const int tc = s[p] >> 4, th = s[p] & 15;
        int cnt = 0;
        for (int l = 0; l < 16; ++l) cnt += s[p + 1 + l];
        if (tc > 1 || th > 3 || cnt > 256 || p + 17 + cnt > sl) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad DHT");
        if (th <= 1) {                                     // baseline: tables 0 and 1; others can only be named by a scan we refuse
          if (!build_huff(s + p + 1, s + p + 17, cnt, &hd[tc][th])) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad DHT: codes do not fit");
          hd_ok[tc][th] = true;
        }
        p += 17 + cnt;
      }
    } else if (m == 0xDB) {                                // DQT
      long p = 0;
      while (p < sl) {
        const int pq = s[p] >> 4, tq = s[p] & 15;
        if (pq > 1 || tq > 3) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad DQT");
        if (pq == 1) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_QUANT16, "a 16-bit quantisation table");
        if (p + 65 > sl) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad DQT");
        memcpy(qt[tq], s + p + 1, 64);
        qt_ok[tq] = true;
        p += 65;
      }
    } else if (m == 0xDD) {
      if (sl != 2) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad DRI");
      ri = rd16(s);
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xE1) {
      if (orientation == 0) orientation = exif_orientation(s, sl);
      if (sl >= 29 && memcmp(s, "http://ns.adobe.com/xap/1.0/", 28) == 0 && contains(s, sl, "Orientation")) xmp_orientation = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = s[11];
      }
    } else if (m == 0xDA) {
      if (!have_sof || sl < 1) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "SOS before SOF0");
      const int ns = s[0];
      if (ns != P->ncomp) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_SCANS, "the first scan does not hold every component");
      if (sl != 4 + 2 * ns) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad SOS");
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != cid[c]) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "SOS names components in another order");
        ctd[c] = s[2 + 2 * c] >> 4;
        cta[c] = s[2 + 2 * c] & 15;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_HEADER, "bad SOS: not 0..63");
      scan_off = i + len;
    }
    // APPn, COM and everything else with a length: skipped
    i += len;
  }
  if (3L * P->h * P->w >= (1L << 31)) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_SIZE, "3 h w >= 2^31");
  if (P->ncomp == 3) {
    if (adobe && adobe_transform == 0) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_ADOBE, "Adobe APP14 with transform 0");
    if (!jfif && !adobe && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B')
      DVD_JPEGDEC_REFUSE(DVD_E_JPEG_COMPONENTS, "component ids R, G, B without JFIF: an RGB file");
    const bool luma_ok = (chs[0] == 1 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 2);
    if (!luma_ok || chs[1] != 1 || cvs[1] != 1 || chs[2] != 1 || cvs[2] != 1)
      DVD_JPEGDEC_REFUSE(DVD_E_JPEG_SAMPLING, "sampling other than 4:4:4, 4:2:2 (2x1) or 4:2:0");
  } else if (chs[0] != 1 || cvs[0] != 1) {
    DVD_JPEGDEC_REFUSE(DVD_E_JPEG_SAMPLING, "a single component not sampled 1x1");
  }
  for (int c = 0; c < P->ncomp; ++c) {
    if (ctq[c] > 3 || !qt_ok[ctq[c]]) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_TABLE, "a quantisation table is missing");
    if (ctd[c] > 1 || cta[c] > 1 || !hd_ok[0][ctd[c]] || !hd_ok[1][cta[c]]) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_TABLE, "a Huffman table is missing");
  }
  if (orientation == 0 && xmp_orientation) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_ORIENTATION, "no EXIF orientation, but an XMP packet names one");
  // the entropy-coded data: up to the first marker that is neither a stuffed FF 00 nor RSTn (or the file's end)
  long j = scan_off;
  while (j < n) {
    if (f[j] != 0xFF) {
      ++j;
    } else if (j + 1 < n && (f[j + 1] == 0 || (f[j + 1] >= 0xD0 && f[j + 1] <= 0xD7))) {
      j += 2;
    } else {
      break;
    }
  }
  const long scan_end = j;
  while (j < n && f[j] == 0xFF) ++j;
  if (j < n && f[j] != 0xD9) DVD_JPEGDEC_REFUSE(DVD_E_JPEG_SCANS, "more than one scan (a marker other than EOI follows the first)");
#undef DVD_JPEGDEC_REFUSE
  P->hs = chs[0];
  P->vs = cvs[0];
  P->mcus_x = (P->w + 8 * P->hs - 1) / (8 * P->hs);
  P->mcus_y = (P->h + 8 * P->vs - 1) / (8 * P->vs);
  P->bpm = P->ncomp == 1 ? 1 : P->hs * P->vs + 2;
  P->ri = ri;
  P->orientation = orientation ? orientation : 1;
  P->out_h = P->orientation >= 5 ? P->w : P->h;
  P->out_w = P->orientation >= 5 ? P->h : P->w;
  for (int s = 0; s < P->bpm; ++s) {
    const int c = P->ncomp == 1 || s < P->bpm - 2 ? 0 : s - (P->bpm - 2) + 1;
    P->dc_mask |= (unsigned)ctd[c] << s;
    P->ac_mask |= (unsigned)cta[c] << s;
  }
  P->scan_off = scan_off;
  P->scan_len = scan_end - scan_off;
  P->nblocks = (long)P->mcus_x * P->mcus_y * P->bpm;
  P->nsub = (P->scan_len + kSubseq - 1) / kSubseq;
  for (int c = 0; c < P->ncomp; ++c) memcpy(P->q[c], qt[ctq[c]], 64);
  for (int t = 0; t < 4; ++t) {
    if (hd_ok[t >> 1][t & 1]) memcpy(P->huff + t * kHuffWords, &hd[t >> 1][t & 1], sizeof(HuffDec));
  }
  return 0;
}

// Device scratch of one decode: byte offsets, each a multiple of 256.
struct Layout {
  size_t state, chg0, chg1, ctr, counts, first, flags, agg, coef, plane[3], total;
  long nchunks;
  int pitch[3], rows[3];
};
inline Layout layout_of(const Plan& P) {
  Layout l;
  const long mcus = (long)P.mcus_x * P.mcus_y;
  l.nchunks = (mcus + kDcChunk - 1) / kDcChunk;
  Carver cv;
  l.state = cv.take((size_t)(P.nsub + 1) * 8);
  l.chg0 = cv.take((size_t)P.nsub + 1);
  l.chg1 = cv.take((size_t)P.nsub + 1);
  l.ctr = cv.take(256);
  l.counts = cv.take((size_t)P.nsub * 4 + 4);
  l.first = cv.take((size_t)P.nsub * 4 + 4);
  l.flags = cv.take((size_t)mcus);
  l.agg = cv.take((size_t)l.nchunks * 16);
  l.coef = cv.take((size_t)P.nblocks * 128);
  for (int c = 0; c < 3; ++c) {
    l.pitch[c] = P.mcus_x * 8 * (c == 0 ? P.hs : 1);
    l.rows[c] = P.mcus_y * 8 * (c == 0 ? P.vs : 1);
    l.plane[c] = cv.take(c < P.ncomp ? (size_t)l.pitch[c] * l.rows[c] : 0);   // a grey file has one plane
  }
  l.total = cv.at;
  return l;
}

// ---------------------------------------------------------------- the byte reader -------------------------------------------
constexpr int kData = 0, kRst = 1, kEnd = 2;
// The byte of the entropy-coded data at index i of scan d[0..n): kData (*v, and *next = the index behind it: FF 00 is one
// byte FF), kRst (FF D0..D7 stands there; *next = the index behind the marker) or kEnd.
DVD_HD int fetch(const uint8_t* d, long n, long i, int* v, long* next) {
  *v = 0;
  *next = i;
  if (i >= n) return kEnd;
  const int b = d[i];
  if (b != 0xFF) {
    *v = b;
    *next = i + 1;
    return kData;
  }
  if (i + 1 >= n) return kEnd;
  const int m = d[i + 1];
  if (m == 0) {
    *v = 0xFF;
    *next = i + 2;
    return kData;
  }
  if (m >= 0xD0 && m <= 0xD7) {
    *next = i + 2;
    return kRst;
  }
  return kEnd;
}

// The 16 bits at bit position p (of the raw scan: byte p / 8, bit p % 8 from the top), stuffing stepped over.  avail = how
// many of them are data; behind them stands `kind` (kData: more data), for kRst with `resume` = the byte behind the marker.
struct Peek {
  uint32_t bits;
  int avail, kind;
  long resume;
};
DVD_HD Peek peek(const uint8_t* d, long n, long p) {
  long i = p >> 3;
  const int off = (int)(p & 7);
  uint32_t acc = 0;
  int got = 0, kind = kData;
  long resume = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    int v = 0;
    if (kind == kData) {
      long nx;
      kind = fetch(d, n, i, &v, &nx);
      if (kind == kData) {
        i = nx;
        got += 8;
      } else {
        resume = nx;
      }
    }
    acc = (acc << 8) | (uint32_t)v;
  }
  Peek w;
  w.bits = (acc >> (8 - off)) & 0xFFFFu;
  w.avail = got - off < 0 ? 0 : got - off > 16 ? 16 : got - off;
  w.kind = kind;
  w.resume = resume;
  return w;
}
// p + l bits, l <= 16, all of them data that peek has seen: at most two byte steps, each over a stuffed pair if it is one
DVD_HD long advance(const uint8_t* d, long n, long p, int l) {
  long i = p >> 3;
  int t = (int)(p & 7) + l;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (t >= 8) {
      i += (d[i] == 0xFF && i + 1 < n && d[i + 1] == 0) ? 2 : 1;
      t -= 8;
    }
  }
  return i * 8 + t;
}

// ---------------------------------------------------------------- the walk --------------------------------------------------
// state = bit position << 16 | block slot within the MCU << 8 | zig-zag index
DVD_HD unsigned long long pack_state(long pos, int slot, int k) { return ((unsigned long long)pos << 16) | ((unsigned)slot << 8) | (unsigned)k; }
DVD_HD unsigned long long guess_state(long j) { return pack_state(j * kSubseq * 8, 0, 0); }

struct NullSink {
  DVD_HD void coef(int, int) {}
  DVD_HD void block_done() {}
  DVD_HD void restart() {}
};
struct CountSink {
  unsigned n;
  DVD_HD void coef(int, int) {}
  DVD_HD void block_done() { ++n; }
  DVD_HD void restart() {}
};
// Coefficients in zig-zag order (index 0: the DC difference) into out[nblocks][64], zero beforehand; the MCU whose first block
// starts behind a restart marker is flagged.  Every index is checked.
struct WriteSink {
  int16_t* out;
  uint8_t* flags;
  long nblocks, blk;
  int bpm;
  DVD_HD void coef(int k, int v) {
    if (blk >= 0 && blk < nblocks && k >= 0 && k < 64) out[blk * 64 + k] = (int16_t)v;
  }
  DVD_HD void block_done() { ++blk; }
  DVD_HD void restart() {
    if (blk >= 0 && blk < nblocks && blk % bpm == 0) flags[blk / bpm] = 1;
  }
};

// Decodes from `state` until the position reaches stop_bits and returns the state there.  A restart marker in the way sets
// (byte behind it, slot 0, index 0) whatever was being decoded; an invalid code, an impossible run or the end of the scan
// returns the fresh guess (stop_bits, 0, 0).  Every pass of the loop consumes at least one bit or steps over a marker.
template <class Sink>
DVD_HD unsigned long long walk(const HuffDec* tabs, unsigned dc_mask, unsigned ac_mask, int bpm, const uint8_t* d, long n,
                               unsigned long long state, long stop_bits, Sink& sink) {
  long p = (long)(state >> 16);
  int slot = (int)((state >> 8) & 255), k = (int)(state & 255);
  const unsigned long long fresh = pack_state(stop_bits, 0, 0);
  if (slot >= bpm || k > 63) return fresh;
  for (long budget = stop_bits - p + 8; p < stop_bits && budget > 0; --budget) {
    const HuffDec& t = tabs[k == 0 ? (int)((dc_mask >> slot) & 1u) : 2 + (int)((ac_mask >> slot) & 1u)];
    const Peek w = peek(d, n, p);
    int len = 0, sym = 0;
#pragma unroll 1
    for (int l = 1; l <= 16; ++l) {
      const int code = (int)(w.bits >> (16 - l));
      if (code <= t.maxcode[l]) {
        len = l;
        sym = t.vals[(t.valoff[l] + code) & 255];
        break;
      }
    }
    int s = 0, v = 0;
    long p1 = p;
    bool short_of_bits = len == 0 || len > w.avail;
    int kind = w.kind;
    long resume = w.resume;
    if (!short_of_bits) {
      p1 = advance(d, n, p, len);
      s = k == 0 ? sym : (sym & 15);
      if (s > 15) return fresh;                            // a DC category that does not exist
      if (s) {
        const Peek w2 = peek(d, n, p1);
        if (s > w2.avail) {
          short_of_bits = true;
          kind = w2.kind;
          resume = w2.resume;
        } else {
          const int raw = (int)(w2.bits >> (16 - s));
          v = raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
          p1 = advance(d, n, p1, s);
        }
      }
    }
    if (short_of_bits) {
      // the symbol does not end in front of what follows the data: a marker restarts the decoder, anything else ends the walk
      if (kind != kRst || (len == 0 && w.avail >= 16)) return fresh;
      p = resume * 8;
      slot = 0;
      k = 0;
      sink.restart();
      continue;
    }
    if (k == 0) {
      sink.coef(0, v);
      k = 1;
    } else if (s == 0) {
      k = (sym >> 4) == 15 ? k + 16 : 64;                  // ZRL, or EOB
    } else {
      k += sym >> 4;
      if (k > 63) return fresh;
      sink.coef(k, v);
      ++k;
    }
    if (k >= 64) {
      sink.block_done();
      slot = slot + 1 == bpm ? 0 : slot + 1;
      k = 0;
    }
    p = p1;
  }
  return p < stop_bits ? fresh : pack_state(p, slot, k);
}

// ---------------------------------------------------------------- IDCT ------------------------------------------------------
// libjpeg's accurate integer IDCT (jidctint: 13 constant bits), one dimension.  shift = 11 for the column pass (2 extra bits
// are kept), 18 for the row pass.  Unsigned arithmetic: the same bits as libjpeg's for every file an encoder can write, and
// wrap-around instead of overflow for coefficients none can.
DVD_HD void idct_1d(const uint32_t in[8], int32_t out[8], int shift) {
  typedef uint32_t U;
  U z2 = in[2], z3 = in[6];
  U z1 = (z2 + z3) * 4433u;
  U tmp2 = z1 + z3 * (U)(-15137);
  U tmp3 = z1 + z2 * 6270u;
  z2 = in[0];
  z3 = in[4];
  U tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
  const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  U z4 = tmp1 + tmp3;
  const U z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u;
  tmp1 *= 16819u;
  tmp2 *= 25172u;
  tmp3 *= 12299u;
  z1 *= (U)(-7373);
  z2 *= (U)(-20995);
  z3 *= (U)(-16069);
  z4 *= (U)(-3196);
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const U r = 1u << (shift - 1);
  out[0] = (int32_t)(tmp10 + tmp3 + r) >> shift;
  out[7] = (int32_t)(tmp10 - tmp3 + r) >> shift;
  out[1] = (int32_t)(tmp11 + tmp2 + r) >> shift;
  out[6] = (int32_t)(tmp11 - tmp2 + r) >> shift;
  out[2] = (int32_t)(tmp12 + tmp1 + r) >> shift;
  out[5] = (int32_t)(tmp12 - tmp1 + r) >> shift;
  out[3] = (int32_t)(tmp13 + tmp0 + r) >> shift;
  out[4] = (int32_t)(tmp13 - tmp0 + r) >> shift;
}
// libjpeg's centred range table on v & 1023: clamp(v + 128) whenever |v| < 512
DVD_HD int sample_of(int32_t v) {
  const int x = v & 1023;
  return x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896;
}
// the component of block slot s of an MCU
DVD_HD int comp_of_slot(int s, int bpm, int ncomp) { return ncomp == 1 || s < bpm - 2 ? 0 : s - (bpm - 2) + 1; }

// ---------------------------------------------------------------- upsampling, colour, orientation ---------------------------
// "fancy" h2v1 (jdsample h2v1_fancy_upsample): output sample x of a row of cw input samples, cw > 2
DVD_HD int up_h2v1(const uint8_t* row, int cw, int x) {
  const int i = x >> 1, c = row[i];
  if (x & 1) return i == cw - 1 ? c : (3 * c + row[i + 1] + 2) >> 2;
  return i == 0 ? c : (3 * c + row[i - 1] + 1) >> 2;
}
// "fancy" h2v2: cur = the chroma row of the output row, nb = the nearer neighbouring row (clamped at the edges), cw > 2
DVD_HD int up_h2v2(const uint8_t* cur, const uint8_t* nb, int cw, int x) {
  const int i = x >> 1, cs = 3 * cur[i] + nb[i];
  if (x & 1) return i == cw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * cur[i + 1] + nb[i + 1] + 7) >> 4;
  return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * cur[i - 1] + nb[i - 1] + 8) >> 4;
}
// The chroma sample of output pixel (y, x) from a plane of pitch `pitch` cropped to ch x cw
DVD_HD int chroma_at(const uint8_t* plane, int pitch, int hs, int vs, int ch, int cw, int y, int x) {
  if (hs == 1) return plane[(size_t)y * pitch + x];
  if (vs == 1) {
    const uint8_t* row = plane + (size_t)y * pitch;
    return cw <= 2 ? row[x >> 1] : up_h2v1(row, cw, x);
  }
  const int j = y >> 1;
  if (cw <= 2) return plane[(size_t)j * pitch + (x >> 1)];
  const int jn = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
  return up_h2v2(plane + (size_t)j * pitch, plane + (size_t)jn * pitch, cw, x);
}
DVD_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// jdcolor's YCbCr -> RGB in 16-bit fixed point; >> of a negative int is the arithmetic shift
DVD_HD void ycc_rgb(int y, int cb, int cr, int* r, int* g, int* b) {
  cb -= 128;
  cr -= 128;
  *r = clamp255(y + ((91881 * cr + 32768) >> 16));
  *g = clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  *b = clamp255(y + ((116130 * cb + 32768) >> 16));
}
// where pixel (y, x) of the h x w image lies in the image transposed as EXIF orientation o asks (ImageOps.exif_transpose)
DVD_HD void oriented(int o, int h, int w, int y, int x, int* yo, int* xo) {
  switch (o) {
    case 2: *yo = y; *xo = w - 1 - x; break;               // mirrored
    case 3: *yo = h - 1 - y; *xo = w - 1 - x; break;       // rotated by 180
    case 4: *yo = h - 1 - y; *xo = x; break;               // flipped
    case 5: *yo = x; *xo = y; break;                       // transposed
    case 6: *yo = x; *xo = h - 1 - y; break;               // rotated clockwise
    case 7: *yo = w - 1 - x; *xo = h - 1 - y; break;       // transverse
    case 8: *yo = w - 1 - x; *xo = y; break;               // rotated counter-clockwise
    default: *yo = y; *xo = x; break;
  }
}

}  // namespace jpegdec
}  // namespace dvd
