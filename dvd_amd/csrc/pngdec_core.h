// The PNG decoder's arithmetic, shared by the kernels of pngdec.hip and by the stand-alone CPU restatement
// pngdec_host_check.cpp (plain C++, no HIP): the chunk parser and the refusals (host only), the bit reader, the check of a
// dynamic block's header - exactly the checks zlib's inflate applies, used by the block finder and by the decoder alike -, the
// canonical decode tables, the symbol walk over one segment of the deflate stream, the chain over the segments (host only)
// and the five filters.  DESIGN.md section 4.9 holds the definition.  Everything is integer arithmetic and a pure function
// of its arguments; no read leaves the padded payload and every loop is bounded by a constant, by the work budget or by the
// bits of the stream.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hd.h"
#include "png_core.h"   // length / distance symbol arithmetic, the fixed code, cl_order, paeth, CRC-32 and Adler-32 pieces
#include "workspace.h"

namespace dvd {
namespace pngdec {

constexpr long kDefaultMaxWork = 1L << 20;   // symbols + stored bytes one lane of the inflate may spend
constexpr int kGroup = 4;                    // doubling rounds launched between two read-backs
constexpr int kLanes = 32;                   // lanes (segments) per workgroup of the count and write passes
constexpr long kMaxCand = 1L << 16;          // rows of the candidate table; more candidates than this is NOSPLIT
constexpr int kAdlerBlock = 16384;           // inflated bytes per Adler-32 partial
constexpr int kPad = 16;                     // zero bytes behind the payload, so that a 64-bit window never leaves it

// status bits the kernels raise (ctr[kCtrStatus]); any of them is DVD_E_PNG_DATA
constexpr uint32_t kStCrc = 1, kStDistance = 2, kStAdler = 4, kStFilter = 8, kStOverflow = 16;
constexpr int kCtrStamp = 0, kCtrCand = 1, kCtrStatus = 2, kCtrBands = 3, kCtrAdler = 4;

// one IDAT chunk: where its data lies in the file, its length, and the payload bytes in front of it
struct Idat {
  unsigned long long off;
  uint32_t len, pre;
};

// What the kernels need of the header; passed by value.
struct Plan {
  int h, w, ctype, bpp;
  long stride;      // 1 + w bpp: a row of the inflated stream with its filter byte
  long inflated;    // h stride
  long nidat;       // IDAT chunks, empty ones included
  long payload;     // their bytes together: zlib header, deflate stream, Adler-32
  long nbits;       // bit positions of the deflate stream: 8 payload - 16
  long ncap;        // rows of the candidate table
};

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// ---------------------------------------------------------------- header (host only) ----------------------------------------
// The file's chunks -> *P and the IDAT table; 0, or the refusal code with *why naming the reason.
inline int parse(const uint8_t* f, long n, Plan* P, std::vector<Idat>* idat, const char** why) {
  memset(P, 0, sizeof *P);
  idat->clear();
#define DVD_PNGDEC_REFUSE(code, text) \
  do {                                \
    *why = text;                      \
    return code;                      \
  } while (0)
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (n < 8 || memcmp(f, sig, 8) != 0) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "no PNG signature");
  bool have_ihdr = false, seen_idat = false, idat_done = false, iend = false;
  int depth = 0, interlace = 0;
  unsigned long long payload = 0;
  long i = 8;
  while (!iend) {
    if (i + 12 > n) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "truncated chunk layout (no IEND)");
    const unsigned long long len = be32(f + i);
    if (len > 0x7FFFFFFFull || (unsigned long long)i + 12 + len > (unsigned long long)n)
      DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "a chunk runs past the end of the file");
    const uint8_t* type = f + i + 4;
    const uint8_t* d = f + i + 8;
    auto is = [&](const char* t) { return memcmp(type, t, 4) == 0; };
    if (!have_ihdr) {
      if (!is("IHDR") || len != 13) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "the first chunk is not IHDR");
      if (~png::crc_bytes(0xFFFFFFFFu, type, 17) != be32(d + 13)) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "IHDR fails its CRC-32");
      const uint32_t w = be32(d), h = be32(d + 4);
      if (w < 1 || h < 1 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "bad IHDR: a side of 0 or above 2^31 - 1");
      depth = d[8];
      P->ctype = d[9];
      interlace = d[12];
      if (P->ctype != 0 && P->ctype != 2 && P->ctype != 3 && P->ctype != 4 && P->ctype != 6)
        DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "bad IHDR: no such colour type");
      if (d[10] != 0 || d[11] != 0 || interlace > 1) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "bad IHDR: compression, filter or interlace method");
      if (interlace == 1) DVD_PNGDEC_REFUSE(DVD_E_PNG_INTERLACE, "Adam7 interlace");
      if (P->ctype == 3 || P->ctype == 4) DVD_PNGDEC_REFUSE(DVD_E_PNG_COLOUR, "colour type 3 (palette) or 4 (gray + alpha)");
      if (depth != 8) DVD_PNGDEC_REFUSE(DVD_E_PNG_DEPTH, "bit depth other than 8");
      if (3ull * h * w >= (1ull << 31)) DVD_PNGDEC_REFUSE(DVD_E_PNG_SIZE, "3 h w >= 2^31");
      P->h = (int)h;
      P->w = (int)w;
      P->bpp = P->ctype == 0 ? 1 : P->ctype == 2 ? 3 : 4;
      have_ihdr = true;
    } else if (is("IHDR")) {
      DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "a second IHDR");
    } else if (is("IDAT")) {
      if (idat_done) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "IDAT chunks that are not consecutive");
      seen_idat = true;
      if (payload + len >= (1ull << 29)) DVD_PNGDEC_REFUSE(DVD_E_PNG_SIZE, "2^29 bytes of IDAT data or more");
      idat->push_back(Idat{(unsigned long long)(i + 8), (uint32_t)len, (uint32_t)payload});
      payload += len;
    } else {
      if (seen_idat) idat_done = true;
      if (is("IEND")) {
        iend = true;
      } else if (is("tRNS")) {
        DVD_PNGDEC_REFUSE(DVD_E_PNG_TRNS, "a tRNS chunk");
      } else if (is("acTL")) {
        DVD_PNGDEC_REFUSE(DVD_E_PNG_APNG, "an acTL chunk (APNG)");
      } else if (is("eXIf")) {
        DVD_PNGDEC_REFUSE(DVD_E_PNG_METADATA, "an eXIf chunk");
      } else if (is("tEXt") || is("zTXt") || is("iTXt")) {
        unsigned long long k = 0;
        while (k < len && d[k]) ++k;
        if ((k >= 16 && memcmp(d, "Raw profile type", 16) == 0) || (k == 17 && memcmp(d, "XML:com.adobe.xmp", 17) == 0))
          DVD_PNGDEC_REFUSE(DVD_E_PNG_METADATA, "a text chunk that may carry an orientation (Raw profile type / XML:com.adobe.xmp)");
      } else if (!(type[0] & 0x20) && !is("PLTE")) {
        DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "an unknown critical chunk");
      }
    }
    i += 12 + (long)len;
  }
  if (!seen_idat) DVD_PNGDEC_REFUSE(DVD_E_PNG_HEADER, "no IDAT chunk");
  // the zlib header: the first two payload bytes, wherever the chunk cuts put them
  int zh[2], got = 0;
  for (size_t k = 0; k < idat->size() && got < 2; ++k)
    for (uint32_t b = 0; b < (*idat)[k].len && got < 2; ++b) zh[got++] = f[(*idat)[k].off + b];
  if (got < 2) DVD_PNGDEC_REFUSE(DVD_E_PNG_ZLIB, "no zlib header");
  if ((zh[0] & 15) != 8 || (zh[0] >> 4) > 7 || (zh[0] * 256 + zh[1]) % 31 != 0) DVD_PNGDEC_REFUSE(DVD_E_PNG_ZLIB, "bad zlib header");
  if (zh[1] & 0x20) DVD_PNGDEC_REFUSE(DVD_E_PNG_ZLIB, "a preset dictionary");
#undef DVD_PNGDEC_REFUSE
  P->stride = 1 + (long)P->w * P->bpp;
  P->inflated = (long)P->h * P->stride;
  P->nidat = (long)idat->size();
  P->payload = (long)payload;
  P->nbits = P->payload * 8 - 16;
  P->ncap = (P->nbits < kMaxCand ? (P->nbits > 1 ? P->nbits : 1) : kMaxCand);
  return 0;
}
// the least payload that can hold a stream: header 2, one byte of deflate data, Adler-32 4
constexpr long kMinPayload = 7;

// one row of the candidate table: where the segment starts, and what the count pass found
constexpr uint32_t kSegFinal = 1, kSegBad = 2, kSegBudget = 4;
struct Seg {
  uint32_t pos, end, nbytes, flags;
};
// one reachable segment for the write pass
struct Reach {
  uint32_t pos, out_off, nbytes, pad;
};

// Device scratch of one decode: byte offsets, each a multiple of 256.
struct Layout {
  size_t idat, payload, masks, prefix, ctr, cand, reach, val, src, adler, band, total;
  long nwords, nmasks, nchunks, nparts;
};
inline Layout layout_of(const Plan& P) {
  Layout l;
  l.nwords = (P.payload + kPad) / 4;
  l.nmasks = (P.nbits + 63) / 64;
  l.nchunks = (l.nmasks + 3) / 4;
  l.nparts = (P.inflated + kAdlerBlock - 1) / kAdlerBlock;
  Carver cv;
  l.idat = cv.take((size_t)P.nidat * sizeof(Idat));
  l.payload = cv.take((size_t)l.nwords * 4 + 4);
  l.masks = cv.take((size_t)l.nchunks * 32);
  l.prefix = cv.take((size_t)l.nchunks * 4 + 4);
  l.ctr = cv.take(256);
  l.cand = cv.take((size_t)P.ncap * sizeof(Seg));
  l.reach = cv.take((size_t)P.ncap * sizeof(Reach));
  l.val = cv.take((size_t)P.inflated);
  l.src = cv.take((size_t)P.inflated * 4);
  l.adler = cv.take((size_t)l.nparts * 8);
  l.band = cv.take((size_t)P.h * 4 + 4);
  l.total = cv.at;
  return l;
}

// ---------------------------------------------------------------- bits -------------------------------------------------------
// The payload as little-endian 32-bit words (nwords of them, zero behind the payload); a read outside them gives zeros.
struct Bits {
  const uint32_t* w;
  long nwords;
  DVD_HD uint32_t word(long i) const { return i < nwords ? w[i] : 0u; }
  DVD_HD uint32_t peek(unsigned long long pos) const {   // the 32 bits from bit position pos on, LSB first
    const long i = (long)(pos >> 5);
    const int s = (int)(pos & 31);
    const uint32_t lo = word(i), hi = word(i + 1);
    return s ? (lo >> s) | (hi << (32 - s)) : lo;
  }
  DVD_HD uint32_t byte(unsigned long long i) const { return (word((long)(i >> 2)) >> (8 * (int)(i & 3))) & 255u; }
};

// ---------------------------------------------------------------- a dynamic block's header -----------------------------------
// What zlib checks of the two codes a header describes: each complete (Kraft sum exactly 1), or - zlib's `max == 1` - a
// single code of one bit, or (the distance code only, as symbol 256 gives the other a length) no code at all.
struct CodeCheck {
  uint32_t kraft_ll, kraft_d;   // in units of 2^-15
  int used_ll, used_d;
  bool eob;
  DVD_HD void len(int i, int hlit, int l) {
    if (!l) return;
    if (i < hlit) {
      kraft_ll += 32768u >> l;
      ++used_ll;
      if (i == 256) eob = true;
    } else {
      kraft_d += 32768u >> l;
      ++used_d;
    }
  }
  DVD_HD static bool code_ok(uint32_t kraft, int used) { return kraft == 32768u || (used == 1 && kraft == 16384u) || used == 0; }
  DVD_HD bool ok() const { return eob && code_ok(kraft_ll, used_ll) && code_ok(kraft_d, used_d); }
};
struct NoStore {
  DVD_HD void len(int, int, int) {}
};

// The header of a dynamic block whose HLIT field stands at *pos (behind BFINAL and BTYPE): HLIT <= 29, HDIST <= 29, a complete
// code-length code, HLIT + HDIST lengths with no repeat before the first and no overrun, a length for symbol 256, two codes
// that pass CodeCheck.  True, *pos behind the header and the lengths handed to store.len(i, hlit, l), or false.  The
// code-length code lives in registers: its nineteen 3-bit lengths in one 64-bit word, the seven 5-bit counts in another.
template <class Store>
DVD_HD bool dyn_header(const Bits& B, unsigned long long* pos, unsigned long long endbits, Store& store, int* hlit_out,
                       int* hdist_out) {
  unsigned long long p = *pos;
  uint32_t v = B.peek(p);
  const int hlit = (int)(v & 31u) + 257, hdist = (int)((v >> 5) & 31u) + 1, hclen = (int)((v >> 10) & 15u) + 4;
  if (hlit > 286 || hdist > 30) return false;
  p += 14;
  unsigned long long cl = 0, counts = 0;
  uint32_t kraft = 0;
  for (int k = 0; k < hclen; ++k) {
    if (k % 10 == 0) v = B.peek(p + 3 * (unsigned)k);
    const uint32_t l = (v >> (3 * (k % 10))) & 7u;
    cl |= (unsigned long long)l << (3 * png::cl_order(k));
    if (l) {
      kraft += 128u >> l;
      counts += 1ull << (5 * (l - 1));
    }
  }
  p += 3 * (unsigned)hclen;
  if (kraft != 128u || p > endbits) return false;
  CodeCheck chk{0, 0, 0, 0, false};
  const int total = hlit + hdist;
  int i = 0, prev = 0;
  while (i < total) {
    if (p > endbits) return false;
    v = B.peek(p);
    int code = 0, first = 0, index = 0, l = 1, k = -1;
    for (; l <= 7; ++l) {
      code |= (int)((v >> (l - 1)) & 1u);
      const int count = (int)((counts >> (5 * (l - 1))) & 31u);
      if (code - count < first) {
        k = index + (code - first);
        break;
      }
      index += count;
      first = (first + count) << 1;
      code <<= 1;
    }
    if (k < 0) return false;                    // cannot happen for a complete code
    k -= index;                                 // the k-th symbol, in symbol order, among those of length l
    int sym = 0;
    for (; sym < 19; ++sym)
      if ((int)((cl >> (3 * sym)) & 7u) == l && k-- == 0) break;
    p += (unsigned)l;
    v >>= l;
    if (sym < 16) {
      chk.len(i, hlit, sym);
      store.len(i, hlit, sym);
      ++i;
      prev = sym;
    } else {
      int rep, val = 0;
      if (sym == 16) {
        if (i == 0) return false;
        val = prev;
        rep = 3 + (int)(v & 3u);
        p += 2;
      } else if (sym == 17) {
        rep = 3 + (int)(v & 7u);
        p += 3;
      } else {
        rep = 11 + (int)(v & 127u);
        p += 7;
      }
      if (i + rep > total) return false;
      for (; rep > 0; --rep, ++i) {
        chk.len(i, hlit, val);
        store.len(i, hlit, val);
      }
      prev = val;
    }
  }
  if (p > endbits || !chk.ok()) return false;
  *pos = p;
  *hlit_out = hlit;
  *hdist_out = hdist;
  return true;
}

// The block finder's test of bit position pos: a dynamic block with a header zlib accepts starts there.
DVD_HD bool is_candidate(const Bits& B, unsigned long long pos, unsigned long long endbits) {
  const uint32_t v = B.peek(pos);
  if (((v >> 1) & 3u) != 2u) return false;
  NoStore none;
  unsigned long long p = pos + 3;
  int hlit, hdist;
  return dyn_header(B, &p, endbits, none, &hlit, &hdist);
}

// ---------------------------------------------------------------- decode tables ----------------------------------------------
// One lane's two canonical codes: symbols sorted by (length, symbol) and the count per length, decoded one bit at a time.
// S lanes share the arrays, lane-interleaved (LDS on the device: neighbouring lanes hit neighbouring banks); S = 1 on the host.
constexpr int kTabHalves = 288 + 32 + 16 + 16 + 16, kTabBytes = 288 + 32;
template <int S>
struct Tab {
  uint16_t* hw;   // [kTabHalves][S]
  uint8_t* by;    // [kTabBytes][S]
  int lane;
  DVD_HD uint16_t& ll_sym(int i) { return hw[i * S + lane]; }
  DVD_HD uint16_t& d_sym(int i) { return hw[(288 + i) * S + lane]; }
  DVD_HD uint16_t& ll_cnt(int i) { return hw[(320 + i) * S + lane]; }
  DVD_HD uint16_t& d_cnt(int i) { return hw[(336 + i) * S + lane]; }
  DVD_HD uint16_t& offs(int i) { return hw[(352 + i) * S + lane]; }
  DVD_HD uint8_t& len(int i) { return by[i * S + lane]; }   // 0..287 literal/length, 288..319 distance
  // from len(0 .. nll) and len(288 .. 288 + nd)
  DVD_HD void build(int nll, int nd) {
    for (int l = 0; l < 16; ++l) {
      ll_cnt(l) = 0;
      d_cnt(l) = 0;
    }
    for (int i = 0; i < nll; ++i) ++ll_cnt(len(i));
    for (int i = 0; i < nd; ++i) ++d_cnt(len(288 + i));
    ll_cnt(0) = 0;
    d_cnt(0) = 0;
    offs(1) = 0;
    for (int l = 1; l < 15; ++l) offs(l + 1) = (uint16_t)(offs(l) + ll_cnt(l));
    for (int i = 0; i < nll; ++i)
      if (len(i)) ll_sym(offs(len(i))++) = (uint16_t)i;
    offs(1) = 0;
    for (int l = 1; l < 15; ++l) offs(l + 1) = (uint16_t)(offs(l) + d_cnt(l));
    for (int i = 0; i < nd; ++i)
      if (len(288 + i)) d_sym(offs(len(288 + i))++) = (uint16_t)i;
  }
  // the symbol whose code starts at bit 0 of v, *nbits its length; -1 if no code does
  DVD_HD int decode(bool dist, uint32_t v, int* nbits) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
      code |= (int)((v >> (l - 1)) & 1u);
      const int count = dist ? d_cnt(l) : ll_cnt(l);
      if (code - count < first) {
        *nbits = l;
        return dist ? d_sym(index + (code - first)) : ll_sym(index + (code - first));
      }
      index += count;
      first = (first + count) << 1;
      code <<= 1;
    }
    return -1;
  }
};
template <int S>
struct TabStore {
  Tab<S>& t;
  DVD_HD void len(int i, int hlit, int l) { t.len(i < hlit ? i : 288 + (i - hlit)) = (uint8_t)l; }
};

// least length of length symbol 257..285 and least distance of distance symbol 0..29: png_core.h's len_symbol / dist_symbol
// read backwards
DVD_HD int len_base(int sym) {
  if (sym == 285) return 258;
  if (sym < 265) return sym - 257 + 3;
  return 3 + ((4 + (sym - 261) % 4) << png::len_extra_bits((uint32_t)sym));
}
DVD_HD int dist_base(int sym) { return sym < 4 ? sym + 1 : 1 + ((2 + (sym & 1)) << png::dist_extra_bits((uint32_t)sym)); }

// ---------------------------------------------------------------- the walk ---------------------------------------------------
struct CountSink {
  unsigned long long n;
  DVD_HD void literal(uint32_t) { ++n; }
  DVD_HD void match(int len, int) { n += (unsigned)len; }
};
// Output byte i: a literal is val[i] with src[i] = i, a match byte src[i] = i - distance.  No store outside [0, limit).
struct WriteSink {
  uint8_t* val;
  uint32_t* src;
  unsigned long long n, limit;
  uint32_t bad;   // kStDistance: a distance reaching before the start of the stream; kStOverflow: more bytes than counted
  DVD_HD void literal(uint32_t v) {
    if (n < limit) {
      val[n] = (uint8_t)v;
      src[n] = (uint32_t)n;
    } else {
      bad |= kStOverflow;
    }
    ++n;
  }
  DVD_HD void match(int len, int dist) {
    for (int k = 0; k < len; ++k, ++n) {
      if (n >= limit) {
        bad |= kStOverflow;
      } else if ((unsigned long long)dist > n) {
        bad |= kStDistance;
        val[n] = 0;
        src[n] = (uint32_t)n;
      } else {
        src[n] = (uint32_t)(n - (unsigned)dist);
      }
    }
  }
};

struct WalkResult {
  unsigned long long end;
  uint32_t flags;
};
// Decodes the segment that starts with the block at bit position pos: that block whatever its type, then every stored and
// fixed block behind it, until a block header of type 2 stands at the position (the next segment: `end`), the final block is
// done (kSegFinal), the data is invalid (kSegBad) or symbols + stored bytes exceed max_work (kSegBudget).
template <int S, class Sink>
DVD_HD WalkResult walk(const Bits& B, unsigned long long endbits, unsigned long long pos, Tab<S>& t, unsigned long long max_work,
                       Sink& sink) {
  unsigned long long work = 0;
  bool first = true;
  for (;;) {
    if (pos + 3 > endbits) return WalkResult{pos, kSegBad};
    uint32_t v = B.peek(pos);
    const bool bfinal = v & 1u;
    const int type = (int)((v >> 1) & 3u);
    if (type == 3) return WalkResult{pos, kSegBad};
    if (type == 2 && !first) return WalkResult{pos, 0};
    first = false;
    pos += 3;
    if (type == 0) {
      pos = (pos + 7) & ~7ull;
      if (pos + 32 > endbits) return WalkResult{pos, kSegBad};
      v = B.peek(pos);
      const uint32_t len = v & 0xFFFFu;
      if ((v >> 16) != (len ^ 0xFFFFu)) return WalkResult{pos, kSegBad};
      pos += 32;
      if (pos + 8ull * len > endbits) return WalkResult{pos, kSegBad};
      work += len;
      if (work > max_work) return WalkResult{pos, kSegBudget};
      for (uint32_t k = 0; k < len; ++k) sink.literal(B.byte((pos >> 3) + k));
      pos += 8ull * len;
    } else {
      if (type == 1) {
        for (int s = 0; s < 288; ++s) t.len(s) = (uint8_t)png::fixed_ll_len(s);
        for (int s = 0; s < 32; ++s) t.len(288 + s) = 5;
        t.build(288, 32);
      } else {
        TabStore<S> store{t};
        int hlit = 0, hdist = 0;
        if (!dyn_header(B, &pos, endbits, store, &hlit, &hdist)) return WalkResult{pos, kSegBad};
        t.build(hlit, hdist);
      }
      for (;;) {
        if (++work > max_work) return WalkResult{pos, kSegBudget};
        v = B.peek(pos);
        int nb = 0;
        const int sym = t.decode(false, v, &nb);
        if (sym < 0 || sym > 285) return WalkResult{pos, kSegBad};
        pos += (unsigned)nb;
        if (pos > endbits) return WalkResult{pos, kSegBad};
        if (sym < 256) {
          sink.literal((uint32_t)sym);
          continue;
        }
        if (sym == 256) break;
        const int eb = (int)png::len_extra_bits((uint32_t)sym);
        const int length = len_base(sym) + (int)((v >> nb) & ((1u << eb) - 1u));
        pos += (unsigned)eb;
        v = B.peek(pos);
        const int dsym = t.decode(true, v, &nb);
        if (dsym < 0 || dsym > 29) return WalkResult{pos, kSegBad};
        const int deb = (int)png::dist_extra_bits((uint32_t)dsym);
        const int dist = dist_base(dsym) + (int)((v >> nb) & ((1u << deb) - 1u));
        pos += (unsigned)(nb + deb);
        if (pos > endbits) return WalkResult{pos, kSegBad};
        sink.match(length, dist);
      }
    }
    if (bfinal) return WalkResult{pos, kSegFinal};
  }
}

// ---------------------------------------------------------------- the chain (host only) --------------------------------------
// From segment 0 along the ends the count pass left: a segment's end must be the start of a candidate (a binary search; the
// candidates the chain never lands on are the false ones).  Fills `reach` with the segments on the chain and their output
// offsets.  0, DVD_E_PNG_DATA or DVD_E_PNG_NOSPLIT; *adler_at = the payload byte where the Adler-32 stands.
inline int chain(const Seg* cand, long ncand, const Plan& P, std::vector<Reach>* reach, long* adler_at, const char** why) {
  reach->clear();
  long k = 0;
  unsigned long long total = 0;
  for (;;) {
    const Seg& s = cand[k];
    if (s.flags & kSegBudget) {
      *why = "a segment on the chain exceeded the work budget";
      return DVD_E_PNG_NOSPLIT;
    }
    if (s.flags & kSegBad) {
      *why = "an invalid block, code, length or distance";
      return DVD_E_PNG_DATA;
    }
    reach->push_back(Reach{s.pos, (uint32_t)total, s.nbytes, 0});
    total += s.nbytes;
    if (total > (unsigned long long)P.inflated) {
      *why = "the stream inflates to more than h (1 + w bpp) bytes";
      return DVD_E_PNG_DATA;
    }
    if (s.flags & kSegFinal) {
      *adler_at = (long)((s.end + 7) / 8);
      break;
    }
    long lo = k + 1, hi = ncand;                   // the candidate at bit position s.end
    while (lo < hi) {
      const long mid = (lo + hi) / 2;
      if (cand[mid].pos < s.end) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= ncand || cand[lo].pos != s.end) {
      *why = "a block header that no decoder accepts";
      return DVD_E_PNG_DATA;
    }
    k = lo;
  }
  if (total != (unsigned long long)P.inflated) {
    *why = "the stream inflates to fewer than h (1 + w bpp) bytes";
    return DVD_E_PNG_DATA;
  }
  if (*adler_at + 4 > P.payload) {
    *why = "no Adler-32 behind the stream";
    return DVD_E_PNG_DATA;
  }
  return 0;
}

// ---------------------------------------------------------------- filters ----------------------------------------------------
// The byte behind filter f: x = the filtered byte, a = left (bpp bytes back), b = up, c = up-left; absent neighbours are 0.
// Paeth's ties go a, b, c (png_core.h's paeth, the spec's order).  f <= 4.
DVD_HD uint8_t unfilter_byte(int f, int x, int a, int b, int c) {
  const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : png::paeth(a, b, c);
  return (uint8_t)(x + pred);
}
// a row starts a band if it does not read the row above
DVD_HD bool starts_band(long row, int f) { return row == 0 || f <= 1; }

}  // namespace pngdec
}  // namespace dvd
