// Stand-alone CPU restatement of the PNG decoder of pngdec.hip on the shared arithmetic of pngdec_core.h: the same chunk
// parser, the gathered payload, the block finder over every bit position, the count pass, the chain, the write pass into
// val / src, pointer doubling (every lane of a round reads the table of the round before), the resolve, both checksums, the
// band table and the unfilter, with the lanes as plain loops and every buffer of exactly the size the layout gives it.
// Plain C++ (no HIP), so it can be built with -fsanitize=address,undefined:
//     g++ -O1 -g -fsanitize=address,undefined pngdec_host_check.cpp -o pngdec_host_check
//     pngdec_host_check in.png out.rgb [max_work]
// prints "status candidates segments rounds bands h w" and writes out.rgb (h * w * 3 bytes) when status is 0.  Its exit
// status is 0 whenever it could print that line - a refusal, DATA or NOSPLIT is a normal outcome - and 2 for a bad command
// line.  It is not part of libdvd_hip.so; tests/test_pngdec_cpu.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host_check_io.hpp"
#include "pngdec_core.h"

using namespace dvd::pngdec;
namespace png = dvd::png;

static int finish(int status, long cand, long segs, int rounds, long bands, int h, int w) {
  printf("%d %ld %ld %d %ld %d %d\n", status, cand, segs, rounds, bands, h, w);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    fprintf(stderr, "usage: %s in.png out.rgb [max_work]\n", argv[0]);
    return 2;
  }
  const long max_work = argc == 4 ? atol(argv[3]) : kDefaultMaxWork;
  std::vector<uint8_t> file;
  if (max_work < 1 || !read_all(argv[1], file) || file.empty()) return 2;
  const long n = (long)file.size();

  Plan P;
  std::vector<Idat> idat;
  const char* why = "";
  const int rc = parse(file.data(), n, &P, &idat, &why);
  if (rc) {
    fprintf(stderr, "refused: %s\n", why);
    return finish(rc, 0, 0, 0, 0, 0, 0);
  }
  if (P.payload < kMinPayload) return finish(DVD_E_PNG_DATA, 0, 0, 0, 0, P.h, P.w);
  const Layout l = layout_of(P);

  // gather, and every IDAT's CRC-32 (type and data), folded as the kernel folds it
  std::vector<uint32_t> words((size_t)l.nwords, 0u);
  uint32_t status = 0;
  {
    std::vector<uint8_t> bytes((size_t)l.nwords * 4, 0);
    for (const Idat& c : idat) {
      memcpy(bytes.data() + c.pre, file.data() + c.off, c.len);
      const long N = (long)c.len + 4;
      const uint32_t body = png::crc_bytes(0u, file.data() + c.off - 4, N);
      const uint32_t crc = ~(png::crc_mul(0xFFFFFFFFu, png::crc_xpow8((unsigned long long)N)) ^ body);
      if (crc != be32(file.data() + c.off + c.len)) status |= kStCrc;
    }
    memcpy(words.data(), bytes.data(), bytes.size());     // little-endian hosts only, as the device is
  }
  const Bits B{words.data(), l.nwords};
  const unsigned long long endbits = 16ull + (unsigned long long)P.nbits;

  // the block finder, flags to a sorted table
  std::vector<Seg> cand;
  for (long g = 0; g < P.nbits; ++g)
    if (g == 0 || is_candidate(B, 16ull + (unsigned long long)g, endbits)) {
      if ((long)cand.size() < P.ncap) cand.push_back(Seg{(uint32_t)(16 + g), 0u, 0u, kSegBad});
      else return finish(DVD_E_PNG_NOSPLIT, P.ncap + 1, 0, 0, 0, P.h, P.w);
    }
  const long ncand = (long)cand.size();

  // count
  std::vector<uint16_t> hw(kTabHalves);
  std::vector<uint8_t> by(kTabBytes);
  Tab<1> t{hw.data(), by.data(), 0};
  for (Seg& s : cand) {
    CountSink sink{0};
    const WalkResult r = walk(B, endbits, s.pos, t, (unsigned long long)max_work, sink);
    s.end = (uint32_t)r.end;
    s.nbytes = (uint32_t)(sink.n > 0xFFFFFFFFull ? 0xFFFFFFFFull : sink.n);
    s.flags = r.flags;
  }
  std::vector<Reach> reach;
  long adler_at = 0;
  const int crc = chain(cand.data(), ncand, P, &reach, &adler_at, &why);
  if (crc) {
    fprintf(stderr, "%s\n", why);
    return finish(crc, ncand, (long)reach.size(), 0, 0, P.h, P.w);
  }

  // write
  std::vector<uint8_t> val((size_t)P.inflated, 0);
  std::vector<uint32_t> src((size_t)P.inflated, 0);
  for (const Reach& r : reach) {
    WriteSink sink{val.data(), src.data(), r.out_off, (unsigned long long)r.out_off + r.nbytes, 0u};
    walk(B, endbits, r.pos, t, (unsigned long long)max_work, sink);
    status |= sink.bad;
  }

  // pointer doubling, synchronous rounds
  int rounds = 0;
  for (bool changed = true; changed;) {
    changed = false;
    std::vector<uint32_t> next(src);
    for (long i = 0; i < P.inflated; ++i) {
      const uint32_t s = src[(size_t)i], tt = src.at(s);
      if (tt != s) {
        next[(size_t)i] = tt;
        changed = true;
      }
    }
    src.swap(next);
    ++rounds;
  }

  // resolve in place, Adler-32 per block and folded
  uint32_t A = 1, Bv = 0;
  for (long p = 0; p < l.nparts; ++p) {
    const long base = p * kAdlerBlock, len = P.inflated - base < kAdlerBlock ? P.inflated - base : kAdlerBlock;
    unsigned long long a = 0, b = 0;
    for (long k = 0; k < len; ++k) {
      const uint8_t d = val.at(src[(size_t)(base + k)]);
      val[(size_t)(base + k)] = d;
      a += d;
      b += (unsigned long long)(len - k) * d;
    }
    png::adler_fold(A, Bv, (uint32_t)len, (uint32_t)(a % png::kAdlerMod), (uint32_t)(b % png::kAdlerMod));
  }
  uint8_t ad[4];
  for (int k = 0; k < 4; ++k) ad[k] = (uint8_t)B.byte((unsigned long long)(adler_at + k));
  if (((Bv << 16) | A) != be32(ad)) status |= kStAdler;

  // bands
  std::vector<uint32_t> band;
  for (long r = 0; r < P.h; ++r) {
    const int f = val[(size_t)(r * P.stride)];
    if (f > 4) status |= kStFilter;
    if (starts_band(r, f)) band.push_back((uint32_t)r);
  }
  const long nbands = (long)band.size();
  if (status) return finish(DVD_E_PNG_DATA, ncand, (long)reach.size(), rounds, nbands, P.h, P.w);

  // unfilter band by band, rows in place behind their filter bytes; a band's first row never reads the row above it
  for (long k = 0; k < nbands; ++k) {
    const long r0 = band[(size_t)k], r1 = k + 1 < nbands ? (long)band[(size_t)k + 1] : (long)P.h;
    for (long r = r0; r < r1; ++r) {
      uint8_t* row = val.data() + r * P.stride + 1;
      const uint8_t* up = r > r0 ? row - P.stride : nullptr;
      const int f = row[-1];
      for (long x = 0; x < (long)P.w * P.bpp; ++x) {
        const int a = x >= P.bpp ? row[x - P.bpp] : 0, b = up ? up[x] : 0, c = up && x >= P.bpp ? up[x - P.bpp] : 0;
        row[x] = unfilter_byte(f, row[x], a, b, c);
      }
    }
  }
  std::vector<uint8_t> rgb((size_t)P.h * P.w * 3);
  for (long y = 0; y < P.h; ++y)
    for (long x = 0; x < P.w; ++x) {
      const uint8_t* p = val.data() + y * P.stride + 1 + x * P.bpp;
      uint8_t* d = &rgb.at((size_t)(y * P.w + x) * 3);
      d[0] = p[0];
      d[1] = P.bpp == 1 ? p[0] : p[1];
      d[2] = P.bpp == 1 ? p[0] : p[2];
    }
  if (!write_all(argv[2], rgb.data(), rgb.size())) return 2;
  return finish(0, ncand, (long)reach.size(), rounds, nbands, P.h, P.w);
}
