// PNG decoder for input photographs and ground-truth scans (DESIGN.md section 4.9 holds the definition; pngdec_core.h its
// arithmetic, shared with the CPU restatement pngdec_host_check.cpp).  The file goes to the device; the host parses the chunk
// layout only, and walks the small candidate table between the count and the write pass.
//   pngdec_gather_kernel    the IDAT payload, gathered from the (offset, length) table, zero padded
//   pngdec_crc_kernel       one workgroup per IDAT chunk: its CRC-32 with png_core.h's folding pieces
//   pngdec_find_kernel      one lane per BIT position: does a dynamic block that zlib accepts start here?  one ballot per wave
//   pngdec_candscan_kernel  exclusive scan of the flags per 256 positions (block_ops.h's chunked_scan_256), the total
//   pngdec_scatter_kernel   the flagged positions into the candidate table: sorted, no atomics
//   pngdec_count_kernel     one lane per candidate: decode to the next dynamic block -> (end, bytes, flags)
//   pngdec_write_kernel     one lane per segment on the chain: decode again -> val[i] / src[i]
//   pngdec_double_kernel    src[i] = src[src[i]] in place
//   pngdec_resolve_kernel   inflated[i] = val[src[i]] in place, Adler-32 partials
//   pngdec_bands_kernel     Adler-32 folded and compared, filter bytes checked, the band table (flags + scan)
//   pngdec_unfilter_kernel  one wave per band, strips of 64 / bpp rows, row r one pixel behind row r - 1
//   pngdec_final_kernel     colour types 0 and 6 -> RGB
// The decode tables live in LDS; no kernel uses scratch memory, spins on another workgroup or loops without a bound.
#include "common.h"
#include "block_ops.h"
#include "pngdec_core.h"

namespace dvd {
namespace pngdec {

__global__ void __launch_bounds__(256) pngdec_gather_kernel(const uint8_t* __restrict__ file, const Idat* __restrict__ idat, long nidat,
                                                            uint8_t* __restrict__ payload, long plen, long padded,
                                                            uint32_t* __restrict__ ctr) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < 64) ctr[i] = 0;
  if (i >= padded) return;
  uint8_t v = 0;
  if (i < plen) {
    long lo = 0, hi = nidat - 1;                 // the last chunk with pre <= i: empty chunks in front of it share its pre
    while (lo < hi) {
      const long mid = (lo + hi + 1) / 2;
      if ((long)idat[mid].pre <= i) lo = mid;
      else hi = mid - 1;
    }
    v = file[idat[lo].off + (unsigned long long)(i - (long)idat[lo].pre)];
  }
  payload[i] = v;
}

// Thread t takes the register state of sub-range t of (type, data) from state 0; the sub-ranges have one length c and are
// right-aligned (leading zero bytes leave a zero state zero), a tree with the factors x^(8 c 2^k) joins them and the initial
// state is carried across the whole by x^(8 N) - png.hip's png_gather_kernel, read instead of written.
__global__ void __launch_bounds__(256) pngdec_crc_kernel(const uint8_t* __restrict__ file, const Idat* __restrict__ idat,
                                                         uint32_t* __restrict__ ctr) {
  __shared__ uint32_t part[256];
  const int tid = threadIdx.x;
  const Idat ch = idat[blockIdx.x];
  const uint8_t* src = file + ch.off - 4;        // the chunk's type, then its data
  const long N = (long)ch.len + 4;
  const long c = (N + 255) / 256, shift = 256 * c - N;
  uint32_t r = 0;
  for (long j = 0; j < c; ++j) {
    const long i = tid * c + j - shift;
    if (i >= 0) r = png::crc_byte(r, src[i]);
  }
  part[tid] = r;
  __syncthreads();
  uint32_t f = png::crc_xpow8((unsigned long long)c);
  for (int d = 1; d < 256; d <<= 1) {
    if ((tid & (2 * d - 1)) == 0) part[tid] = png::crc_mul(part[tid], f) ^ part[tid + d];
    f = png::crc_mul(f, f);
    __syncthreads();
  }
  if (tid == 0) {
    const uint32_t crc = ~(png::crc_mul(0xFFFFFFFFu, png::crc_xpow8((unsigned long long)N)) ^ part[0]);
    const uint8_t* p = src + N;
    const uint32_t want = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    if (crc != want) atomicOr(ctr + kCtrStatus, kStCrc);
  }
}

// Lane g looks at bit position 16 + g.  Position 16, behind the zlib header, is segment 0 whatever stands there.
__global__ void __launch_bounds__(256) pngdec_find_kernel(Bits B, long nbits, unsigned long long* __restrict__ masks) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long endbits = 16ull + (unsigned long long)nbits;
  const bool hit = g < nbits && (g == 0 || is_candidate(B, 16ull + (unsigned long long)g, endbits));
  const unsigned long long m = __ballot(hit);
  if ((threadIdx.x & 63) == 0) masks[g >> 6] = m;
}

// One workgroup: prefix[c] = candidates in front of chunk c (4 masks = 256 positions); ctr[kCtrCand] = their total, saturated.
__global__ void __launch_bounds__(256) pngdec_candscan_kernel(const unsigned long long* __restrict__ masks, long nchunks,
                                                              uint32_t* __restrict__ prefix, uint32_t* __restrict__ ctr) {
  __shared__ unsigned long long part[256];
  const unsigned long long total = chunked_scan_256(
      part, nchunks, 0ull,
      [&](long c) { return (unsigned long long)(__popcll(masks[4 * c]) + __popcll(masks[4 * c + 1]) + __popcll(masks[4 * c + 2]) + __popcll(masks[4 * c + 3])); },
      [](unsigned long long a, unsigned long long b) { return a + b; },
      [&](long c, unsigned long long pre) { prefix[c] = (uint32_t)(pre > 0xFFFFFFFFull ? 0xFFFFFFFFull : pre); });
  if (threadIdx.x == 0) ctr[kCtrCand] = (uint32_t)(total > 0xFFFFFFFFull ? 0xFFFFFFFFull : total);
}

__global__ void __launch_bounds__(256) pngdec_scatter_kernel(const unsigned long long* __restrict__ masks, const uint32_t* __restrict__ prefix,
                                                             long nbits, Seg* __restrict__ cand, long ncap) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const long c = blockIdx.x;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long before = prefix[c];
  for (int k = 0; k < wv; ++k) before += (unsigned)__popcll(masks[4 * c + k]);
  const unsigned long long m = masks[4 * c + wv];
  if (g >= nbits || !((m >> lane) & 1ull)) return;
  const unsigned long long row = before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
  if (row < (unsigned long long)ncap) cand[row] = Seg{(uint32_t)(16 + g), 0u, 0u, kSegBad};
}

__device__ __forceinline__ Tab<kLanes> lane_tab(uint16_t* hw, uint8_t* by) { return Tab<kLanes>{hw, by, (int)threadIdx.x}; }

__global__ void __launch_bounds__(kLanes) pngdec_count_kernel(Bits B, long nbits, Seg* __restrict__ cand, long ncand,
                                                              unsigned long long max_work) {
  __shared__ uint16_t hw[kTabHalves * kLanes];
  __shared__ uint8_t by[kTabBytes * kLanes];
  const long k = (long)blockIdx.x * kLanes + threadIdx.x;
  if (k >= ncand) return;
  Tab<kLanes> t = lane_tab(hw, by);
  CountSink sink{0};
  const WalkResult r = walk(B, 16ull + (unsigned long long)nbits, cand[k].pos, t, max_work, sink);
  cand[k].end = (uint32_t)r.end;
  cand[k].nbytes = (uint32_t)(sink.n > 0xFFFFFFFFull ? 0xFFFFFFFFull : sink.n);
  cand[k].flags = r.flags;
}

__global__ void __launch_bounds__(kLanes) pngdec_write_kernel(Bits B, long nbits, const Reach* __restrict__ reach, long nreach,
                                                              uint8_t* __restrict__ val, uint32_t* __restrict__ src,
                                                              unsigned long long max_work, uint32_t* __restrict__ ctr) {
  __shared__ uint16_t hw[kTabHalves * kLanes];
  __shared__ uint8_t by[kTabBytes * kLanes];
  const long k = (long)blockIdx.x * kLanes + threadIdx.x;
  if (k >= nreach) return;
  Tab<kLanes> t = lane_tab(hw, by);
  const Reach r = reach[k];
  // the sink stores inside [out_off, out_off + nbytes) only, whatever the walk does
  WriteSink sink{val, src, r.out_off, (unsigned long long)r.out_off + r.nbytes, 0u};
  walk(B, 16ull + (unsigned long long)nbits, r.pos, t, max_work, sink);
  if (sink.bad) atomicOr(ctr + kCtrStatus, sink.bad);
}

// Lane i reads src[s] while the lane that owns s may be writing it: either value is an ancestor of i on the chain of
// copies (src only ever moves towards the chain's root, and a 32-bit store is whole), so the race costs at most a round.
// The fixpoint - every src at its root - is what remains when a round changes nothing.  ctr[kCtrStamp] = 1 + the last
// round that changed an entry.
__global__ void __launch_bounds__(256) pngdec_double_kernel(uint32_t* src, long n, uint32_t* ctr, int round) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (i < n) {
    uint32_t s = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s > (uint32_t)i) s = (uint32_t)i;            // never: the write pass stores src[i] <= i; no read outside the table
    const uint32_t t = __hip_atomic_load(src + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != s) {
      __hip_atomic_store(src + i, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      changed = true;
    }
  }
  if (__ballot(changed) && (threadIdx.x & 63) == 0) atomicMax(ctr + kCtrStamp, (uint32_t)round + 1u);
}

// One workgroup per kAdlerBlock bytes.  In place: a root's own byte stays (src[i] = i), and after the fixpoint only roots
// are read.  part[b] = the block's (sum d_k, sum (n - k) d_k) mod 65521.
__global__ void __launch_bounds__(256) pngdec_resolve_kernel(uint8_t* val, const uint32_t* __restrict__ src, long n,
                                                             uint2* __restrict__ part) {
  __shared__ unsigned long long sa[4], sb[4];
  const long base = (long)blockIdx.x * kAdlerBlock;
  const long len = n - base < kAdlerBlock ? n - base : kAdlerBlock;
  unsigned long long a = 0, b = 0;
  for (long k = threadIdx.x; k < len; k += 256) {
    uint32_t s = src[base + k];
    if (s > (uint32_t)(base + k)) s = (uint32_t)(base + k);   // never (see pngdec_double_kernel)
    const uint8_t d = val[s];
    if (s != (uint32_t)(base + k)) val[base + k] = d;
    a += d;
    b += (unsigned long long)(len - k) * d;
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sa[threadIdx.x >> 6] = a;
    sb[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    part[blockIdx.x] = make_uint2((uint32_t)((sa[0] + sa[1] + sa[2] + sa[3]) % png::kAdlerMod), (uint32_t)((sb[0] + sb[1] + sb[2] + sb[3]) % png::kAdlerMod));
}

// One workgroup: the Adler-32 folded in block order and compared with the four bytes behind the stream; every filter byte
// checked; band[k] = first row of band k (rows that do not read the row above: flags, scan, scatter), ctr[kCtrBands] = bands.
__global__ void __launch_bounds__(256) pngdec_bands_kernel(Plan P, const uint8_t* __restrict__ infl, const uint2* __restrict__ part,
                                                           long nparts, const uint8_t* __restrict__ adler_at, uint32_t* __restrict__ band,
                                                           uint32_t* __restrict__ ctr) {
  __shared__ uint32_t lds[256];
  if (threadIdx.x == 0) {
    uint32_t A = 1, Bv = 0;
    for (long k = 0; k < nparts; ++k) {
      const long left = P.inflated - k * kAdlerBlock;
      png::adler_fold(A, Bv, (uint32_t)(left < kAdlerBlock ? left : kAdlerBlock), part[k].x, part[k].y);
    }
    const uint32_t got = (Bv << 16) | A;
    const uint32_t want = ((uint32_t)adler_at[0] << 24) | ((uint32_t)adler_at[1] << 16) | ((uint32_t)adler_at[2] << 8) | adler_at[3];
    ctr[kCtrAdler] = got;
    if (got != want) atomicOr(ctr + kCtrStatus, kStAdler);
  }
  bool bad = false;
  for (long r = threadIdx.x; r < P.h; r += 256) bad |= infl[r * P.stride] > 4;
  if (bad) atomicOr(ctr + kCtrStatus, kStFilter);
  const uint32_t total = chunked_scan_256(
      lds, (long)P.h, 0u, [&](long r) { return starts_band(r, infl[r * P.stride]) ? 1u : 0u; },
      [](uint32_t a, uint32_t b) { return a + b; },
      [&](long r, uint32_t pre) {
        if (starts_band(r, infl[r * P.stride])) band[pre] = (uint32_t)r;
      });
  if (threadIdx.x == 0) ctr[kCtrBands] = total;
}

// One wave per band; the grid is h workgroups, the surplus returns.  Lane = (row j of the strip, channel c).  At step t lane
// (j, c) rebuilds pixel x = t - j of its row: a is its own last value, b and c are the last and the last but one value of
// lane (j - 1, c), which is one pixel ahead - two cross-lane moves.  Row 0 of a strip reads the row above from dst, where
// this wave left it one strip earlier (behind a fence, with loads that go to memory).  DIRECT: dst is the [h,w,3] output
// (colour type 2); otherwise the rows are rebuilt in place, behind their filter bytes.
template <int BPP, bool DIRECT>
__global__ void __launch_bounds__(64) pngdec_unfilter_kernel(Plan P, uint8_t* infl, const uint32_t* __restrict__ band,
                                                             const uint32_t* __restrict__ ctr, uint8_t* out) {
  constexpr int R = 64 / BPP;
  const uint32_t nbands = ctr[kCtrBands];
  if (blockIdx.x >= nbands) return;
  const long r0 = band[blockIdx.x], r1 = blockIdx.x + 1 < nbands ? (long)band[blockIdx.x + 1] : (long)P.h;
  const int lane = threadIdx.x, j = lane / BPP, c = lane % BPP;
  const long w = P.w, pitch = DIRECT ? w * BPP : P.stride;
  uint8_t* dst = DIRECT ? out : infl + 1;
  for (long rs = r0; rs < r1; rs += R) {
    const long rows = r1 - rs < R ? r1 - rs : R;
    const long row = rs + j;
    const bool live = j < rows;
    const int ft = live ? infl[row * P.stride] : 0;
    const uint8_t* in = infl + row * P.stride + 1 + c;
    uint8_t* o = dst + row * pitch + c;
    const uint8_t* up = dst + (rs - 1) * pitch + c;   // read only if rs > r0
    const bool has_up = rs > r0;
    int last = 0, last2 = 0, upprev = 0;
    const long steps = w + rows - 1;
    for (long t = 0; t < steps; ++t) {
      const long x = t - j;
      int b = __shfl(last, (lane - BPP) & 63, 64), cc = __shfl(last2, (lane - BPP) & 63, 64);
      const bool on = live && x >= 0 && x < w;
      if (j == 0) {
        b = (on && has_up) ? (int)__hip_atomic_load(up + x * BPP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        cc = upprev;
        upprev = b;
      }
      if (on) {
        const int v = unfilter_byte(ft, in[x * BPP], last, b, cc);
        o[x * BPP] = (uint8_t)v;
        last2 = last;
        last = v;
      }
    }
    __threadfence();
  }
}

// colour type 0: gray replicated; 6: alpha dropped.  One lane per pixel.
__global__ void __launch_bounds__(256) pngdec_final_kernel(Plan P, const uint8_t* __restrict__ infl, uint8_t* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)P.h * P.w) return;
  const long y = idx / P.w, x = idx % P.w;
  const uint8_t* p = infl + y * P.stride + 1 + x * P.bpp;
  uint8_t* d = out + idx * 3;
  d[0] = p[0];
  d[1] = P.bpp == 1 ? p[0] : p[1];
  d[2] = P.bpp == 1 ? p[0] : p[2];
}

static int parse_or_refuse(const char* what, const uint8_t* file_host, long n, Plan* P, std::vector<Idat>* idat) {
  const char* why = "";
  const int rc = parse(file_host, n, P, idat, &why);
  if (rc) set_error("%s: refused: %s", what, why);
  return rc;
}

}  // namespace pngdec
}  // namespace dvd

using namespace dvd;

extern "C" int dvd_pngdec_probe(const uint8_t* file_host, long n, dvd_pngdec_info* info) {
  DVD_REQUIRE(file_host && info, "pngdec_probe: null pointer");
  DVD_REQUIRE(n >= 1, "pngdec_probe: bad length %ld", n);
  pngdec::Plan P;
  std::vector<pngdec::Idat> idat;
  const int rc = pngdec::parse_or_refuse("pngdec_probe", file_host, n, &P, &idat);
  if (rc) return rc;
  info->h = P.h;
  info->w = P.w;
  info->colour_type = P.ctype;
  info->bpp = P.bpp;
  info->idat_chunks = P.nidat;
  info->payload_bytes = P.payload;
  info->scratch_bytes = (long)pngdec::layout_of(P).total;
  return DVD_OK;
}

extern "C" int dvd_png_decode_rgb8(const uint8_t* file_host, const uint8_t* file_dev, long n, uint8_t* out_hwc, long cap,
                                   long max_work, dvd_pngdec_stats* stats_out, void* scratch, void* stream) {
  using namespace pngdec;
  DVD_REQUIRE(file_host && file_dev && out_hwc && scratch, "png_decode_rgb8: null pointer");
  DVD_REQUIRE(n >= 1, "png_decode_rgb8: bad length %ld", n);
  DVD_REQUIRE(max_work >= 0, "png_decode_rgb8: max_work %ld is negative (0 = the default, %ld)", max_work, kDefaultMaxWork);
  DVD_REQUIRE(((uintptr_t)scratch & 15) == 0, "png_decode_rgb8: scratch must be 16-byte aligned");
  Plan P;
  std::vector<Idat> idat;
  const int rc = parse_or_refuse("png_decode_rgb8", file_host, n, &P, &idat);
  if (rc) return rc;
  DVD_REQUIRE(cap >= 3L * P.h * P.w, "png_decode_rgb8: cap %ld below 3 h w = %ld", cap, 3L * P.h * P.w);
  if (stats_out) *stats_out = dvd_pngdec_stats{0, 0, 0, 0};
  if (P.payload < kMinPayload) {
    set_error("png_decode_rgb8: %ld bytes of IDAT data cannot hold a stream", P.payload);
    return DVD_E_PNG_DATA;
  }
  if (max_work == 0) max_work = kDefaultMaxWork;
  if (max_work > (1L << 23)) max_work = 1L << 23;   // a lane's byte count stays inside 32 bits
  hipStream_t st = (hipStream_t)stream;
  const Layout l = layout_of(P);
  uint8_t* base = (uint8_t*)scratch;
  Idat* d_idat = (Idat*)(base + l.idat);
  uint8_t* payload = base + l.payload;
  unsigned long long* masks = (unsigned long long*)(base + l.masks);
  uint32_t* prefix = (uint32_t*)(base + l.prefix);
  uint32_t* ctr = (uint32_t*)(base + l.ctr);
  Seg* cand = (Seg*)(base + l.cand);
  Reach* d_reach = (Reach*)(base + l.reach);
  uint8_t* val = base + l.val;
  uint32_t* src = (uint32_t*)(base + l.src);
  uint2* part = (uint2*)(base + l.adler);
  uint32_t* band = (uint32_t*)(base + l.band);
  auto fail = [&](const char* what) {
    set_error("png_decode_rgb8: %s: %s", what, hipGetErrorString(hipGetLastError()));
    return DVD_E_LAUNCH;
  };
  auto read_back = [&](const void* from, void* to, size_t bytes) {
    return hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  };
  if (hipMemcpyAsync(d_idat, idat.data(), idat.size() * sizeof(Idat), hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload");
  const long padded = l.nwords * 4;
  pngdec_gather_kernel<<<(unsigned)cdiv(padded, 256), 256, 0, st>>>(file_dev, d_idat, P.nidat, payload, P.payload, padded, ctr);
  pngdec_crc_kernel<<<(unsigned)P.nidat, 256, 0, st>>>(file_dev, d_idat, ctr);
  const Bits B{(const uint32_t*)payload, l.nwords};
  pngdec_find_kernel<<<(unsigned)l.nchunks, 256, 0, st>>>(B, P.nbits, masks);
  pngdec_candscan_kernel<<<1, 256, 0, st>>>(masks, l.nchunks, prefix, ctr);
  pngdec_scatter_kernel<<<(unsigned)l.nchunks, 256, 0, st>>>(masks, prefix, P.nbits, cand, P.ncap);
  uint32_t ncand = 0;
  if (!read_back(ctr + kCtrCand, &ncand, 4)) return fail("read-back");
  if (stats_out) stats_out->candidates = (int)(ncand > 0x7FFFFFFFu ? 0x7FFFFFFFu : ncand);
  if ((long)ncand > P.ncap) {
    set_error("png_decode_rgb8: %u candidate block starts, the table holds %ld", ncand, P.ncap);
    return DVD_E_PNG_NOSPLIT;
  }
  pngdec_count_kernel<<<(unsigned)cdiv((long)ncand, kLanes), kLanes, 0, st>>>(B, P.nbits, cand, (long)ncand, (unsigned long long)max_work);
  std::vector<Seg> rows(ncand);
  if (!read_back(cand, rows.data(), rows.size() * sizeof(Seg))) return fail("read-back");
  std::vector<Reach> reach;
  long adler_at = 0;
  const char* why = "";
  const int crc = chain(rows.data(), (long)ncand, P, &reach, &adler_at, &why);
  if (stats_out) stats_out->segments = (int)reach.size();
  if (crc) {
    set_error("png_decode_rgb8: %s", why);
    return crc;
  }
  const long nreach = (long)reach.size();
  if (hipMemcpyAsync(d_reach, reach.data(), reach.size() * sizeof(Reach), hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload");
  pngdec_write_kernel<<<(unsigned)cdiv(nreach, kLanes), kLanes, 0, st>>>(B, P.nbits, d_reach, nreach, val, src, (unsigned long long)max_work, ctr);
  // pointer doubling: a chain of n copies is at its roots after ceil(log2 n) rounds, one more sees no change; the race can
  // cost rounds only where it saved some before, and the cap below is generous
  int max_rounds = 3;
  while ((1L << (max_rounds - 3)) < P.inflated) ++max_rounds;
  max_rounds *= 2;
  const unsigned dgrid = (unsigned)cdiv(P.inflated, 256);
  int it = 0;
  bool fixed = false;
  while (it < max_rounds && !fixed) {
    for (int k = 0; k < kGroup; ++k, ++it) pngdec_double_kernel<<<dgrid, 256, 0, st>>>(src, P.inflated, ctr, it);
    uint32_t stamp = 0;
    if (!read_back(ctr + kCtrStamp, &stamp, 4)) return fail("read-back");
    if ((int)stamp < it) {                         // the group's last round changed nothing: the fixpoint
      fixed = true;
      it = (int)stamp + 1;
    }
  }
  if (stats_out) stats_out->rounds = it;
  if (!fixed) {
    set_error("png_decode_rgb8: the copies did not resolve within %d rounds", max_rounds);
    return DVD_E_PNG_DATA;
  }
  pngdec_resolve_kernel<<<(unsigned)l.nparts, 256, 0, st>>>(val, src, P.inflated, part);
  pngdec_bands_kernel<<<1, 256, 0, st>>>(P, val, part, l.nparts, payload + adler_at, band, ctr);
  uint32_t tail[2] = {0, 0};                       // status, bands
  if (!read_back(ctr + kCtrStatus, tail, 8)) return fail("read-back");
  if (stats_out) stats_out->bands = (int)tail[1];
  if (tail[0]) {
    set_error("png_decode_rgb8: damaged data:%s%s%s%s%s", tail[0] & kStCrc ? " IDAT CRC-32 mismatch;" : "",
              tail[0] & kStDistance ? " a distance reaching before the start of the stream;" : "",
              tail[0] & kStAdler ? " Adler-32 mismatch;" : "", tail[0] & kStFilter ? " a filter byte above 4;" : "",
              tail[0] & kStOverflow ? " a segment longer than counted;" : "");
    return DVD_E_PNG_DATA;
  }
  const unsigned ugrid = (unsigned)P.h;
  if (P.bpp == 3) {
    pngdec_unfilter_kernel<3, true><<<ugrid, 64, 0, st>>>(P, val, band, ctr, out_hwc);
  } else {
    if (P.bpp == 1) pngdec_unfilter_kernel<1, false><<<ugrid, 64, 0, st>>>(P, val, band, ctr, nullptr);
    else pngdec_unfilter_kernel<4, false><<<ugrid, 64, 0, st>>>(P, val, band, ctr, nullptr);
    pngdec_final_kernel<<<(unsigned)cdiv((long)P.h * P.w, 256), 256, 0, st>>>(P, val, out_hwc);
  }
  return check_launch("png_decode_rgb8");
}
