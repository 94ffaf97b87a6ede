// Baseline JPEG decoder for the input photograph (DESIGN.md section 4.6 holds the definition; jpegdec_core.h its arithmetic,
// shared with the CPU restatement jpegdec_host_check.cpp).  The file goes to the device; the host parses the header only.
// Baseline Huffman data has no index, so the entropy decoder synchronises itself: the scan is cut into subsequences of kSubseq
// bytes, one lane each; E[j] = the decoder state (bit position, block slot, zig-zag index) at the start of subsequence j is
// iterated to its unique fixpoint from the guesses (j kSubseq 8, 0, 0).
//   jpegdec_init_kernel    the guesses, every lane marked changed
//   jpegdec_sync_kernel    one iteration: E[j + 1] = walk(E[j]) for every j whose E[j] changed in the iteration before
//   jpegdec_count_kernel   blocks completed per subsequence; jpegdec_scan_kernel their exclusive scan and total (block_ops.h's
//                          chunked_scan_256, as is jpegdec_dc_kernel<1> with dc_join for +)
//   jpegdec_write_kernel   decodes again into the zeroed int16 [blocks][64] buffer (zig-zag order, DC differences)
//   jpegdec_dc_kernel<0..2>  segmented prefix sum of the DC differences per component, restarted behind RSTn
//   jpegdec_idct_kernel    dequantisation and libjpeg's integer IDCT, eight lanes per block -> u8 planes
//   jpegdec_final_kernel   chroma upsampling, colour, EXIF orientation -> HWC bytes
// The Huffman tables live in LDS; no kernel uses scratch memory, spins on another workgroup or loops without a bound.
#include "common.h"
#include "block_ops.h"
#include "jpegdec_core.h"

namespace dvd {
namespace jpegdec {

struct Izz { uint8_t p[64]; };
constexpr Izz make_izz() {
  Izz z{};
  for (int k = 0; k < 64; ++k) z.p[kZigzag[k]] = (uint8_t)k;
  return z;
}
__device__ const Izz kIzzDev = make_izz();       // natural index -> position in the zig-zag sequence

__device__ __forceinline__ const HuffDec* load_tables(uint32_t* lds, const Plan& P) {
  for (int i = threadIdx.x; i < 4 * kHuffWords; i += 256) lds[i] = P.huff[i];
  __syncthreads();
  return (const HuffDec*)lds;
}
__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long stop_of(long j) { return (j + 1) * (long)kSubseq * 8; }

__global__ void __launch_bounds__(256) jpegdec_init_kernel(unsigned long long* __restrict__ E, uint8_t* __restrict__ chg0,
                                                           uint8_t* __restrict__ chg1, uint32_t* __restrict__ ctr, long nsub) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j > nsub) return;
  E[j] = guess_state(j);
  chg0[j] = j < nsub;
  chg1[j] = 0;
  if (j < 4) ctr[j] = 0;
}

// Lane j reads E[j] while lane j - 1 may be writing it: either value is a complete 64-bit state, and a lane whose input
// changed in this iteration is marked and runs again in the next, so the fixpoint - which is unique - is what remains when
// nothing is marked.  ctr[0] = 1 + the last iteration that changed a state.
__global__ void __launch_bounds__(256) jpegdec_sync_kernel(Plan P, const uint8_t* __restrict__ scan, unsigned long long* E,
                                                           uint8_t* chg_in, uint8_t* chg_out, uint32_t* ctr, int iter) {
  __shared__ uint32_t lds[4 * kHuffWords];
  const HuffDec* tabs = load_tables(lds, P);
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= P.nsub || !chg_in[j]) return;
  chg_in[j] = 0;
  NullSink sink;
  const unsigned long long in = __hip_atomic_load(E + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long s = walk(tabs, P.dc_mask, P.ac_mask, P.bpm, scan, P.scan_len, in, stop_of(j), sink);
  if (j + 1 < P.nsub && s != __hip_atomic_load(E + j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
    __hip_atomic_store(E + j + 1, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    chg_out[j + 1] = 1;
    atomicMax(ctr, (uint32_t)iter + 1u);
  }
}

__global__ void __launch_bounds__(256) jpegdec_count_kernel(Plan P, const uint8_t* __restrict__ scan,
                                                            const unsigned long long* __restrict__ E, uint32_t* __restrict__ counts) {
  __shared__ uint32_t lds[4 * kHuffWords];
  const HuffDec* tabs = load_tables(lds, P);
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= P.nsub) return;
  CountSink sink{0};
  walk(tabs, P.dc_mask, P.ac_mask, P.bpm, scan, P.scan_len, E[j], stop_of(j), sink);
  counts[j] = sink.n;
}

// One workgroup: first[j] = blocks completed in front of subsequence j; ctr[1] = their total, saturated.
__global__ void __launch_bounds__(256) jpegdec_scan_kernel(const uint32_t* __restrict__ counts, long nsub, uint32_t* __restrict__ first,
                                                           uint32_t* __restrict__ ctr) {
  __shared__ unsigned long long part[256];
  const auto saturated = [](unsigned long long v) { return (uint32_t)(v > 0xFFFFFFFFull ? 0xFFFFFFFFull : v); };
  const unsigned long long total = chunked_scan_256(
      part, nsub, 0ull, [&](long i) { return (unsigned long long)counts[i]; },
      [](unsigned long long a, unsigned long long b) { return a + b; },
      [&](long i, unsigned long long pre) { first[i] = saturated(pre); });
  if (threadIdx.x == 0) ctr[1] = saturated(total);
}

__global__ void __launch_bounds__(256) jpegdec_write_kernel(Plan P, const uint8_t* __restrict__ scan,
                                                            const unsigned long long* __restrict__ E, const uint32_t* __restrict__ first,
                                                            int16_t* __restrict__ coef, uint8_t* __restrict__ flags) {
  __shared__ uint32_t lds[4 * kHuffWords];
  const HuffDec* tabs = load_tables(lds, P);
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= P.nsub) return;
  WriteSink sink{coef, flags, P.nblocks, (long)first[j], P.bpm};
  walk(tabs, P.dc_mask, P.ac_mask, P.bpm, scan, P.scan_len, E[j], stop_of(j), sink);
}

// ---------------------------------------------------------------- DC prefix sum ---------------------------------------------
// Per component over stream order, restarted at every flagged MCU.  A lane owns kDcChunk consecutive MCUs.
//   PHASE 0  agg[chunk] = (a flag was seen, the sums behind the last flag)
//   PHASE 1  one workgroup: agg[chunk] = the same over every chunk in front of it (the segmented scan's exclusive prefix)
//   PHASE 2  the DC differences become DC values, in place
struct DcAcc { int f, y, cb, cr; };
// on agg's int4 (f, y, cb, cr): what stands behind a flag forgets what stood in front of it
__device__ __forceinline__ int4 dc_join(const int4& a, const int4& b) {
  return b.x ? b : make_int4(a.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
template <int PHASE>
__global__ void __launch_bounds__(256) jpegdec_dc_kernel(Plan P, int16_t* __restrict__ coef, const uint8_t* __restrict__ flags,
                                                         int4* __restrict__ agg, long nchunks) {
  if (PHASE == 1) {
    __shared__ int4 part[256];
    chunked_scan_256(
        part, nchunks, make_int4(0, 0, 0, 0), [&](long i) { return agg[i]; }, dc_join, [&](long i, const int4& pre) { agg[i] = pre; });
    return;
  }
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= nchunks) return;
  const long mcus = (long)P.mcus_x * P.mcus_y;
  const long m0 = c * kDcChunk, m1 = lmin(m0 + kDcChunk, mcus);
  DcAcc acc{0, 0, 0, 0};
  if (PHASE == 2) {
    const int4 v = agg[c];
    acc = DcAcc{0, v.y, v.z, v.w};
  }
  for (long m = m0; m < m1; ++m) {
    if (flags[m]) acc = DcAcc{1, 0, 0, 0};
    for (int s = 0; s < P.bpm; ++s) {
      int16_t* dc = coef + (m * P.bpm + s) * 64;
      const int comp = comp_of_slot(s, P.bpm, P.ncomp);
      if (comp == 0) {
        acc.y += *dc;
        if (PHASE == 2) *dc = (int16_t)acc.y;
      } else if (comp == 1) {
        acc.cb += *dc;
        if (PHASE == 2) *dc = (int16_t)acc.cb;
      } else {
        acc.cr += *dc;
        if (PHASE == 2) *dc = (int16_t)acc.cr;
      }
    }
  }
  if (PHASE == 0) agg[c] = make_int4(acc.f, acc.y, acc.cb, acc.cr);
}

// ---------------------------------------------------------------- IDCT ------------------------------------------------------
// 32 blocks per workgroup, eight lanes per block.  Column pass: lane (block j, column c); the transpose goes through `tmp`
// with 9 dwords per row, so that the eight rows a lane writes and the eight columns it reads next hit different banks
// (jpeg.hip's forward transform, mirrored); row pass: lane (block j, row r) writes the row's eight samples as two dwords.
constexpr int kIdctBlocks = 32, kTmpPitch = 9, kTmpBlock = 72;
__global__ void __launch_bounds__(256) jpegdec_idct_kernel(Plan P, const int16_t* __restrict__ coef, uint8_t* __restrict__ plane0,
                                                           uint8_t* __restrict__ plane1, uint8_t* __restrict__ plane2, int pitch0,
                                                           int pitch12) {
  __shared__ __attribute__((aligned(16))) int16_t cf[kIdctBlocks * 64];
  __shared__ int tmp[4][8 * kTmpBlock];
  __shared__ uint8_t q[3 * 64];
  const int tid = threadIdx.x;
  const long b0 = (long)blockIdx.x * kIdctBlocks;
  const int nb = (int)lmin((long)kIdctBlocks, P.nblocks - b0);
  const uint4* src = (const uint4*)(coef + b0 * 64);
  for (int i = tid; i < nb * 8; i += 256) ((uint4*)cf)[i] = src[i];
  if (tid < 64 * P.ncomp) q[tid] = P.q[tid >> 6][tid & 63];
  __syncthreads();
  const int wv = tid >> 6, lane = tid & 63, j = lane >> 3, c = lane & 7;
  const int bl = wv * 8 + j;
  const bool valid = bl < nb;
  const long b = b0 + bl;
  const int slot = (int)(b % P.bpm);
  const int comp = comp_of_slot(slot, P.bpm, P.ncomp);
  uint32_t in[8];
  int32_t out[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int kk = kIzzDev.p[r * 8 + c];
    in[r] = valid ? (uint32_t)(int32_t)cf[bl * 64 + kk] * (uint32_t)q[comp * 64 + kk] : 0u;
  }
  idct_1d(in, out, 11);
  int* t = tmp[wv] + j * kTmpBlock;
#pragma unroll
  for (int r = 0; r < 8; ++r) t[r * kTmpPitch + c] = out[r];
  __syncthreads();
#pragma unroll
  for (int x = 0; x < 8; ++x) in[x] = (uint32_t)t[c * kTmpPitch + x];   // c is the row now
  idct_1d(in, out, 18);
  if (!valid) return;
  const long m = b / P.bpm;
  const int mx = (int)(m % P.mcus_x), my = (int)(m / P.mcus_x);
  uint8_t* plane = comp == 0 ? plane0 : comp == 1 ? plane1 : plane2;
  const int pitch = comp == 0 ? pitch0 : pitch12;
  const int bx = comp == 0 ? mx * P.hs + slot % P.hs : mx, by = comp == 0 ? my * P.vs + slot / P.hs : my;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    lo |= (uint32_t)sample_of(out[x]) << (8 * x);
    hi |= (uint32_t)sample_of(out[4 + x]) << (8 * x);
  }
  // block (by, bx) lies inside the plane of mcus_y vs 8 rows of pitch bytes; pitch is a multiple of 8 and the plane's base of 256
  *(uint2*)(plane + ((size_t)by * 8 + c) * pitch + (size_t)bx * 8) = make_uint2(lo, hi);
}

// ---------------------------------------------------------------- upsampling, colour, orientation ---------------------------
// One lane per pixel of the file's own h x w; only samples inside the cropped planes are read.
__global__ void __launch_bounds__(256) jpegdec_final_kernel(Plan P, const uint8_t* __restrict__ plane0, const uint8_t* __restrict__ plane1,
                                                            const uint8_t* __restrict__ plane2, int pitch0, int pitch12,
                                                            uint8_t* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)P.h * P.w) return;
  const int y = (int)(idx / P.w), x = (int)(idx % P.w);
  int r, g, b;
  r = g = b = plane0[(size_t)y * pitch0 + x];
  if (P.ncomp == 3) {
    const int cw = (P.w + P.hs - 1) / P.hs, ch = (P.h + P.vs - 1) / P.vs;
    const int cb = chroma_at(plane1, pitch12, P.hs, P.vs, ch, cw, y, x);
    const int cr = chroma_at(plane2, pitch12, P.hs, P.vs, ch, cw, y, x);
    ycc_rgb(r, cb, cr, &r, &g, &b);
  }
  int yo, xo;
  oriented(P.orientation, P.h, P.w, y, x, &yo, &xo);
  uint8_t* dst = out + ((size_t)yo * P.out_w + xo) * 3;
  dst[0] = (uint8_t)r;
  dst[1] = (uint8_t)g;
  dst[2] = (uint8_t)b;
}

static void fill_info(const Plan& P, dvd_jpegdec_info* info) {
  info->h = P.h;
  info->w = P.w;
  info->out_h = P.out_h;
  info->out_w = P.out_w;
  info->components = P.ncomp;
  info->hs = P.hs;
  info->vs = P.vs;
  info->orientation = P.orientation;
  info->restart_interval = P.ri;
  info->scan_offset = P.scan_off;
  info->scan_bytes = P.scan_len;
  info->blocks = P.nblocks;
  info->scratch_bytes = (long)layout_of(P).total;
}

static int parse_or_refuse(const char* what, const uint8_t* file_host, long n, Plan* P) {
  const char* why = "";
  const int rc = parse(file_host, n, P, &why);
  if (rc) set_error("%s: refused: %s", what, why);
  return rc;
}

}  // namespace jpegdec
}  // namespace dvd

using namespace dvd;

extern "C" int dvd_jpegdec_probe(const uint8_t* file_host, long n, dvd_jpegdec_info* info) {
  DVD_REQUIRE(file_host && info, "jpegdec_probe: null pointer");
  DVD_REQUIRE(n >= 1, "jpegdec_probe: bad length %ld", n);
  jpegdec::Plan P;
  const int rc = jpegdec::parse_or_refuse("jpegdec_probe", file_host, n, &P);
  if (rc) return rc;
  jpegdec::fill_info(P, info);
  return DVD_OK;
}

extern "C" int dvd_jpeg_decode_rgb8(const uint8_t* file_host, const uint8_t* file_dev, long n, uint8_t* out_hwc, long cap,
                                    int max_iters, int* iters_out, void* scratch, void* stream) {
  using namespace jpegdec;
  DVD_REQUIRE(file_host && file_dev && out_hwc && scratch, "jpeg_decode_rgb8: null pointer");
  DVD_REQUIRE(n >= 1, "jpeg_decode_rgb8: bad length %ld", n);
  DVD_REQUIRE(max_iters >= 0, "jpeg_decode_rgb8: max_iters %d is negative (0 = the default, %d)", max_iters, kDefaultMaxIters);
  DVD_REQUIRE(((uintptr_t)scratch & 15) == 0, "jpeg_decode_rgb8: scratch must be 16-byte aligned");
  Plan P;
  const int rc = parse_or_refuse("jpeg_decode_rgb8", file_host, n, &P);
  if (rc) return rc;
  DVD_REQUIRE(cap >= 3L * P.h * P.w, "jpeg_decode_rgb8: cap %ld below 3 h w = %ld", cap, 3L * P.h * P.w);
  if (iters_out) *iters_out = 0;
  if (P.nsub == 0) {
    set_error("jpeg_decode_rgb8: the scan is empty");
    return DVD_E_JPEG_DATA;
  }
  if (max_iters == 0) max_iters = kDefaultMaxIters;
  hipStream_t st = (hipStream_t)stream;
  const Layout l = layout_of(P);
  uint8_t* base = (uint8_t*)scratch;
  unsigned long long* E = (unsigned long long*)(base + l.state);
  uint8_t* chg[2] = {base + l.chg0, base + l.chg1};
  uint32_t* ctr = (uint32_t*)(base + l.ctr);
  uint32_t* counts = (uint32_t*)(base + l.counts);
  uint32_t* first = (uint32_t*)(base + l.first);
  uint8_t* flags = base + l.flags;
  int4* agg = (int4*)(base + l.agg);
  int16_t* coef = (int16_t*)(base + l.coef);
  uint8_t* plane[3] = {base + l.plane[0], base + l.plane[P.ncomp == 3 ? 1 : 0], base + l.plane[P.ncomp == 3 ? 2 : 0]};
  const uint8_t* scan = file_dev + P.scan_off;
  const unsigned lanes = (unsigned)cdiv(P.nsub, 256);
  auto read_back = [&](const uint32_t* src, uint32_t* dst) {
    if (hipMemcpyAsync(dst, src, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      set_error("jpeg_decode_rgb8: read-back: %s", hipGetErrorString(hipGetLastError()));
      return false;
    }
    return true;
  };
  jpegdec_init_kernel<<<(unsigned)cdiv(P.nsub + 1, 256), 256, 0, st>>>(E, chg[0], chg[1], ctr, P.nsub);
  int it = 0;
  bool synced = false;
  while (it < max_iters && !synced) {
    const int group = max_iters - it < kGroup ? max_iters - it : kGroup;
    for (int k = 0; k < group; ++k, ++it)
      jpegdec_sync_kernel<<<lanes, 256, 0, st>>>(P, scan, E, chg[it & 1], chg[(it + 1) & 1], ctr, it);
    uint32_t stamp = 0;
    if (!read_back(ctr, &stamp)) return DVD_E_LAUNCH;
    if ((int)stamp < it) {                                  // the group's last iteration changed nothing: the fixpoint
      synced = true;
      it = (int)stamp + 1;
    }
  }
  if (iters_out) *iters_out = it;
  if (!synced) {
    set_error("jpeg_decode_rgb8: no fixpoint within %d iterations", max_iters);
    return DVD_E_JPEG_NOSYNC;
  }
  jpegdec_count_kernel<<<lanes, 256, 0, st>>>(P, scan, E, counts);
  jpegdec_scan_kernel<<<1, 256, 0, st>>>(counts, P.nsub, first, ctr);
  uint32_t total = 0;
  if (!read_back(ctr + 1, &total)) return DVD_E_LAUNCH;
  if ((long)total != P.nblocks) {
    set_error("jpeg_decode_rgb8: the scan holds %u blocks, the header implies %ld", total, P.nblocks);
    return DVD_E_JPEG_DATA;
  }
  const long mcus = (long)P.mcus_x * P.mcus_y;
  if (hipMemsetAsync(coef, 0, (size_t)P.nblocks * 128, st) != hipSuccess || hipMemsetAsync(flags, 0, (size_t)mcus, st) != hipSuccess)
    return check_launch("jpeg_decode_rgb8");
  jpegdec_write_kernel<<<lanes, 256, 0, st>>>(P, scan, E, first, coef, flags);
  const unsigned chunks = (unsigned)cdiv(l.nchunks, 256);
  jpegdec_dc_kernel<0><<<chunks, 256, 0, st>>>(P, coef, flags, agg, l.nchunks);
  jpegdec_dc_kernel<1><<<1, 256, 0, st>>>(P, coef, flags, agg, l.nchunks);
  jpegdec_dc_kernel<2><<<chunks, 256, 0, st>>>(P, coef, flags, agg, l.nchunks);
  jpegdec_idct_kernel<<<(unsigned)cdiv(P.nblocks, kIdctBlocks), 256, 0, st>>>(P, coef, plane[0], plane[1], plane[2], l.pitch[0], l.pitch[1]);
  jpegdec_final_kernel<<<(unsigned)cdiv((long)P.h * P.w, 256), 256, 0, st>>>(P, plane[0], plane[1], plane[2], l.pitch[0], l.pitch[1], out_hwc);
  return check_launch("jpeg_decode_rgb8");
}
