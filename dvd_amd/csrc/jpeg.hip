// Baseline JPEG encoder for uint8 RGB pages on the device where the unwarp tail leaves them (DESIGN.md section 4.5 holds the
// format; jpeg_core.h its arithmetic, shared with the CPU restatement jpeg_host_check.cpp).  The file is a pure function of
// (h, w, pixels, quality, subsampling): integers only, no atomics on global memory, no dependence on the batch, the stream or
// the device.  One restart interval per MCU row makes the entropy-coded data a row of independent, byte-aligned pieces.
//   jpeg_transform_kernel  one workgroup per strip of kStripPx pixel columns of one MCU row: the HWC bytes through LDS, YCbCr,
//                          the 2 x 2 chroma average, level shift, 8 x 8 DCT (rows, then columns, eight lanes per block),
//                          quantisation -> zig-zag int16 coefficients in MCU order
//   jpeg_entropy_kernel    one workgroup per interval, kTile blocks at a time: bit lengths, scan, the blocks' bits joined in
//                          LDS, byte stuffing (count, scan, write) -> the interval's slot and its length; both scans are
//                          block_ops.h's block_scan_256
//   jpeg_layout_kernel     scan of the interval lengths (chunked_scan_256) -> file offsets; the header; the file's length
//   jpeg_gather_kernel     one workgroup per interval: its bytes and its marker (RSTn, EOI after the last) into the file
#include "common.h"
#include "block_ops.h"
#include "jpeg_core.h"
#include "workspace.h"

namespace dvd {
namespace jpeg {

__device__ const HuffEnc kEncDev[2] = {make_enc(0), make_enc(1)};

// natural index -> position in the zig-zag sequence
struct Izz { uint8_t p[64]; };
constexpr Izz make_izz() {
  Izz z{};
  for (int k = 0; k < 64; ++k) z.p[kZigzag[k]] = (uint8_t)k;
  return z;
}
__device__ const Izz kIzzDev = make_izz();

__device__ __forceinline__ uint32_t add_u32(uint32_t a, uint32_t b) { return a + b; }

// ---------------------------------------------------------------- transform -------------------------------------------------
constexpr int kStripPx = 256;                 // pixel columns per workgroup: 16 MCUs of 4:2:0, 32 of 4:4:4
constexpr int kStripBlocks = 96;              // 16 x 6 = 32 x 3 blocks: three rounds of 4 waves x 8 blocks
constexpr int kTmpPitch = 9, kTmpBlock = 72;  // dwords per row / block of the transpose buffer: 8 rows of 8 + 1

// The transpose between the passes goes through `tmp`, 9 dwords per row: lane (block j, row r) writes dwords 72 j + 9 r + u,
// lane (block j, column c) reads 72 j + 9 y + c.  Within a half-wave (4 blocks) both hit 32 different banks.
template <int SS>
__global__ void __launch_bounds__(256) jpeg_transform_kernel(const uint8_t* __restrict__ img, int h, int w, int mcus_x,
                                                             QuantTables qt, int16_t* __restrict__ coef) {
  constexpr int M = SS == DVD_JPEG_420 ? 16 : 8;          // MCU side in pixels
  constexpr int BPM = SS == DVD_JPEG_420 ? 6 : 3;
  constexpr int MPS = kStripPx / M;                       // MCUs per strip
  static_assert(MPS * BPM == kStripBlocks, "");
  __shared__ uint8_t raw[M][3 * kStripPx];
  __shared__ __attribute__((aligned(16))) int16_t blk[kStripBlocks * 64];
  __shared__ int tmp[4][8 * kTmpBlock];
  __shared__ uint16_t q[2][64];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kStripPx, y0 = blockIdx.y * M;
  const int cols = min(kStripPx, w - x0), rows = min(M, h - y0);   // pixels of the image in the strip: both >= 1
  // neighbouring lanes take neighbouring bytes; a row starts at any byte address, so the loads are byte-wide
  for (int r = 0; r < rows; ++r) {
    const uint8_t* src = img + ((size_t)(y0 + r) * w + x0) * 3;
    for (int i = tid; i < 3 * cols; i += 256) raw[r][i] = src[i];
  }
  if (tid < 128) q[tid >> 6][tid & 63] = qt.q[tid >> 6][tid & 63];
  __syncthreads();
  // samples, level-shifted, into the blocks of the strip's MCUs; pixels past the image repeat its last row / column
  if (SS == DVD_JPEG_420) {
    for (int i = 0; i < 4; ++i) {                         // 8 x 128 quads of 2 x 2 pixels
      const int qd = tid + 256 * i, qy = qd >> 7, qx = qd & 127;
      const int m = qx >> 3;
      int cb[4], cr[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int py = 2 * qy + (d >> 1), px = 2 * (qx & 7) + (d & 1);                 // inside the MCU
        const uint8_t* p = &raw[min(py, rows - 1)][3 * min(16 * m + px, cols - 1)];
        const int r = p[0], g = p[1], b = p[2];
        blk[(m * 6 + (py >> 3) * 2 + (px >> 3)) * 64 + (py & 7) * 8 + (px & 7)] = (int16_t)(rgb_y(r, g, b) - 128);
        cb[d] = rgb_cb(r, g, b);
        cr[d] = rgb_cr(r, g, b);
      }
      blk[(m * 6 + 4) * 64 + qy * 8 + (qx & 7)] = (int16_t)(box4(cb[0], cb[1], cb[2], cb[3]) - 128);
      blk[(m * 6 + 5) * 64 + qy * 8 + (qx & 7)] = (int16_t)(box4(cr[0], cr[1], cr[2], cr[3]) - 128);
    }
  } else {
    for (int i = 0; i < 8; ++i) {                         // 8 x 256 pixels
      const int py = i, px = tid;
      const int m = px >> 3;
      const uint8_t* p = &raw[min(py, rows - 1)][3 * min(px, cols - 1)];
      const int r = p[0], g = p[1], b = p[2];
      int16_t* dst = blk + m * 3 * 64 + py * 8 + (px & 7);
      dst[0] = (int16_t)(rgb_y(r, g, b) - 128);
      dst[64] = (int16_t)(rgb_cb(r, g, b) - 128);
      dst[128] = (int16_t)(rgb_cr(r, g, b) - 128);
    }
  }
  __syncthreads();
  const int wv = tid >> 6, lane = tid & 63, j = lane >> 3, r = lane & 7;
  int* t = tmp[wv] + j * kTmpBlock;
  for (int round = 0; round < 3; ++round) {
    const int b = (round * 4 + wv) * 8 + j;
    int in[8], out[8];
    const uint4 v = *(const uint4*)(blk + b * 64 + r * 8);
    in[0] = (int16_t)(v.x & 0xFFFF); in[1] = (int16_t)(v.x >> 16);
    in[2] = (int16_t)(v.y & 0xFFFF); in[3] = (int16_t)(v.y >> 16);
    in[4] = (int16_t)(v.z & 0xFFFF); in[5] = (int16_t)(v.z >> 16);
    in[6] = (int16_t)(v.w & 0xFFFF); in[7] = (int16_t)(v.w >> 16);
    dct8_rows(in, out);
#pragma unroll
    for (int u = 0; u < 8; ++u) t[r * kTmpPitch + u] = out[u];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = t[y * kTmpPitch + r];   // r is the column now
    dct8_cols(in, out);
    const uint16_t* qq = q[(b % BPM) >= BPM - 2];
#pragma unroll
    for (int vv = 0; vv < 8; ++vv) blk[b * 64 + kIzzDev.p[vv * 8 + r]] = (int16_t)quantize(out[vv], qq[vv * 8 + r]);
    __syncthreads();                                      // tmp is written again in the next round
  }
  // the strip's blocks are contiguous in MCU order; blocks of MCUs past the row's last are not written
  const int m0 = blockIdx.x * MPS;
  const int nvalid = min(MPS, mcus_x - m0) * BPM;
  uint4* dst = (uint4*)(coef + ((size_t)blockIdx.y * mcus_x + m0) * BPM * 64);
  for (int i = tid; i < nvalid * 8; i += 256) dst[i] = ((const uint4*)blk)[i];
}

// ---------------------------------------------------------------- entropy coding --------------------------------------------
struct LdsOps {
  static __device__ __forceinline__ void store32(uint32_t* p, uint32_t v) { *p = v; }
  static __device__ __forceinline__ void or32(uint32_t* p, uint32_t v) { atomicOr(p, v); }   // LDS only
};

// One workgroup per interval.  A tile is kTile consecutive blocks, one per thread.  `words` holds the tile's bitstream in front
// of which stand the `carry` < 32 bits that the tile before left in word 0; all but the last tile hand their complete words to
// the stuffing pass and carry the rest, the last one is padded with 1-bits to a byte.
__global__ void __launch_bounds__(256) jpeg_entropy_kernel(const int16_t* __restrict__ coef, long row_blocks, int bpm,
                                                           uint8_t* __restrict__ slots, long slot_bytes,
                                                           uint32_t* __restrict__ lens) {
  __shared__ uint32_t words[kTileWords];
  __shared__ uint32_t scan[256];
  const int tid = threadIdx.x;
  const int16_t* base = coef + (size_t)blockIdx.x * row_blocks * 64;
  uint8_t* out = slots + (size_t)blockIdx.x * slot_bytes;
  long outpos = 0;
  uint32_t carry = 0;
  if (tid == 0) words[0] = 0;
  for (long t0 = 0; t0 < row_blocks; t0 += kTile) {
    const long b = t0 + tid;
    const bool have = b < row_blocks;
    const bool last = t0 + kTile >= row_blocks;
    const int16_t* zz = base + b * 64;
    const HuffEnc& enc = kEncDev[have && is_chroma(b, bpm)];
    int pred = 0;
    uint32_t bits = 0;
    if (have) {
      const int d = pred_distance(b, bpm);
      pred = d ? zz[-64 * d] : 0;
      CountSink cs{0};
      encode_block(zz, pred, enc, cs);
      bits = (uint32_t)cs.bits;
    }
    uint32_t total;
    const uint32_t incl = block_scan_256(scan, bits, 0u, add_u32, &total);
    const uint32_t end = carry + total;                   // bits in `words` after this tile: < 32 + kTile * kBlockBitsMax
    for (uint32_t i = 1 + tid; i <= (end >> 5); i += 256) words[i] = 0;
    __syncthreads();
    if (have) {
      EmitSink<LdsOps> es(words, (long)(carry + incl - bits));
      encode_block(zz, pred, enc, es);
      es.finish();
    }
    __syncthreads();
    uint32_t nbytes = (end >> 5) * 4;
    if (last) {
      const uint32_t pad = (8 - (end & 7)) & 7;
      if (tid == 0 && pad) words[end >> 5] |= ((1u << pad) - 1u) << (32 - (end & 31) - pad);
      nbytes = (end + 7) >> 3;
      __syncthreads();
    }
    const uint32_t rest = words[end >> 5];                // the word the next tile starts in
    // stuffing: a run of bytes per thread; count its 0xFF, scan, write the run with a 0x00 behind each 0xFF
    const uint32_t per = (nbytes + 255) / 256;
    const uint32_t lo = min(tid * per, nbytes), hi = min(lo + per, nbytes);
    uint32_t ff = 0;
    for (uint32_t i = lo; i < hi; ++i) ff += stream_byte(words, i) == 0xFF;
    uint32_t ff_total;
    const uint32_t ff_incl = block_scan_256(scan, ff, 0u, add_u32, &ff_total);
    uint8_t* dst = out + outpos + lo + (ff_incl - ff);
    for (uint32_t i = lo; i < hi; ++i) {
      const uint8_t v = stream_byte(words, i);
      *dst++ = v;
      if (v == 0xFF) *dst++ = 0;
    }
    outpos += nbytes + ff_total;
    carry = end & 31;
    __syncthreads();                                      // every read of `words` and `scan` is done
    if (tid == 0) words[0] = carry ? rest : 0u;
  }
  if (tid == 0) lens[blockIdx.x] = (uint32_t)outpos;
}

// ---------------------------------------------------------------- layout ----------------------------------------------------
// One workgroup.  offs[i] = file position of interval i; each interval is followed by a 2-byte marker.
__global__ void __launch_bounds__(256) jpeg_layout_kernel(const uint32_t* __restrict__ lens, int n, Header hd,
                                                          unsigned long long* __restrict__ offs, uint8_t* __restrict__ out,
                                                          unsigned long long* __restrict__ out_len) {
  __shared__ unsigned long long part[256];
  const int tid = threadIdx.x;
  const unsigned long long body = chunked_scan_256(
      part, n, 0ull, [&](int i) { return 2ull + lens[i]; }, [](unsigned long long a, unsigned long long b) { return a + b; },
      [&](int i, unsigned long long pre) { offs[i] = (unsigned long long)kHeaderBytes + pre; });
  for (int i = tid; i < kHeaderBytes; i += 256) out[i] = hd.b[i];
  if (tid == 0) *out_len = (unsigned long long)kHeaderBytes + body;
}

// ---------------------------------------------------------------- gather ----------------------------------------------------
__global__ void __launch_bounds__(256) jpeg_gather_kernel(const uint8_t* __restrict__ slots, long slot_bytes,
                                                          const uint32_t* __restrict__ lens,
                                                          const unsigned long long* __restrict__ offs, int n,
                                                          uint8_t* __restrict__ out) {
  const int tid = threadIdx.x;
  const int iv = blockIdx.x;
  const uint8_t* src = slots + (size_t)iv * slot_bytes;
  const uint32_t len = lens[iv];
  uint8_t* dst = out + offs[iv];
  for (uint32_t i = tid; i < len; i += 256) dst[i] = src[i];
  if (tid == 0) {
    dst[len] = 0xFF;
    dst[len + 1] = iv == n - 1 ? 0xD9 : (uint8_t)(0xD0 + (iv & 7));   // EOI, or RSTm with m = interval mod 8
  }
}

struct Layout { size_t coef, slots, lens, offs, total; };

static Layout layout_of(const Geom& g) {
  Layout l;
  Carver c;
  l.coef = c.take((size_t)g.mcus_y * (size_t)g.row_blocks * 128);
  l.slots = c.take((size_t)g.mcus_y * (size_t)interval_slot(g.row_blocks), 1);   // not rounded up: a slot is a multiple of 16 only
  l.lens = c.take((size_t)g.mcus_y * sizeof(uint32_t));
  l.offs = c.take((size_t)g.mcus_y * sizeof(unsigned long long));
  l.total = c.at;
  return l;
}

static bool subsampling_ok(int ss) { return ss == DVD_JPEG_420 || ss == DVD_JPEG_444; }

}  // namespace jpeg
}  // namespace dvd

using namespace dvd;

static const char* jpeg_size_args(const char* what, int h, int w, int ss) {
  if (!jpeg::shape_ok(h, w)) {
    set_error("%s: bad shape %dx%d (1 <= h, w <= 65535 and the padded planes below 2^31 bytes)", what, h, w);
    return "shape";
  }
  if (!jpeg::subsampling_ok(ss)) {
    set_error("%s: unknown subsampling %d (DVD_JPEG_420 or DVD_JPEG_444)", what, ss);
    return "subsampling";
  }
  return nullptr;
}

extern "C" long dvd_jpeg_bound(int h, int w, int subsampling) {
  if (jpeg_size_args("jpeg_bound", h, w, subsampling)) return DVD_E_ARG;
  return jpeg::file_bound(jpeg::geom_of(h, w, subsampling));
}

extern "C" long dvd_jpeg_scratch_bytes(int h, int w, int subsampling) {
  if (jpeg_size_args("jpeg_scratch_bytes", h, w, subsampling)) return DVD_E_ARG;
  return (long)jpeg::layout_of(jpeg::geom_of(h, w, subsampling)).total;
}

extern "C" int dvd_jpeg_encode_rgb8(const uint8_t* img_hwc, int h, int w, int quality, int subsampling, uint8_t* out, long cap,
                                    unsigned long long* out_len, void* scratch, void* stream) {
  DVD_REQUIRE(img_hwc && out && out_len && scratch, "jpeg_encode_rgb8: null pointer");
  DVD_REQUIRE(h >= 1 && w >= 1, "jpeg_encode_rgb8: bad shape %dx%d (h >= 1, w >= 1)", h, w);
  DVD_REQUIRE(jpeg::shape_ok(h, w), "jpeg_encode_rgb8: image %dx%d too large (h, w <= 65535 and the padded planes below 2^31 bytes)",
              h, w);
  DVD_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode_rgb8: quality %d outside 1..100", quality);
  DVD_REQUIRE(jpeg::subsampling_ok(subsampling), "jpeg_encode_rgb8: unknown subsampling %d (DVD_JPEG_420 or DVD_JPEG_444)",
              subsampling);
  const jpeg::Geom g = jpeg::geom_of(h, w, subsampling);
  // before anything is launched: no kernel can write past the caller's buffer
  DVD_REQUIRE(cap >= jpeg::file_bound(g), "jpeg_encode_rgb8: cap %ld below dvd_jpeg_bound(%d, %d, %d) = %ld", cap, h, w,
              subsampling, jpeg::file_bound(g));
  DVD_REQUIRE(((uintptr_t)scratch & 15) == 0, "jpeg_encode_rgb8: scratch must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const jpeg::Layout l = jpeg::layout_of(g);
  uint8_t* base = (uint8_t*)scratch;
  int16_t* coef = (int16_t*)(base + l.coef);
  uint8_t* slots = base + l.slots;
  uint32_t* lens = (uint32_t*)(base + l.lens);
  unsigned long long* offs = (unsigned long long*)(base + l.offs);
  const long slot = jpeg::interval_slot(g.row_blocks);
  const jpeg::QuantTables qt = jpeg::quant_tables(quality);
  const jpeg::Header hd = jpeg::make_header(h, w, g, qt);
  const dim3 grid((unsigned)cdiv(w, jpeg::kStripPx), (unsigned)g.mcus_y);
  if (subsampling == DVD_JPEG_420)
    jpeg::jpeg_transform_kernel<DVD_JPEG_420><<<grid, 256, 0, st>>>(img_hwc, h, w, g.mcus_x, qt, coef);
  else
    jpeg::jpeg_transform_kernel<DVD_JPEG_444><<<grid, 256, 0, st>>>(img_hwc, h, w, g.mcus_x, qt, coef);
  jpeg::jpeg_entropy_kernel<<<g.mcus_y, 256, 0, st>>>(coef, g.row_blocks, g.bpm, slots, slot, lens);
  jpeg::jpeg_layout_kernel<<<1, 256, 0, st>>>(lens, g.mcus_y, hd, offs, out, out_len);
  jpeg::jpeg_gather_kernel<<<g.mcus_y, 256, 0, st>>>(slots, slot, lens, offs, g.mcus_y, out);
  return check_launch("jpeg_encode_rgb8");
}
