// Lossless PNG encoder for uint8 RGB pages on the device where the unwarp tail leaves them (DESIGN.md section 4.4 holds the
// format; png_core.h its arithmetic, shared with the CPU restatement png_host_check.cpp).  The file is a pure function of
// (h, w, pixels): no atomics, no dependence on the batch, the stream or the device.
//   png_filter_kernel     one row per workgroup: the five filters' costs, the winner's bytes -> the filtered stream
//   png_compress_kernel   one wave per DVD_PNG_SEGMENT bytes of that stream: LZ77 + one fixed-Huffman block -> the segment's slot,
//                         its length and Adler-32 partials
//   png_compress_dyn_kernel  DVD_PNG_HUFFMAN_DYNAMIC: the same token loop into 16-bit tokens, their histograms, the two
//                         length-limited codes, then the smaller of the dynamic and the fixed block written by all lanes
//   png_layout_kernel     exclusive scan of the chunk sizes (chunked_scan_256), signature, IHDR, IEND, the Adler-32, the
//                         file's length
//   png_gather_kernel     one workgroup per segment: its IDAT chunk (length, type, data, CRC-32) into the contiguous file
// Both compress kernels begin with stage_segment; the wave sums and the scan are block_ops.h's, the scratch layout workspace.h's.
#include "common.h"
#include "block_ops.h"
#include "png_core.h"
#include "workspace.h"

namespace dvd {
namespace png {

// ---------------------------------------------------------------- filter ----------------------------------------------------
// Filtering reads raw neighbour bytes only, so rows are independent.  Two passes over the row (the second one hits the cache):
// the costs, then the winner's bytes.  Neighbouring lanes take neighbouring bytes; rows start at any byte address, so the
// accesses are byte-wide.
__global__ void __launch_bounds__(256) png_filter_kernel(const uint8_t* __restrict__ img, int w, uint8_t* __restrict__ filt) {
  __shared__ unsigned long long red[5][4];
  const int tid = threadIdx.x;
  const long rb = 3L * w;
  const long y = blockIdx.x;
  const uint8_t* cur = img + (size_t)y * rb;
  const bool has_up = y > 0;
  const uint8_t* up = has_up ? cur - rb : cur;  // read only when y > 0
  unsigned cost[5] = {0, 0, 0, 0, 0};          // per thread at most rb / 256 * 128 < 2^31
  for (long i = tid; i < rb; i += 256) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
#pragma unroll
    for (int f = 0; f < 5; ++f) cost[f] += residual_cost(filter_byte(f, x, a, b, c));
  }
  unsigned long long sum[5];
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    sum[f] = wave_sum((unsigned long long)cost[f]);
    if ((tid & 63) == 0) red[f][tid >> 6] = sum[f];
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < 5; ++f) sum[f] = red[f][0] + red[f][1] + red[f][2] + red[f][3];
  const int best = pick_filter(sum);
  uint8_t* dst = filt + (size_t)y * (rb + 1);
  if (tid == 0) dst[0] = (uint8_t)best;
  for (long i = tid; i < rb; i += 256) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
    dst[1 + i] = filter_byte(best, x, a, b, c);
  }
}

// ---------------------------------------------------------------- segment compressor ----------------------------------------
struct SegMeta { uint32_t len, a, b, pad; };   // compressed bytes in the slot, Adler-32 partials of the segment's stream bytes

// The wave runs the token loop in step (every value of the loop is wave-uniform); the lanes share the match extension (64
// bytes per step, one ballot) and lane 0 stores the output words.
struct WaveOps {
  static __device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
  static __device__ __forceinline__ int match_len(const uint8_t* seg, int cand, int pos, int maxlen) {
    const int lane = threadIdx.x;
    for (int k = 0; k < maxlen; k += kWave) {
      const int i = k + lane;
      const bool differs = i < maxlen ? seg[cand + i] != seg[pos + i] : true;   // lanes past maxlen end the match
      const unsigned long long m = __ballot(differs);
      if (m) return k + __builtin_ctzll(m);
    }
    return maxlen;
  }
  static __device__ __forceinline__ void store32(uint32_t* p, uint32_t v) { if (threadIdx.x == 0) *p = v; }
  static __device__ __forceinline__ void store16(uint16_t* p, uint16_t v) { *p = v; }   // all lanes: one address, one value
  static __device__ __forceinline__ void store_tok(uint16_t* p, uint16_t v) { if (threadIdx.x == 0) *p = v; }
  static __device__ __forceinline__ int lane() { return threadIdx.x; }
  static __device__ __forceinline__ int lanes() { return kWave; }
  // an LDS integer atomic: integer sums do not depend on the order of the additions, so the histogram is the tokens' alone
  static __device__ __forceinline__ void count(uint32_t* p) { atomicAdd(p, 1u); }
};

// What both compress kernels begin with: the segment's bytes into LDS, the hash table cleared, the segment's Adler-32
// partials (valid in lane 0).  Returns the segment's length.
__device__ __forceinline__ int stage_segment(const uint8_t* __restrict__ filt, long stream, long s, uint8_t* seg, uint16_t* table,
                                             uint32_t* adler_a, uint32_t* adler_b) {
  const int lane = threadIdx.x;
  const long base = s * kSeg;
  const int n = (int)(stream - base < kSeg ? stream - base : kSeg);
  // 16 bytes per lane; the filtered stream's buffer is padded to a multiple of 256 bytes, so the last vector stays inside it
  const uint4* src = (const uint4*)(filt + base);
  for (int k = lane; k * 16 < n; k += kWave) ((uint4*)seg)[k] = src[k];
  for (int k = lane; k < kHashSize; k += kWave) table[k] = (uint16_t)kEmpty;
  __syncthreads();
  unsigned long long a = 0, b = 0;             // b < 32768 * 255 * 512
  for (int k = lane; k < n; k += kWave) {
    a += seg[k];
    b += (unsigned long long)(n - k) * seg[k];
  }
  *adler_a = (uint32_t)(wave_sum(a) % kAdlerMod);
  *adler_b = (uint32_t)(wave_sum(b) % kAdlerMod);
  return n;
}

// LDS: the segment (kSeg bytes) and the hash table (8 KB), both written by this kernel before they are read.
__global__ void __launch_bounds__(kWave) png_compress_kernel(const uint8_t* __restrict__ filt, long stream, int nseg,
                                                              uint8_t* __restrict__ slots, SegMeta* __restrict__ meta) {
  __shared__ __attribute__((aligned(16))) uint8_t seg[kSeg];
  __shared__ uint16_t table[kHashSize];
  const long s = blockIdx.x;
  uint32_t a, b;
  const int n = stage_segment(filt, stream, s, seg, table, &a, &b);
  const int len = compress_segment<WaveOps>(seg, n, table, (uint32_t*)(slots + s * kSlot), s == 0, s == nseg - 1);
  if (threadIdx.x == 0) meta[s] = SegMeta{(uint32_t)len, a, b, 0u};
}

// ---------------------------------------------------------------- segment compressor, dynamic Huffman ----------------------
// The tokens go to global scratch (2 bytes per stream byte, one 64 KiB run per segment, written by lane 0 as the token loop
// produces them and read back by all lanes, from L2), not to LDS: segment + table + tokens would be 104 KB, one workgroup per
// CU; this way the kernel keeps the fixed route's 40 KB and four workgroups per CU.  Once the token loop has ended, the
// segment's bytes are dead and the DynState (histograms, codes, staging dwords) takes their place in LDS.
//   1. token loop (wave-uniform, as in png_compress_kernel), entries to tok[]
//   2. histograms: the lanes stride over the entries, LDS integer atomics
//   3. lane 0: plan_block - the code lengths, the header, both block types priced, the code tables of the smaller one
//   4. the block's header through the serial bit writer (lane 0 stores), continued by
//   5. the parallel emitter: 64 entries per step, one per lane; a lane looks up its token's bits, an inclusive scan over the
//      wave gives its bit offset, it ORs its (at most 3) dwords into the LDS staging area - two lanes that share a dword are
//      combined there -, then the lanes store the step's complete dwords to the slot and the last partial dword is carried
//   6. end of block, the stored block and 03 00 through the serial bit writer again.
__global__ void __launch_bounds__(kWave) png_compress_dyn_kernel(const uint8_t* __restrict__ filt, long stream, int nseg,
                                                                  uint8_t* __restrict__ slots, uint16_t* tokens,
                                                                  SegMeta* __restrict__ meta) {
  __shared__ __attribute__((aligned(16))) uint8_t seg[kSeg];
  __shared__ uint16_t table[kHashSize];
  static_assert(sizeof(DynState) <= kSeg && alignof(DynState) <= 16, "the DynState takes the segment's place");
  const int lane = threadIdx.x;
  const long s = blockIdx.x;
  uint32_t a, b;
  const int n = stage_segment(filt, stream, s, seg, table, &a, &b);
  if (lane == 0) meta[s] = SegMeta{0u, a, b, 0u};
  uint16_t* tok = tokens + s * kSeg;           // at most n <= kSeg entries
  TokenSink<WaveOps> sink{tok, 0};
  tokenise<WaveOps>(seg, n, table, sink);
  const int m = sink.count;
  __syncthreads();                             // seg is dead from here; lane 0's entries are visible to the wave
  DynState& st = *reinterpret_cast<DynState*>(seg);
  for (int k = lane; k < 288; k += kWave) st.ll_freq[k] = k == 256 ? 1u : 0u;   // one end of block
  if (lane < 32) st.d_freq[lane] = 0;
  for (int k = lane; k < kStageWords; k += kWave) st.stage[k] = 0;
  __syncthreads();
  count_tokens<WaveOps>(tok, m, st);
  __syncthreads();
  if (lane == 0) plan_block(st);
  __syncthreads();
  BitWriter<WaveOps> bw{0, 0, (uint32_t*)(slots + s * kSlot), 0};
  put_block_header(bw, st, s == 0);
  int words = bw.words, cnt = bw.cnt;          // wave-uniform: dwords stored, bits pending in stage[0]
  if (lane == 0) st.stage[0] = (uint32_t)bw.buf;
  __syncthreads();
  for (int i0 = 0; i0 < m; i0 += kWave) {
    const int i = i0 + lane;
    uint64_t bits = 0;
    int nb = 0;
    if (i < m) {
      const uint32_t e = tok[i];
      if (!(e & kDistFlag)) bits = token_bits(st, e, e >= 256 ? (uint32_t)tok[i + 1] : 0u, nb);   // a head's distance word: i + 1 < m
    }
    int incl = nb;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    const int end = cnt + __shfl(incl, kWave - 1, 64);
    if (nb) {
      const int off = cnt + incl - nb;         // <= 31 + 63 * 48: dwords 0 .. 97 of the staging area
      const int w = off >> 5, sh = off & 31;
      const uint64_t lo = bits << sh;
      const uint32_t hi = sh ? (uint32_t)(bits >> (64 - sh)) : 0u;
      atomicOr(&st.stage[w], (uint32_t)lo);    // LDS; OR does not depend on the order
      if ((uint32_t)(lo >> 32)) atomicOr(&st.stage[w + 1], (uint32_t)(lo >> 32));
      if (hi) atomicOr(&st.stage[w + 2], hi);
    }
    __syncthreads();
    const int full = end >> 5;                 // <= 96 complete dwords
    const uint32_t carry = st.stage[full];
    for (int k = lane; k < full; k += kWave) bw.out[words + k] = st.stage[k];
    __syncthreads();
    for (int k = lane; k <= full; k += kWave) st.stage[k] = k == 0 ? carry : 0u;
    __syncthreads();
    words += full;
    cnt = end & 31;
  }
  bw.words = words;
  bw.cnt = cnt;
  bw.buf = WaveOps::uniform(st.stage[0]);
  bw.put(WaveOps::uniform(st.ll_code[256]), (int)WaveOps::uniform(st.ll_len[256]));   // end of block
  const int len = finish_segment(bw, s == nseg - 1);
  if (lane == 0) meta[s].len = (uint32_t)len;
}

// ---------------------------------------------------------------- layout ----------------------------------------------------
DVD_HD void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// One workgroup.  offs[s] = file position of segment s's IDAT chunk; the last chunk also carries the Adler-32.
__global__ void __launch_bounds__(256) png_layout_kernel(const SegMeta* __restrict__ meta, int nseg, long stream, int h, int w,
                                                         unsigned long long* __restrict__ offs, uint32_t* __restrict__ adler_out,
                                                         uint8_t* __restrict__ out, unsigned long long* __restrict__ out_len) {
  __shared__ unsigned long long part[256];
  // a chunk is 12 bytes and its data; the signature and IHDR take the file's first 33 bytes
  const unsigned long long chunks = chunked_scan_256(
      part, nseg, 0ull, [&](int s) { return 12ull + meta[s].len + (s == nseg - 1 ? 4u : 0u); },
      [](unsigned long long a, unsigned long long b) { return a + b; }, [&](int s, unsigned long long pre) { offs[s] = 33ull + pre; });
  if (threadIdx.x == 0) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int k = 0; k < 8; ++k) out[k] = sig[k];
    uint8_t* ih = out + 8;
    put_be32(ih, 13);
    ih[4] = 'I'; ih[5] = 'H'; ih[6] = 'D'; ih[7] = 'R';
    put_be32(ih + 8, (uint32_t)w);
    put_be32(ih + 12, (uint32_t)h);
    ih[16] = 8; ih[17] = 2; ih[18] = 0; ih[19] = 0; ih[20] = 0;   // depth 8, colour type 2 (RGB), deflate, adaptive, no interlace
    put_be32(ih + 21, ~crc_bytes(0xFFFFFFFFu, ih + 4, 17));
    uint32_t A = 1, B = 0;
    for (int s = 0; s < nseg; ++s) {
      const long left = stream - (long)s * kSeg;
      adler_fold(A, B, (uint32_t)(left < kSeg ? left : kSeg), meta[s].a, meta[s].b);
    }
    *adler_out = (B << 16) | A;
    const unsigned long long end = 33ull + chunks;
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int k = 0; k < 12; ++k) out[end + k] = iend[k];
    *out_len = end + 12;
  }
}

// ---------------------------------------------------------------- gather ----------------------------------------------------
// One workgroup per segment.  The chunk's CRC-32 covers the type and the data (for the last chunk the Adler-32 too): thread t
// takes the register state of sub-range t of the data from state 0; the sub-ranges have one length c and are right-aligned
// (leading zero bytes leave a zero state zero), so a tree with the factors x^(8 c 2^k) joins them; the state after "IDAT" is
// carried across the whole data by x^(8 N).
__global__ void __launch_bounds__(256) png_gather_kernel(const uint8_t* __restrict__ slots, const SegMeta* __restrict__ meta,
                                                         const unsigned long long* __restrict__ offs,
                                                         const uint32_t* __restrict__ adler, int nseg, uint8_t* __restrict__ out) {
  __shared__ uint32_t part[256];
  __shared__ uint8_t tail[4];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const uint8_t* src = slots + (size_t)s * kSlot;
  const int len = (int)meta[s].len;
  const int extra = s == nseg - 1 ? 4 : 0;
  const int N = len + extra;                   // the chunk's data bytes
  uint8_t* dst = out + offs[s];
  if (tid == 0 && extra) put_be32(tail, *adler);
  __syncthreads();
  for (int i = tid; i < N; i += 256) dst[8 + i] = i < len ? src[i] : tail[i - len];
  const int c = (N + 255) / 256;
  const int shift = 256 * c - N;               // virtual zero bytes in front
  uint32_t r = 0;
  for (int j = 0; j < c; ++j) {
    const int i = tid * c + j - shift;
    if (i >= 0) r = crc_byte(r, i < len ? src[i] : tail[i - len]);
  }
  part[tid] = r;
  __syncthreads();
  uint32_t f = crc_xpow8((unsigned long long)c);
  for (int d = 1; d < 256; d <<= 1) {
    if ((tid & (2 * d - 1)) == 0) part[tid] = crc_mul(part[tid], f) ^ part[tid + d];
    f = crc_mul(f, f);
    __syncthreads();
  }
  if (tid == 0) {
    put_be32(dst, (uint32_t)N);
    dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T';
    const uint32_t head = crc_bytes(0xFFFFFFFFu, dst + 4, 4);
    put_be32(dst + 8 + N, ~(crc_mul(head, crc_xpow8((unsigned long long)N)) ^ part[0]));
  }
}

struct Layout { size_t filt, slots, meta, offs, adler, total, tokens, total_dyn; };

static Layout layout_of(long stream) {
  const size_t ns = (size_t)segments(stream);
  Layout l;
  Carver c;
  l.filt = c.take((size_t)stream);
  l.slots = c.take(ns * (size_t)kSlot, 1);     // not rounded up: kSlot is a multiple of 16 only
  l.meta = c.take(ns * sizeof(SegMeta));
  l.offs = c.take(ns * sizeof(unsigned long long));
  l.adler = c.take(256);
  l.total = c.at;                              // the fixed route's scratch ends here
  l.tokens = c.take(ns * (size_t)kSeg * sizeof(uint16_t), 1);   // the dynamic route's: 2 bytes per stream byte of a full segment
  l.total_dyn = c.at;
  return l;
}

// h >= 1, w >= 1 and h (3 w + 1) < 2^31, without overflow
static bool shape_ok(int h, int w) { return h >= 1 && w >= 1 && 3L * w + 1 <= ((1L << 31) - 1) / h; }

}  // namespace png
}  // namespace dvd

using namespace dvd;

extern "C" long dvd_png_bound(int h, int w) {
  if (!png::shape_ok(h, w)) {
    set_error("png_bound: bad shape %dx%d (h >= 1, w >= 1, h * (3 w + 1) < 2^31)", h, w);
    return DVD_E_ARG;
  }
  return png::file_bound(png::stream_bytes(h, w));
}

extern "C" long dvd_png_scratch_bytes(int h, int w) {
  if (!png::shape_ok(h, w)) {
    set_error("png_scratch_bytes: bad shape %dx%d (h >= 1, w >= 1, h * (3 w + 1) < 2^31)", h, w);
    return DVD_E_ARG;
  }
  return (long)png::layout_of(png::stream_bytes(h, w)).total;
}

extern "C" long dvd_png_scratch_bytes_huff(int h, int w, int huffman) {
  if (huffman != DVD_PNG_HUFFMAN_FIXED && huffman != DVD_PNG_HUFFMAN_DYNAMIC) {
    set_error("png_scratch_bytes_huff: huffman %d is neither DVD_PNG_HUFFMAN_FIXED nor DVD_PNG_HUFFMAN_DYNAMIC", huffman);
    return DVD_E_ARG;
  }
  if (!png::shape_ok(h, w)) {
    set_error("png_scratch_bytes_huff: bad shape %dx%d (h >= 1, w >= 1, h * (3 w + 1) < 2^31)", h, w);
    return DVD_E_ARG;
  }
  const png::Layout l = png::layout_of(png::stream_bytes(h, w));
  return (long)(huffman == DVD_PNG_HUFFMAN_DYNAMIC ? l.total_dyn : l.total);
}

// every check comes before the first launch
static int png_encode_args(const char* name, const uint8_t* img_hwc, int h, int w, uint8_t* out, long cap,
                           unsigned long long* out_len, void* scratch) {
  DVD_REQUIRE(img_hwc && out && out_len && scratch, "%s: null pointer", name);
  DVD_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %dx%d (h >= 1, w >= 1)", name, h, w);
  DVD_REQUIRE(png::shape_ok(h, w), "%s: image %dx%d too large (h * (3 w + 1) must be below 2^31)", name, h, w);
  const long bound = png::file_bound(png::stream_bytes(h, w));
  // no kernel can write past the caller's buffer
  DVD_REQUIRE(cap >= bound, "%s: cap %ld below dvd_png_bound(%d, %d) = %ld", name, cap, h, w, bound);
  DVD_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", name);
  return DVD_OK;
}

static int png_encode_launch(const char* name, const uint8_t* img_hwc, int h, int w, uint8_t* out, unsigned long long* out_len,
                             void* scratch, int huffman, void* stream) {
  const long bytes = png::stream_bytes(h, w);
  hipStream_t st = (hipStream_t)stream;
  const int nseg = (int)png::segments(bytes);
  const png::Layout l = png::layout_of(bytes);
  uint8_t* base = (uint8_t*)scratch;
  uint8_t* filt = base + l.filt;
  uint8_t* slots = base + l.slots;
  png::SegMeta* meta = (png::SegMeta*)(base + l.meta);
  unsigned long long* offs = (unsigned long long*)(base + l.offs);
  uint32_t* adler = (uint32_t*)(base + l.adler);
  png::png_filter_kernel<<<h, 256, 0, st>>>(img_hwc, w, filt);
  if (huffman == DVD_PNG_HUFFMAN_DYNAMIC)
    png::png_compress_dyn_kernel<<<nseg, kWave, 0, st>>>(filt, bytes, nseg, slots, (uint16_t*)(base + l.tokens), meta);
  else
    png::png_compress_kernel<<<nseg, kWave, 0, st>>>(filt, bytes, nseg, slots, meta);
  png::png_layout_kernel<<<1, 256, 0, st>>>(meta, nseg, bytes, h, w, offs, adler, out, out_len);
  png::png_gather_kernel<<<nseg, 256, 0, st>>>(slots, meta, offs, adler, nseg, out);
  return check_launch(name);
}

extern "C" int dvd_png_encode_rgb8(const uint8_t* img_hwc, int h, int w, uint8_t* out, long cap, unsigned long long* out_len,
                                   void* scratch, void* stream) {
  const int rc = png_encode_args("png_encode_rgb8", img_hwc, h, w, out, cap, out_len, scratch);
  if (rc != DVD_OK) return rc;
  return png_encode_launch("png_encode_rgb8", img_hwc, h, w, out, out_len, scratch, DVD_PNG_HUFFMAN_FIXED, stream);
}

extern "C" int dvd_png_encode_rgb8_huff(const uint8_t* img_hwc, int h, int w, uint8_t* out, long cap,
                                        unsigned long long* out_len, void* scratch, int huffman, void* stream) {
  DVD_REQUIRE(huffman == DVD_PNG_HUFFMAN_FIXED || huffman == DVD_PNG_HUFFMAN_DYNAMIC,
              "png_encode_rgb8_huff: huffman %d is neither DVD_PNG_HUFFMAN_FIXED nor DVD_PNG_HUFFMAN_DYNAMIC", huffman);
  const int rc = png_encode_args("png_encode_rgb8_huff", img_hwc, h, w, out, cap, out_len, scratch);
  if (rc != DVD_OK) return rc;
  return png_encode_launch("png_encode_rgb8_huff", img_hwc, h, w, out, out_len, scratch, huffman, stream);
}
