// GeoTr (DocTr's geometry transformer; train_settings/models/geotr/geotr_core.py:337-480,496-581,690-742) - the kernels of
// its pre-stage init-flow prior that the conv-net executor (convnet.hip) and the exact-f32 GEMM (gemm.hip) do not cover:
//   flash attention at head_dim 32 in exact f32 (nn.MultiheadAttention's core: q * hd^-0.5, softmax(q k^T), . v),
//   LayerNorm over 256 channels with affine (the post-norms of attnLayer), the positional-embedding add (tgt + pos),
//   a batched [n, a, b] -> [n, b, a] transpose (NCHW maps <-> token rows), the soft document-mask product msk * x
//   (GeoTr_Seg_Inf.forward, geotr_core.py:1007) and the convex upsampling (GeoTr.upsample_flow, :712-723) fused with the
//   sampler hand-off: / 287 and the align_corners bilinear resize to the coordinate grid (evaluation.py:172-178).
// Everything is f32 with fp32 arithmetic: GeoTr's output enters the first denoiser prediction additively.
// Every output element is computed by one thread from its own inputs in a fixed order: a document gives the same bits
// alone and in a batch.
#include "common.h"

namespace dvd {

namespace {

constexpr int HD = 32;          // head_dim of the f32 attention
constexpr int AQ = 64;          // queries per workgroup (one per lane of the single wave)
constexpr int AK = 64;          // keys per LDS tile
constexpr int KPAD = HD + 4;    // K tile row stride in floats (keeps 16-byte rows, spreads the writes over banks)

// O = softmax(scale * Q K^T) V for one (query block, head, batch): lane l owns query row q0 + l, holds its 32 scaled query
// values and 32 accumulators in registers and walks the keys in LDS tiles of 64 (online softmax, one rescale per tile).
// q is scaled BEFORE the dot products, as F.multi_head_attention_forward does (q_scaled = q * sqrt(1 / E)).
__global__ void __launch_bounds__(64) flash_attn_f32_hd32_kernel(const float* __restrict__ Q, int ldq, long sQ,
                                                                 const float* __restrict__ K, int ldk, long sK,
                                                                 const float* __restrict__ Vt, int ldvt, long sVt,
                                                                 float* __restrict__ O, int ldo, long sO, int tq, int tk,
                                                                 int kv_div, float scale) {
  __shared__ float ks[AK * KPAD];
  __shared__ float vs[HD * AK];
  const int lane = threadIdx.x, head = blockIdx.y, b = blockIdx.z, bkv = b / kv_div;
  const int row = blockIdx.x * AQ + lane;
  const int qr = min(row, tq - 1);
  const float* qp = Q + b * sQ + (long)qr * ldq + head * HD;
  float q[HD], acc[HD];
#pragma unroll
  for (int d = 0; d < HD; d += 4) {
    const float4 v = *reinterpret_cast<const float4*>(qp + d);
    q[d] = mul_rn(v.x, scale); q[d + 1] = mul_rn(v.y, scale); q[d + 2] = mul_rn(v.z, scale); q[d + 3] = mul_rn(v.w, scale);
  }
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
  float m = -INFINITY, l = 0.f;
  const float* kb = K + bkv * sK + head * HD;
  const float* vb = Vt + bkv * sVt + (long)head * HD * ldvt;
  for (int k0 = 0; k0 < tk; k0 += AK) {
    __syncthreads();                     // the previous tile is consumed
    {
      const int key = min(k0 + lane, tk - 1);
      const float* kp = kb + (long)key * ldk;
#pragma unroll
      for (int d = 0; d < HD; d += 4) *reinterpret_cast<float4*>(ks + lane * KPAD + d) = *reinterpret_cast<const float4*>(kp + d);
#pragma unroll
      for (int d = 0; d < HD; ++d) vs[d * AK + lane] = vb[(long)d * ldvt + key];
    }
    __syncthreads();
    const int nk = min(AK, tk - k0);
    float s[AK];
    float mt = m;
#pragma unroll
    for (int j = 0; j < AK; ++j) {
      float dot = 0.f;
#pragma unroll
      for (int d = 0; d < HD; d += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(ks + j * KPAD + d);
        dot = fmaf(q[d], kv.x, dot); dot = fmaf(q[d + 1], kv.y, dot);
        dot = fmaf(q[d + 2], kv.z, dot); dot = fmaf(q[d + 3], kv.w, dot);
      }
      s[j] = j < nk ? dot : -INFINITY;
      mt = fmaxf(mt, s[j]);
    }
    const float corr = expf(m - mt);     // m = -inf on the first tile: corr = 0 scales zeros
    l *= corr;
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] *= corr;
#pragma unroll
    for (int j = 0; j < AK; ++j) {
      const float p = expf(s[j] - mt);   // 0 for the masked tail
      l += p;
#pragma unroll
      for (int d = 0; d < HD; ++d) acc[d] = fmaf(p, vs[d * AK + j], acc[d]);
    }
    m = mt;
  }
  if (row >= tq) return;
  float* op = O + b * sO + (long)row * ldo + head * HD;
  const float inv = 1.f / l;
#pragma unroll
  for (int d = 0; d < HD; d += 4)
    *reinterpret_cast<float4*>(op + d) = make_float4(acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv);
}

// nn.LayerNorm(256): one wave per row, 4 channels per lane; biased variance from the centred values, y = (x - mean) * rstd
// * gamma + beta.  Reductions are butterflies over the 64 lanes: a fixed order per row.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) layernorm256_f32_kernel(const float* __restrict__ in, float* __restrict__ out, long rows,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float eps) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float4 x = *reinterpret_cast<const float4*>(in + r * 256 + lane * 4);
  const float mean = wave_sum((x.x + x.y) + (x.z + x.w)) * (1.f / 256.f);
  const float d0 = x.x - mean, d1 = x.y - mean, d2 = x.z - mean, d3 = x.w - mean;
  const float var = wave_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * (1.f / 256.f);
  const float rstd = 1.f / sqrtf(var + eps);
  const float4 g = *reinterpret_cast<const float4*>(gamma + lane * 4), bb = *reinterpret_cast<const float4*>(beta + lane * 4);
  *reinterpret_cast<float4*>(out + r * 256 + lane * 4) =
      make_float4(fmaf(d0 * rstd, g.x, bb.x), fmaf(d1 * rstd, g.y, bb.y), fmaf(d2 * rstd, g.z, bb.z), fmaf(d3 * rstd, g.w, bb.w));
}

// out[r, c] = a[r, c] + pos[r % pos_rows, c]   (attnLayer.with_pos_embed), 4 channels per thread
__global__ void __launch_bounds__(256) add_rows_kernel(const float* __restrict__ a, const float* __restrict__ pos,
                                                       float* __restrict__ out, long rows, int pos_rows, int c4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * c4) return;
  const long r = i / c4;
  const int q = (int)(i - r * c4);
  const float4 x = reinterpret_cast<const float4*>(a)[i];
  const float4 p = reinterpret_cast<const float4*>(pos)[(r % pos_rows) * c4 + q];
  reinterpret_cast<float4*>(out)[i] = make_float4(x.x + p.x, x.y + p.y, x.z + p.z, x.w + p.w);
}

// [n, ra, cb] -> [n, cb, ra] through a 32 x 32 LDS tile (both sides coalesced)
__global__ void __launch_bounds__(256) transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int ra, int cb) {
  __shared__ float t[32][33];
  const long img = blockIdx.z;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  in += img * ra * cb; out += img * ra * cb;
  for (int y = ty; y < 32; y += 8)
    if (r0 + y < ra && c0 + tx < cb) t[y][tx] = in[(long)(r0 + y) * cb + c0 + tx];
  __syncthreads();
  for (int y = ty; y < 32; y += 8)
    if (c0 + y < cb && r0 + tx < ra) out[(long)(c0 + y) * ra + r0 + tx] = t[tx][y];
}

// out[n, ch, p] = m[n, p] * x[n, ch, p]   (x = msk * x, geotr_core.py:1007: the probability itself, no threshold)
__global__ void __launch_bounds__(256) soft_mask_mul_kernel(const float* __restrict__ msk, const float* __restrict__ x,
                                                            float* __restrict__ out, int c, long hw) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long img = blockIdx.y;
  const float m = msk[img * hw + i];
  for (int ch = 0; ch < c; ++ch) out[(img * c + ch) * hw + i] = m * x[(img * c + ch) * hw + i];
}

// One value of GeoTr.upsample_flow(coords1 - coords0, mask) at fine pixel (y, x) of channel ch (geotr_core.py:712-723):
// mask [576, h, w] planar = 0.25 * conv output is folded here (exact: a power of two), softmax over the 9 taps of sub-pixel
// (y % 8, x % 8), then the taps' weighted sum of unfold(8 * flow, 3x3, pad 1).  flow = (coords0 + dflow) - coords0 as
// the reference forms it (coords1 = coords0 + dflow first).
__device__ __forceinline__ float convex_value(const float* __restrict__ mask, const float* __restrict__ dflow, int h, int w,
                                              int ch, int y, int x) {
  const int cy = y >> 3, cx = x >> 3, sub = (y & 7) * 8 + (x & 7);
  const long hw = (long)h * w, at = (long)cy * w + cx;
  float lg[9], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    lg[k] = 0.25f * mask[(k * 64 + sub) * hw + at];
    mx = fmaxf(mx, lg[k]);
  }
  float e[9], sum = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    e[k] = expf(lg[k] - mx);
    sum += e[k];
  }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = cy + k / 3 - 1, xx = cx + k % 3 - 1;
    float f = 0.f;
    if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
      const float base = ch == 0 ? (float)xx : (float)yy;       // coords_grid: channel 0 = x, channel 1 = y
      f = 8.f * sub_rn(add_rn(base, dflow[ch * hw + (long)yy * w + xx]), base);
    }
    acc = add_rn(acc, mul_rn(e[k] / sum, f));
  }
  return acc;
}

// bm [n, 2, 8h, 8w]
__global__ void __launch_bounds__(256) convex_bm_kernel(const float* __restrict__ mask, const float* __restrict__ dflow,
                                                        float* __restrict__ bm, int h, int w, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int W8 = 8 * w, H8 = 8 * h;
  const int x = (int)(i % W8);
  const long q = i / W8;
  const int y = (int)(q % H8);
  const long pl = q / H8;                               // n * 2 + ch
  const long img = pl >> 1;
  const int ch = (int)(pl & 1);
  const long hw = (long)h * w;
  bm[i] = convex_value(mask + img * 576 * hw, dflow + img * 2 * hw, h, w, ch, y, x);
}

// F.interpolate(bm / norm, (g, g), bilinear, align_corners=True) without materialising bm: each output reads its four
// source pixels' convex values (ATen's source index and blend order, as resize_planar_kernel in convnet.hip)
__global__ void __launch_bounds__(256) convex_init_flow_kernel(const float* __restrict__ mask, const float* __restrict__ dflow,
                                                               float* __restrict__ out, int h, int w, int g, float norm,
                                                               long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int gx = (int)(i % g);
  const long q = i / g;
  const int gy = (int)(q % g);
  const long pl = q / g;
  const long img = pl >> 1;
  const int ch = (int)(pl & 1);
  const int H8 = 8 * h, W8 = 8 * w;
  const float sy = g > 1 ? (float)(H8 - 1) / (float)(g - 1) : 0.f, sx = g > 1 ? (float)(W8 - 1) / (float)(g - 1) : 0.f;
  const float fy = sy * (float)gy, fx = sx * (float)gx;
  const int y0 = min((int)fy, H8 - 1), x0 = min((int)fx, W8 - 1), y1 = min(y0 + 1, H8 - 1), x1 = min(x0 + 1, W8 - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
  const long hw = (long)h * w;
  const float* mk = mask + img * 576 * hw;
  const float* df = dflow + img * 2 * hw;
  const float v00 = convex_value(mk, df, h, w, ch, y0, x0) / norm, v01 = convex_value(mk, df, h, w, ch, y0, x1) / norm;
  const float v10 = convex_value(mk, df, h, w, ch, y1, x0) / norm, v11 = convex_value(mk, df, h, w, ch, y1, x1) / norm;
  out[i] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

}  // namespace
}  // namespace dvd

using namespace dvd;

extern "C" int dvd_flash_attn_f32(const dvd_attn_desc* d, void* stream) {
  DVD_REQUIRE(d && d->Q && d->K && d->Vt && d->O, "flash_attn_f32: null pointer");
  DVD_REQUIRE(d->head_dim == HD, "flash_attn_f32: head_dim %d, only 32 is built", d->head_dim);
  DVD_REQUIRE(d->heads > 0 && d->heads <= 65535 && d->batch > 0 && d->batch <= 65535 && d->tq > 0 && d->tk > 0 &&
                  d->kv_batch_div > 0,
              "flash_attn_f32: bad shape");
  DVD_REQUIRE(d->ldq % 4 == 0 && d->ldk % 4 == 0 && d->ldo % 4 == 0 && d->strideQ % 4 == 0 && d->strideK % 4 == 0 &&
                  d->strideO % 4 == 0 && ((uintptr_t)d->Q % 16) == 0 && ((uintptr_t)d->K % 16) == 0 &&
                  ((uintptr_t)d->O % 16) == 0,
              "flash_attn_f32: Q / K / O rows must be 16-byte aligned");
  DVD_REQUIRE(d->ldvt >= d->tk && d->ldq >= d->heads * HD && d->ldk >= d->heads * HD && d->ldo >= d->heads * HD,
              "flash_attn_f32: leading dimensions too small");
  const dim3 grid(cdiv(d->tq, AQ), d->heads, d->batch);
  flash_attn_f32_hd32_kernel<<<grid, 64, 0, (hipStream_t)stream>>>(
      (const float*)d->Q, d->ldq, d->strideQ, (const float*)d->K, d->ldk, d->strideK, (const float*)d->Vt, d->ldvt,
      d->strideVt, (float*)d->O, d->ldo, d->strideO, d->tq, d->tk, d->kv_batch_div, d->scale);
  return check_launch("flash_attn_f32");
}

extern "C" int dvd_layernorm256_f32(const float* in, float* out, long rows, const float* gamma, const float* beta, float eps,
                                    void* stream) {
  DVD_REQUIRE(in && out && gamma && beta, "layernorm256_f32: null pointer");
  DVD_REQUIRE(rows > 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)gamma % 16) == 0 &&
                  ((uintptr_t)beta % 16) == 0,
              "layernorm256_f32: bad rows or unaligned operand");
  layernorm256_f32_kernel<<<cdiv(rows, 4), 256, 0, (hipStream_t)stream>>>(in, out, rows, gamma, beta, eps);
  return check_launch("layernorm256_f32");
}

extern "C" int dvd_add_rows_f32(const float* a, const float* pos, float* out, long rows, int pos_rows, int c, void* stream) {
  DVD_REQUIRE(a && pos && out, "add_rows_f32: null pointer");
  DVD_REQUIRE(rows > 0 && pos_rows > 0 && c > 0 && c % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)pos % 16) == 0 &&
                  ((uintptr_t)out % 16) == 0,
              "add_rows_f32: bad shape or unaligned operand");
  add_rows_kernel<<<cdiv(rows * (c / 4), 256), 256, 0, (hipStream_t)stream>>>(a, pos, out, rows, pos_rows, c / 4);
  return check_launch("add_rows_f32");
}

extern "C" int dvd_transpose_f32(const float* in, float* out, int n, int rows, int cols, void* stream) {
  DVD_REQUIRE(in && out && in != out, "transpose_f32: null or aliased pointer");
  DVD_REQUIRE(n > 0 && n <= 65535 && rows > 0 && cols > 0, "transpose_f32: bad shape");
  transpose_kernel<<<dim3(cdiv(cols, 32), cdiv(rows, 32), n), 256, 0, (hipStream_t)stream>>>(in, out, rows, cols);
  return check_launch("transpose_f32");
}

extern "C" int dvd_soft_mask_mul_batch(const float* msk, const float* x_nchw, float* out_nchw, int n, int c, long hw,
                                       void* stream) {
  DVD_REQUIRE(msk && x_nchw && out_nchw && n > 0 && n <= 65535 && c > 0 && hw > 0, "soft_mask_mul_batch: bad arguments");
  soft_mask_mul_kernel<<<dim3(cdiv(hw, 256), n), 256, 0, (hipStream_t)stream>>>(msk, x_nchw, out_nchw, c, hw);
  return check_launch("soft_mask_mul_batch");
}

extern "C" int dvd_convex_upsample(const float* mask, const float* dflow, int n, int h, int w, float* bm, float* init_flow,
                                   int g, float norm, void* stream) {
  DVD_REQUIRE(mask && dflow && (bm || init_flow), "convex_upsample: null pointer");
  DVD_REQUIRE(n > 0 && h > 0 && w > 0 && (!init_flow || (g > 0 && norm != 0.f)), "convex_upsample: bad shape");
  hipStream_t st = (hipStream_t)stream;
  if (bm) {
    const long total = (long)n * 2 * 64 * h * w;
    convex_bm_kernel<<<cdiv(total, 256), 256, 0, st>>>(mask, dflow, bm, h, w, total);
  }
  if (init_flow) {
    const long total = (long)n * 2 * g * g;
    convex_init_flow_kernel<<<cdiv(total, 256), 256, 0, st>>>(mask, dflow, init_flow, h, w, g, norm, total);
  }
  return check_launch("convex_upsample");
}
