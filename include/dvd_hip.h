/* dvd_hip.h - C ABI of libdvd_hip.so, the MI355X (gfx950) engine for the DvD
 * coordinate-diffusion sampling path.
 *
 * The reference (hanquansanren/DvD) is pure Python on PyTorch and has no FFI of its own;
 * the functions below sit UNDER the Python callables the reference's plug-in surface uses
 *  and each names the reference call site it replaces.  Paths are relative
 * to the reference root; idf/ = train_settings/dvd/improved_diffusion/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions cross the boundary.
 *   - Every function returns 0 on success or a negative DVD_E_* code; dvd_last_error()
 *     returns a thread-local message for the last failure.
 *   - All tensor pointers are BORROWED DEVICE pointers, valid for the duration of the call;
 *     functions only ENQUEUE work on `stream` (a hipStream_t passed as void*) and never
 *     synchronise, allocate or free device memory (workspaces are caller-provided), so every
 *     entry point may be captured into a hipGraph.
 *   - "tok" layouts are token-major [rows, channels] with `ld` = row stride in elements.
 */
#ifndef DVD_HIP_H
#define DVD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVD_OK 0
#define DVD_E_ARG (-1)     /* bad argument (null pointer, unsupported size/alignment) */
#define DVD_E_LAUNCH (-2)  /* HIP reported a launch error */
#define DVD_E_STATE (-3)   /* engine used out of order (weights missing, docs not prepared) */

const char* dvd_last_error(void);
/* library/ABI version: major*1000 + minor */
int dvd_version(void);

/* ------------------------------------------------------------------------------------------
 * Warps
 * ---------------------------------------------------------------------------------------- */

/* Drop-in for register_model2 / SpatialTransformer2.forward
 * (datasets/utils/warping.py:14-23,50-73): F.grid_sample(src, grid.permute(0,2,3,1),
 * mode='bilinear', padding_mode='zeros', align_corners=True).
 * src [N,C,Hin,Win] f32, grid [N,2,H,W] f32 (channel 0 = x, 1 = y, normalised [-1,1]),
 * out [N,C,H,W] f32.  src_batch_div: source image of sample n is n / src_batch_div
 * (1 = reference behaviour; H_hyp lets the hypotheses of one document share one source). */
int dvd_grid_sample_bilinear_zeros_ac(const float* src, const float* grid, float* out,
                                      int n, int c, int hin, int win, int h, int w,
                                      int src_batch_div, void* stream);

/* Fused full-resolution unwarp tail (train_settings/dvd/evaluation.py:301-306 +
 * utils_flow/visualization_utils.py:75-77):
 *   s    = bilinear_upsample(flow[2,G,G] -> H x W, align_corners=True)
 *   grid = ((s + base) * 2 - 1) * scale,  base_x = j/(W-1), base_y = i/(H-1)
 *   out  = grid_sample(src, grid, bilinear, zeros, align_corners=True)
 * f32 variant: src [3,H,W] f32 planar (values 0..255), out [H,W,3] f32 (HWC, what the
 * reference hands to numpy); u8 variant: src [H,W,3] u8, out [H,W,3] u8 with C-style
 * truncation of the f32 result (numpy .astype(uint8) on in-range values). */
int dvd_unwarp_f32(const float* flow, int g, const float* src_chw, float* out_hwc,
                   int h, int w, float scale, void* stream);
int dvd_unwarp_u8(const float* flow, int g, const uint8_t* src_hwc, uint8_t* out_hwc,
                  int h, int w, float scale, void* stream);
/* The same for n documents of one size in ONE launch (flow [n,2,G,G], src / out [n,...] contiguous):
 * the per-document loop of run_evaluation_docunet (evaluation.py:245-306) for a batch of documents. */
int dvd_unwarp_f32_batch(const float* flow, int g, const float* src_chw, float* out_hwc,
                         int n, int h, int w, float scale, void* stream);
int dvd_unwarp_u8_batch(const float* flow, int g, const uint8_t* src_hwc, uint8_t* out_hwc,
                        int n, int h, int w, float scale, void* stream);
/* Documents of DIFFERENT sizes in one launch (real evaluation sets are photographs of many sizes; the reference runs one
 * document at a time, evaluation.py:245-306).  docs is a HOST array of n entries holding DEVICE pointers to separate
 * buffers; it is read during the call only (the table travels as a kernel argument).  At most DVD_RAGGED_CAP documents go
 * into one launch: a larger n is cut into ceil(n / DVD_RAGGED_CAP) launches by the entry point. */
#define DVD_RAGGED_CAP 64
typedef struct {
  const uint8_t* src; /* [h,w,3] uint8 */
  uint8_t* out;       /* [h,w,3] uint8 */
  int h, w;           /* 1 <= h <= 65535, 1 <= w */
} dvd_ragged_image;
/* flow [n,2,G,G]: docs[d].out == dvd_unwarp_u8(flow + d*2*G*G, g, docs[d].src, docs[d].out, h_d, w_d, scale) byte for
 * byte - each document takes the kernel path its own shape takes alone.  src and out of all documents must not overlap. */
int dvd_unwarp_u8_ragged(const float* flow, int g, const dvd_ragged_image* docs, int n, float scale, void* stream);
/* Materialise the full-resolution sampling grid only ([2,H,W] f32), i.e. evaluation.py:301-306. */
int dvd_unwarp_grid(const float* flow, int g, float* grid_out, int h, int w, float scale, void* stream);

/* The same warps with mode='bicubic': F.grid_sample(src, grid, mode='bicubic', padding_mode='zeros',
 * align_corners=True).  Each entry point takes the parameters of its bilinear sibling above.
 *   ix = (gx + 1) * ((Win - 1) / 2) in f32 (the bilinear warps' unnormalisation), fx = floor(ix), tx = ix - fx; y alike.
 *   Taps: columns fx-1 .. fx+2, rows fy-1 .. fy+2.  A tap outside [0,Win) x [0,Hin) contributes 0: zeros padding is per
 *   tap, the coordinate is not clipped.
 *   Weights per axis, A = -0.75: w = [c2(t+1), c1(t), c1(1-t), c2(2-t)] with c1(x) = ((A+2)x - (A+3))x^2 + 1 and
 *   c2(x) = ((Ax - 5A)x + 8A)x - 4A;  out = sum_i sum_j wy[i] wx[j] v[i][j], accumulated in f32 by ONE device function on
 *   every kernel route, so a pixel has the same bits whichever kernel its shape selects.
 *   A non-finite grid value gives NaN in the f32 output and 0 in the u8 output; no grid value makes a kernel read outside
 *   src.
 *   u8 output = (uint8_t)(int)fminf(fmaxf(a, 0), 255): clamped, then truncated - np.clip(a, 0, 255).astype(np.uint8).
 *   Bicubic overshoots (about -56 .. 297 on random bytes), so unlike the bilinear tail the clamp is part of the result.
 * dvd_unwarp_u8_bicubic_batch: the grid of each pixel is dvd_unwarp_grid's, bit for bit; out equals the clamp of
 * dvd_grid_sample_bicubic_zeros_ac on the same image as f32 planes, byte for byte.  dvd_unwarp_u8_bicubic_ragged:
 * docs[d].out == dvd_unwarp_u8_bicubic_batch(flow + d*2*G*G, g, docs[d].src, docs[d].out, 1, h_d, w_d, scale) byte for
 * byte; at most DVD_RAGGED_CAP documents per launch, as dvd_unwarp_u8_ragged. */
int dvd_grid_sample_bicubic_zeros_ac(const float* src, const float* grid, float* out,
                                     int n, int c, int hin, int win, int h, int w,
                                     int src_batch_div, void* stream);
int dvd_unwarp_u8_bicubic_batch(const float* flow, int g, const uint8_t* src_hwc, uint8_t* out_hwc,
                                int n, int h, int w, float scale, void* stream);
int dvd_unwarp_u8_bicubic_ragged(const float* flow, int g, const dvd_ragged_image* docs, int n, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scheduler step (idf/gaussian_diffusion.py:434-438,445-491 ddim_sample; :270-292 posterior
 * mean for the DDPM variant).  One fused elementwise kernel over [n_elem] floats:
 *   DDIM: eps = (c_recip*x_t - x0)/c_recipm1 ; x_prev = x0*sqrt_abar_prev + dir_coef*eps + sigma*noise
 *   DDPM: x_prev = coef1*x0 + coef2*x_t + sigma*noise
 * Coefficients are the float32 casts of the float64 schedule tables (`_extract_into_tensor`,
 * :1181-1197); sigma already contains the (t != 0) mask.  noise may be NULL when sigma == 0.
 * If next_grid != NULL it also receives (x0 + base_G)*2 - 1 ([N,2,G,G], idf/gaussian_diffusion.py:622),
 * the sampling grid of the next step's feature warp. */
typedef struct {
  int kind;             /* 0 = DDIM, 1 = DDPM */
  float c_recip;        /* sqrt(1/abar_t)        DDIM */
  float c_recipm1;      /* sqrt(1/abar_t - 1)    DDIM */
  float sqrt_abar_prev; /* sqrt(abar_{t-1})      DDIM */
  float dir_coef;       /* sqrt(1 - abar_{t-1} - sigma^2) DDIM */
  float coef1;          /* posterior_mean_coef1  DDPM */
  float coef2;          /* posterior_mean_coef2  DDPM */
  float sigma;          /* noise scale incl. (t != 0) mask */
} dvd_sched_coef;

int dvd_sched_step(const dvd_sched_coef* coef, const float* x_t, const float* x0, const float* noise,
                   float* x_prev, float* next_grid, int n, int g, void* stream);

/* The same step behind process_xstart's clamp (idf/gaussian_diffusion.py:380-385, clip_denoised=True), in ONE launch:
 * x0 is clamped to [-1, 1] IN PLACE with torch.clamp's result bit for bit (NaN stays NaN, -0 stays -0) - so the buffer
 * the next denoiser evaluation reads as its init_flow holds pred_xstart - and x_prev / next_grid are computed from the
 * clamped value with dvd_sched_step's arithmetic.  x0 must not alias x_t, noise, x_prev or next_grid. */
int dvd_sched_step_clip(const dvd_sched_coef* coef, const float* x_t, float* x0, const float* noise,
                        float* x_prev, float* next_grid, int n, int g, void* stream);

/* mean over the H hypotheses of each document + clamp to [-1,1]
 * (idf/gaussian_diffusion.py:639-640): x0 [docs*H,2,G,G] -> out [docs,2,G,G]. */
int dvd_hyp_mean_clamp(const float* x0, float* out, int docs, int n_hyp, int g, void* stream);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:  C[M,N] = epi(A[M,K] . B[N,K]^T)  - replaces every nn.Linear / 1x1 conv
 * / patch-embed conv on the path together with the ATen ops that follow it in the reference:
 *   timm Attention.qkv/proj, Mlp.fc1(+GELU tanh)/fc2 (idf/cross_model.py:163-174,268-292),
 *   nn.MultiheadAttention in/out projections (:203-205,237-265), PatchEmbed + pos-embed (:571-605),
 *   decoder linear_q/k/v/fc and conv1/conv2 + folded BatchNorm + ReLU (idf/cross_attn.py:52-57,197-221),
 *   adaLN gate * (.) + residual (idf/cross_model.py:268-292).
 * dtype 0: A,B f16, fp32 accumulate (MFMA 32x32x16 f16);  dtype 1: A,B f32, exact fp32 MFMA.
 *   out = acc (+ bias[col] or bias[row]) -> act -> (+ pos[row % pos_rows][col]) -> (* gate[row / gate_rows][col])
 *         -> (+ res[row][col]);  stored to C32 (f32) and/or C16 (f16).
 * B_lo/lo_scale: weights split into two f16 parts (hi + lo_scale * lo) give fp32-grade weights at twice the MFMA
 * work; used for every per-step weight because f16 weight rounding is a SYSTEMATIC error that accumulates
 * linearly over the diffusion steps (precision).
 * Batched over `batch` with element strides (0 = shared operand).  K % 64 == 0 (f16) / % 16 (f32);
 * rows of A/B 16-byte aligned. */
typedef struct {
  int dtype;
  int M, N, K, batch;
  const void* A; int lda; long strideA;
  const void* B; int ldb; long strideB;
  const void* B_lo; const void* A_lo; float lo_scale; /* optional split weight (f16 only), on ONE side:
                                                          X_true = X + lo_scale * X_lo */
  float* C32; int ldc; long strideC32;
  void* C16; int ldc16; long strideC16;
  const float* bias; int bias_row; long strideBias;
  int act;                                   /* 0 none, 1 GELU(tanh), 2 ReLU */
  const float* pos; int ldpos; int pos_rows;
  const float* gate; int ldgate; int gate_rows; long strideGate;
  const float* res; int ldres; long strideRes;
  int small_tiles;                           /* f16 only: 1 = 128x128 tiles for every shape.  The caller's statement about
                                                its PROBLEM FAMILY (the engine derives 1 from the grid alone): at a few
                                                thousand rows the 256x256 persistent kernels put < 50 workgroups on 256 CUs
                                                and run one workgroup's K loop latency-bound.  2 = the same family with MANY
                                                rows (the engine: >= 16 384 token rows, i.e. the choice between 1 and 2 DOES
                                                depend on the batch): N % 256 == 0 shapes take the 256x256 kernel in the
                                                two-sweep form whose accumulation sequence IS the 128x128 kernel's - the
                                                same bits, which is what keeps 'alone == in a batch' true
                                                (tests/test_gpu_gemm.py::test_gemm_small_family_engine_shapes_same_bits,
                                                tests/test_gpu_engine.py::test_large_batch_of_small_grids_matches_single) */
} dvd_gemm_desc;

int dvd_gemm_nt(const dvd_gemm_desc* desc, void* stream);
/* Name of the kernel instance dvd_gemm_nt launches for a descriptor, demangled as rocprofv3 prints it (e.g.
 * "gemm_nt_t384_kernel<0, 2, true, true>", "gemm_nt_split128_kernel<true>", "gemm_nt_ring256_kernel"); "" for a descriptor
 * dvd_gemm_nt refuses.  Host-only: no device call, so pointers may be any values of the alignment the caller means to test.
 * The returned string stays valid until the calling thread's next call. */
const char* dvd_gemm_kernel_name(const dvd_gemm_desc* desc);

/* ------------------------------------------------------------------------------------------
 * Flash attention core  O = softmax(scale * Q K^T) V  per (batch, head); f16 in/out, fp32 softmax.
 * Replaces the score/softmax/value products inside nn.MultiheadAttention (idf/cross_model.py:237-265),
 * timm Attention (:268-289) and SATRN ScaledDotProductAttention (idf/cross_attn.py:73-83; its
 * all-ones mask is a no-op and dropout is identity in eval mode).
 *   Q  [batch, tq, heads*head_dim]  row stride ldq  (may point into a fused qkv buffer)
 *   K  [kv_batch, tk, heads*head_dim] row stride ldk
 *   Vt [kv_batch, heads*head_dim, tk] row stride ldvt  (V TRANSPOSED: keys contiguous)
 *   O  [batch, tq, heads*head_dim]  row stride ldo
 * kv batch of query batch b is b / kv_batch_div (hypotheses of one document share its conditioning
 * K/V).  head_dim in {64, 256}; tk % 8 == 0.  (head_dim 32 runs in f32: dvd_flash_attn_f32.) */
typedef struct {
  int head_dim, heads, batch, tq, tk, kv_batch_div;
  const void* Q; int ldq; long strideQ;
  const void* K; int ldk; long strideK;
  const void* Vt; int ldvt; long strideVt;
  void* O; int ldo; long strideO;
  float scale;
} dvd_attn_desc;

int dvd_flash_attn(const dvd_attn_desc* desc, void* stream);
/* Name of the kernel dvd_flash_attn launches for a problem shape (the choice depends on head_dim, tq and tk only -
 * never on the batch or the environment).  Measurement tooling matches rocprofv3 / PMC records against it.  head_dim 32
 * names the kernel of dvd_flash_attn_f32. */
const char* dvd_flash_attn_kernel_name(int head_dim, int tq, int tk);

/* ------------------------------------------------------------------------------------------
 * Token-side kernels (each also reachable on its own for parity tests).  "rows" = tokens of all
 * samples, token-major; f16 outputs feed the GEMM / attention operands.
 * ---------------------------------------------------------------------------------------- */

/* obs_embedder (PatchEmbed k=s=2, 2->384) + bias + pos-embed, and cross_norm LayerNorm (no affine,
 * eps 1e-6) of the result (idf/cross_model.py:571,238).  x [N,2,G,G]; w [384,8]; pos [T,384];
 * tok32 [N*T,384] f32; ln16 [N*T,384] f16. */
int dvd_embed_obs_ln(const float* x, const float* w, const float* bias, const float* pos, float* tok32,
                     void* ln16, int n, int g, void* stream);

/* LayerNorm over c in {384,1536} channels (+affine gamma/beta) (+adaLN modulate y*(1+scale)+shift with
 * row / mod_rows selecting the modulation row) -> f16.  nn.LayerNorm + modulate() call sites:
 * idf/cross_model.py:13-14,268-292; idf/cross_attn.py:386-391.  Batched over `batch` slices. */
int dvd_layernorm_rows(const float* in, int ldin, long stride_in, void* out16, int ldout, long stride_out,
                       int batch, long rows, int c, const float* gamma, const float* beta, const float* shift,
                       const float* scale, int ldmod, int mod_rows, float eps, void* stream);

/* Rows of the r_embedder GEMM: per token and 2x2 patch position the 258 channels
 * cat([init_flow, init_feat]) (idf/cross_model.py:596-603) where init_feat is, by `mode`,
 * 0: zeros, 1: feat itself (t > 600), 2: bilinear warp of feat by (init_flow + base)*2-1
 * (idf/gaussian_diffusion.py:618-624), 3: the explicit tensor init_feat_nchw [N,256,G,G].
 * feat is channels-last [docs,G,G,256]; out f16 [N*T, ldo>=1032]. */
int dvd_build_r_rows(const float* feat_nhwc, const float* init_feat_nchw, const float* flow, void* out16, int ldo,
                     int n, int g, int n_hyp, int mode, void* stream);

/* 2x2 patch rows of a map with arbitrary element strides (PatchEmbed operand, idf/cross_model.py:585,594,605):
 * out[(n*T+t)*ldo + (p*2+q)*c + ch] = in[n*sn + ch*sc + (2ty+p)*sy + (2tx+q)*sx]. */
int dvd_patch_rows(const float* in, long sn, long sc, long sy, long sx, float* out, int ldo, int n, int c, int g,
                   void* stream);

/* Depthwise 3x3 (pad 1) + folded eval-mode BatchNorm + ReLU on the side x side token grid
 * (LocalityAwareFeedforward.depthwise_conv, idf/cross_attn.py:33-41,54).  f16 [n*side*side, c]; w [9,c]. */
int dvd_dwconv3x3(const void* in16, void* out16, const float* w9c, const float* b, int n, int side, int c,
                  void* stream);

/* Adaptive2DPositionalEncoding (idf/cross_attn.py:143-157): token mean per sample (deterministic two-stage),
 * then z += hs[n,c]*htab[ty,c] + ws[n,c]*wtab[tx,c]. */
int dvd_colmean(const float* z, float* partial, float* pooled, int n, int t, int c, int chunks, void* stream);
int dvd_posenc_add(float* z, const float* hs, const float* ws, const float* htab, const float* wtab, int n, int side,
                   int c, void* stream);

/* Tiny-M linear y = act_out(W . act_in(x) + b): TimestepEmbedder (act_in 2 = sinusoid of x[m], idf/cross_model.py:111-139),
 * adaLN_modulation (act_in 1 = SiLU, :175-177,325-327, kmod tiles the input: t.repeat(1,4) :331), pos-enc scale MLPs
 * (act_out 2 ReLU / 3 sigmoid, idf/cross_attn.py:136-141). */
int dvd_small_linear(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int m, int k, int n,
                     int kmod, int act_in, int act_out, void* stream);

/* decoder.layer_norm + FinalLayer2 + unpatchify + init_flow (idf/cross_attn.py:457; idf/cross_model.py:329-336,
 * 553-566,645-646).  z [N*T,1536]; x0 [N,2,G,G]; tok8 (optional) [N*T,8]. */
int dvd_final_tokens(const float* z, const float* gamma, const float* beta, const float* shift, const float* scale,
                     int ldmod, int mod_rows, const float* w8, const float* b8, const float* init_flow, float* x0,
                     float* tok8, int n, int g, void* stream);

/* Conv pyramid pieces (idf/cross_model.py:18-95), channels-last f32. */
int dvd_im2col3x3(const float* in, long sc, long sy, long sx, float* out, int ldo, int c, int h, int w, void* stream);
/* 3x3 / pad 1 / stride 1 convolution + bias (+ReLU when relu != 0) of a channels-last map in [h, w, c], c % 16 == 0, as an
 * implicit GEMM: the arithmetic of dvd_im2col3x3 + dvd_gemm_nt (f32) on weights wgt [cout, kp] (K order tap-major; kp >= 9 c
 * for cout <= 64, kp == 9 c above) - same K-tiles, same MFMA sequence, same bits - without the [h w, kp] matrix.  At most 64
 * output channels: operands straight to registers (conv_f32_narrow_kernel); more: the exact-f32 128 x 128 GEMM gathering its
 * A tiles from the map (gemm_nt_kernel<f32, CONV>). */
int dvd_conv3x3_nhwc(const float* in, int c, const float* wgt, int kp, const float* bias, float* out, int cout, int h, int w,
                     int relu, void* stream);
int dvd_maxpool2_nhwc(const float* in, float* out, int c, int h, int w, void* stream);
int dvd_resize_bilinear_nhwc(const float* in, float* out, int c, int hin, int win, int hout, int wout, void* stream);
int dvd_nhwc_to_nchw(const float* in, float* out, int c, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pre-stage conditioning nets: the U2NETP document-mask nets and the text-line
 * UNet that produce mask_cat / mask_y512 / line_msk once per document, before the diffusion loop
 * (train_settings/dvd/evaluation.py:162-216; train_settings/models/geotr/geotr_core.py:24-46,48-330,
 * 745-845,984-1019; unet_model.py:4-37; unet_parts.py:8-77).
 * A net is a flat list of ops over numbered activation slots (slot 0 = the input); the host builds the
 * list from the architecture and packs the weights (eval-mode BatchNorm folded into conv weight + bias,
 * conv weight as [cout, kpad] with K order (ky*ks+kx)*cin + c, kpad = ks*ks*cin rounded up to 16,
 * followed by the bias [cout] padded to a multiple of 4 floats; convs packed in op order).  Activations are channels-last f32; convs run
 * on the exact-f32 MFMA GEMM. */
enum { DVD_CN_CONV = 0, DVD_CN_POOL = 1, DVD_CN_RESIZE = 2, DVD_CN_ADD = 3, DVD_CN_SIGMOID = 4, DVD_CN_INSTNORM = 5 };
typedef struct {
  int op;           /* DVD_CN_* */
  int a, b;         /* input slots; b = -1 when unused.  conv: b is concatenated after a along channels
                       (torch.cat((a, b), 1)); add: second operand; resize: the slot whose size is the target */
  int dst;          /* output slot (each slot is written once) */
  int ks, dil;      /* conv: kernel size 1, 3 or 7, dilation (padding = dil * (ks / 2)) */
  int cout, act;    /* conv: output channels; act 0 none, 2 ReLU - also for add (relu(a + b)) and instnorm */
  long w_off;       /* conv: offset, in floats, of this conv's [cout, kpad] weights (+ bias) in the blob */
  int h, w;         /* resize with b = -1: explicit target size */
  int flag;         /* resize: align_corners; pool: ceil_mode; conv: stride (0 or 1 = stride 1; 2 = stride 2, single
                       source) */
} dvd_cn_op;
/* DVD_CN_INSTNORM: nn.InstanceNorm2d without affine parameters (per image and channel over h*w, biased variance,
 * eps 1e-5; extractor.py:31-35,62-63), then ReLU when act == 2. */

int dvd_convnet_create(const dvd_cn_op* ops, int n_ops, int n_slots, int in_c, int in_h, int in_w, void** handle);
/* The same net for `batch` images per run (the documents of a batch, evaluation.py:162-216 is called per document in the
 * reference): every op is ONE launch over all images (a conv's GEMM has M = batch * h * w rows).  Kernel choices depend on
 * the per-image shape only: an image gives the same bits alone or in a batch. */
int dvd_convnet_create_batched(const dvd_cn_op* ops, int n_ops, int n_slots, int in_c, int in_h, int in_w, int batch,
                               void** handle);
int dvd_convnet_destroy(void* handle);
long dvd_convnet_workspace_bytes(void* handle);
long dvd_convnet_weight_floats(void* handle);
int dvd_convnet_slot_shape(void* handle, int slot, int* h, int* w, int* c);
/* The route dvd_convnet_run takes for op `op` of the list, decided once in dvd_convnet_create from the shapes alone
 * (host-only; tests assert it so that a case written for one kernel cannot silently move to another):
 *   NARROW1    conv_f32_narrow_kernel<1>, one column group       (cout <= 32, sources 8-aligned, their sum 16-aligned)
 *   NARROW1X2  conv_f32_narrow_kernel<1>, two column groups      (cout 33..64, fewer than 16384 rows in the batch)
 *   NARROW2    conv_f32_narrow_kernel<2>                         (cout 33..64, at least 16384 rows)
 *   WIDE       the 128 x 128 GEMM gathering its A tiles itself   (cout > 64, sources 16-aligned, no split-K, not a
 *                                                                 single-source 1x1)
 *   DIRECT     the GEMM reads a 1x1 conv's single 16-aligned source in place
 *   GATHER     im2col matrix + GEMM (everything else at stride 1)
 *   STRIDED    im2col matrix of the output pixels + GEMM (stride 2)
 * *ksplit: the number of K slices (1 = none; > 1 only with GATHER and DIRECT: S partial GEMMs, then a reduction in slice
 * order).  Ops that are no conv report NONE and 1. */
enum { DVD_CN_PATH_NONE = 0, DVD_CN_PATH_NARROW1 = 1, DVD_CN_PATH_NARROW1X2 = 2, DVD_CN_PATH_NARROW2 = 3,
       DVD_CN_PATH_WIDE = 4, DVD_CN_PATH_DIRECT = 5, DVD_CN_PATH_GATHER = 6, DVD_CN_PATH_STRIDED = 7 };
int dvd_convnet_op_info(void* handle, int op, int* path, int* ksplit);
/* One forward pass: in_nchw [batch, in_c, in_h, in_w] f32 planar (batch = 1 for dvd_convnet_create); the requested slots
 * are written to out_nchw[k] as planar [batch, c, h, w].  workspace: >= dvd_convnet_workspace_bytes, 256-byte aligned. */
int dvd_convnet_run(void* handle, const float* in_nchw, const float* weights, void* workspace, long workspace_bytes,
                    int n_out, const int* out_slots, float* const* out_nchw, void* stream);
/* F.interpolate(mode='bilinear', align_corners=...) on `planes` independent [hin, win] f32 images
 * (evaluation.py:162,199-204,210; geotr_core.py:992,1010). */
int dvd_resize_bilinear_nchw(const float* in, float* out, long planes, int hin, int win, int hout, int wout,
                             int align_corners, void* stream);
/* mskx = (d0 > thr).float() * x  (Seg.forward, geotr_core.py:989-990): d0 [hw], x / out [c, hw];
 * mask_out (optional) receives the 0/1 mask. */
int dvd_threshold_mask_mul(const float* d0, const float* x_nchw, float* out_nchw, float* mask_out, int c, long hw,
                           float thr, void* stream);
/* the same for n images in one launch: d0 [n, hw], x / out [n, c, hw], mask_out [n, hw] */
int dvd_threshold_mask_mul_batch(const float* d0, const float* x_nchw, float* out_nchw, float* mask_out, int n, int c,
                                 long hw, float thr, void* stream);

/* ------------------------------------------------------------------------------------------
 * GeoTr, DocTr's geometry transformer (the init-flow prior of env.use_init_flow; train_settings/models/geotr/
 * geotr_core.py:337-480,496-581,690-742, evaluation.py:172-178).  Its convolutions run on the conv-net executor above,
 * its projections and FFNs on dvd_gemm_nt dtype 1; these are the remaining pieces, all exact f32.
 * Attention core at head_dim 32 on f32 operands (dvd_attn_desc as for dvd_flash_attn; Q, K, Vt, O point to floats):
 * O = softmax(scale * Q K^T) V, q scaled before the products as nn.MultiheadAttention does. */
int dvd_flash_attn_f32(const dvd_attn_desc* desc, void* stream);
/* nn.LayerNorm(256) with affine over `rows` contiguous rows: out = (x - mean) / sqrt(var + eps) * gamma + beta. */
int dvd_layernorm256_f32(const float* in, float* out, long rows, const float* gamma, const float* beta, float eps,
                         void* stream);
/* out[r, c] = a[r, c] + pos[r % pos_rows, c] (c % 4 == 0). */
int dvd_add_rows_f32(const float* a, const float* pos, float* out, long rows, int pos_rows, int c, void* stream);
/* [n, rows, cols] -> [n, cols, rows]. */
int dvd_transpose_f32(const float* in, float* out, int n, int rows, int cols, void* stream);
/* out = msk * x with a [n, hw] soft mask (no threshold; GeoTr_Seg_Inf.forward, geotr_core.py:1007); x / out [n, c, hw]. */
int dvd_soft_mask_mul_batch(const float* msk, const float* x_nchw, float* out_nchw, int n, int c, long hw, void* stream);
/* GeoTr.upsample_flow(coords1 - coords0, 0.25 * mask): mask [n, 576, h, w] (the mask head's raw conv output), dflow
 * [n, 2, h, w].  bm (optional) [n, 2, 8h, 8w]; init_flow (optional) [n, 2, g, g] = F.interpolate(bm / norm, g, bilinear,
 * align_corners=True) computed without materialising bm. */
int dvd_convex_upsample(const float* mask, const float* dflow, int n, int h, int w, float* bm, float* init_flow, int g,
                        float norm, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image ingest (datasets/doc_dataset/doc_benchmark.py:75-97 after the decode):
 *   y = cv2.resize(rgb, (out, out)) / 255.  as planar f32 [3,out,out]  (OpenCV 8-bit INTER_LINEAR fixed point),
 *   rgb_hwc_out (optional) = the full-resolution image in RGB order (what the unwarp tail samples).
 * src_hwc [h,w,3] uint8 on the device; swap_rb: the source is BGR (cv2.imread order).
 * scratch: dvd_ingest_scratch_bytes(out_size) device bytes. */
long dvd_ingest_scratch_bytes(int out_size);
int dvd_ingest_u8(const uint8_t* src_hwc, int h, int w, int swap_rb, float* y_chw, int out_size,
                  uint8_t* rgb_hwc_out, void* scratch, void* stream);

/* The same for n images of n sizes in at most three launches (axis tables, resize, RGB copies): y_nchw [n,3,out,out],
 * y_nchw[d] == dvd_ingest_u8(docs[d].src, ...) bit for bit.  docs[d].out (optional; may equal src when swap_rb == 0, which
 * copies nothing) receives the full-resolution image in RGB order.  scratch: dvd_ingest_ragged_scratch_bytes(out_size, n)
 * device bytes.  n above DVD_RAGGED_CAP is cut into several launches per stage. */
long dvd_ingest_ragged_scratch_bytes(int out_size, int n);
int dvd_ingest_u8_ragged(const dvd_ragged_image* docs, int n, int swap_rb, float* y_nchw, int out_size, void* scratch,
                         void* stream);

/* Temporal dithering of the f16 weight rounding (no reference counterpart: the reference is fp32; the GEMMs that consume
 * the result are the per-step nn.Linear / 1x1 convs, idf/cross_attn.py:197-221,52-57, idf/cross_model.py:163-174).
 * hi, lo [nelem] f16 with W = hi + lo (hi = round-to-nearest f16 of W); out [nelem] f16 = W re-rounded to one of its two
 * f16 neighbours so that the MEAN over consecutive `step`s is W: up iff hash(elem0 + i) + step * 2^32/phi (mod 2^32) <
 * 2^32 * (W - down)/(up - down).  nelem % 8 == 0, 16-byte aligned.  The engine calls it before each evaluation when
 * its "dither" option is on. */
int dvd_dither_f16(const void* hi, const void* lo, void* out, long nelem, unsigned elem0, unsigned step, void* stream);

/* ------------------------------------------------------------------------------------------
 * Engine: DiT.forward of the live model (idf/cross_model.py:568-647) for docs x n_hyp samples.
 *   create -> workspace_bytes -> bind_workspace -> set_tensor(every tensor of tensor_info) ->
 *   prepare_docs (once per batch of documents) -> denoise_step (once per diffusion step).
 * The engine owns no device memory.  Tensor names/sizes are enumerated by tensor_info; the host-side
 * packer (dvd_amd/weights.py) derives them from a reference-named state_dict (model1852000.pt keys).
 * ---------------------------------------------------------------------------------------- */
int dvd_engine_create(int grid, int docs, int n_hyp, void** handle);
int dvd_engine_destroy(void* handle);
long dvd_engine_workspace_bytes(void* handle);
int dvd_engine_bind_workspace(void* handle, void* workspace, long bytes);
int dvd_engine_tensor_count(void* handle);
int dvd_engine_tensor_info(void* handle, int index, const char** name, int* dtype /*0 f32, 1 f16*/, long* nelem);
int dvd_engine_set_tensor(void* handle, const char* name, const void* dev_ptr, long nelem);
/* options (per handle; no environment variable is read anywhere in the library):
 *   "split_weights" (default 1): use the (hi, lo) f16 weight pairs -> fp32-grade weights, 2x GEMM MFMAs;
 *   "dither"        (default: 1 when the grid takes the 256-wide GEMM kernels, i.e. grid >= 66, else 0): the weights of
 *                                the 256-wide per-step GEMMs are re-rounded to ONE f16 before every evaluation with a
 *                                step-dependent sub-ulp offset (dvd_dither_f16: zero-mean over the steps) and those
 *                                GEMMs run one pass - half the MFMAs of the split; the other GEMMs keep the (hi, lo) pair
 *                                (no effect on small-tile grids, which keep the pair everywhere);
 *   "dither_step"  (default 0) : the dithering phase of every following denoise_step until it is set again.  The engine keeps
 *                                NO running counter: an evaluation is a pure function of its inputs and the handle's
 *                                options (the reference's model() is pure, idf/cross_model.py:568-647).  A roll-out sets it
 *                                to its loop index (0 at the first step: S-1-i at timestep index i) before every
 *                                evaluation, which is what makes the rounding zero-mean over the steps; left constant the
 *                                evaluations are still correct, each with plain f16 weight rounding;
 *   "ffn_lo"        (default 1): 0 drops the lo pass of the decoder FFN's two 1x1 convs only (-4.8 % step time;
 *                                measured coordinate error on synthetic weights 1.2e-4 -> 3.3e-4: opt-in);
 *   "graphs"        (default 0): replay each denoiser evaluation as a captured hipGraph (bit-identical results;
 *                                the Python engine turns it on for grids <= 128);
 *   "small_tiles"   (default: 1 when (grid/2)^2 <= 1024 tokens, i.e. grid <= 64, else 0): 128x128 GEMM tiles for
 *                                the per-step GEMMs - a function of the grid only, so a document takes the same kernels
 *                                and the same summation order alone or in a batch. */
int dvd_engine_set_option(void* handle, const char* name, int value);
/* y512 [docs,3,512,512] (0..1), mask_cat [docs,1,512,512], mask_y512 [docs,384,G,G], line_msk [docs,64,G,G]
 * (kwargs of the denoiser call, train_settings/dvd/evaluation.py:106-115). */
int dvd_engine_prepare_docs(void* handle, const float* y512, const float* mask_cat, const float* mask_y512,
                            const float* line_msk, void* stream);
/* feat as the reference returns it: [docs,256,G,G] (idf/cross_model.py:647). */
int dvd_engine_feat_nchw(void* handle, float* out, void* stream);
/* x_t, init_flow, x0_out [N,2,G,G].  t_embed = value fed to the timestep embedder after the override rule
 * (idf/cross_model.py:575-580); feat_mode as in dvd_build_r_rows. */
int dvd_engine_denoise_step(void* handle, const float* x_t, float t_embed, int feat_mode, const float* init_flow,
                            const float* init_feat_nchw /* feat_mode 3 only, else NULL */, float* x0_out, void* stream);
/* Per-launch timing of the dominant kernel (the head_dim-256 decoder attention) with HIP events recorded on
 * the launch stream: profile(1) arms it, profile_read returns the number of timed launches and their summed
 * duration since the last read (synchronises on the events).  Used by bench.py's roofline leg. */
int dvd_engine_profile(void* handle, int enable);
int dvd_engine_profile_read(void* handle, int* launches, double* total_ms);
/* Internal activation buffers by name (parity tests only); debug_stop makes denoise_step return after
 * stage k: 1 cross-attention streams, 2 DiT block, 3 decoder pos-enc, 4+j decoder layer j (0 = run all). */
int dvd_engine_debug_buffer(void* handle, const char* name, void** ptr, long* bytes);
int dvd_engine_debug_stop(void* handle, int stage);

/* ------------------------------------------------------------------------------------------
 * Hardware self-test of the MFMA fragment layouts the kernels rely on (exact integer data).
 * a16 [32,16], b16 [16,32], vt16 [32,32] f16; out [3072] f32 = {A.B, Vt.(A.B) via accumulator-as-
 * operand, f32-MFMA A[:, :2].B[:2, :]}.  No reference counterpart (test infrastructure). */
int dvd_selftest_mfma(const void* a16, const void* b16, const void* vt16, float* out3072, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image-quality metric of the evaluation tail: MS-SSIM of a dewarped page against its flat ground-truth scan.  The
 * reference leaves it to offline MATLAB (matlab_code/run_docunet.m, whose evalUnwarp is not in its tree); the definition
 * is this project's own (float64 statement: tests/msssim_model.py) and parity with MATLAB's imresize /
 * rgb2gray / ssim / impyramid is UNPINNED.  No kernel uses an atomic: the same inputs give the same bits on every launch,
 * and document d of a batch gets the bits it gets alone.
 * ---------------------------------------------------------------------------------------- */
#define DVD_SSIM_REPLICATE 0 /* window centred, indices clamped: the map is h x w */
#define DVD_SSIM_VALID 1     /* full windows only: the map is (h-10) x (w-10) */
#define DVD_MSSSIM_DOCUNET 0 /* replicate border, [1,4,6,4,1]/16 reduce */
#define DVD_MSSSIM_WANG 1    /* valid border, 2-tap box reduce */
/* Fused preparation: src [n,h,w,3] u8 RGB -> out [n,out_h,out_w] f32 gray (integer values 0..255).  Separable anti-aliased
 * triangle resize (per axis r = out/in, centre u = (o+0.5)/r - 0.5, taps j = ceil(u - 1/s) .. floor(u + 1/s) with
 * s = min(r,1), weight tri((u-j) s), tap indices clamped, weights normalised to sum 1; f64 taps and sums), rounded half
 * to even to u8 once, then gray = round(0.2989 R + 0.5870 G + 0.1140 B).  The tap tables are built on the device in
 * `scratch` (dvd_resize_gray_scratch_bytes; a negative DVD_E_* value for a bad shape).  Every side 1..32768. */
long dvd_resize_gray_scratch_bytes(int h, int w, int out_h, int out_w);
int dvd_resize_gray_u8(const uint8_t* src_nhwc, int n, int h, int w, float* out, int out_h, int out_w,
                       void* scratch, void* stream);
/* One scale on gray planes x, y [n,h,w] f32 (values 0..255, each side 11..32768): the 11-tap Gaussian (sigma 1.5) moments
 * mu_x, mu_y, E[xx], E[yy], E[xy] of both planes less 127.5, cs = (2 s_xy + C2) / (s_xx + s_yy + C2) and
 * ssim = cs (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1), C1 = 6.5025, C2 = 58.5225.  partials [n, tiles, 2] f64 receives
 * (sum ssim, sum cs) of every 32 x 32 tile of the map, tiles = ceil(map_h / 32) * ceil(map_w / 32), row-major. */
int dvd_ssim_scale(const float* x, const float* y, int n, int h, int w, int border, double* partials, void* stream);
/* out[d, scale, 0..1] = (sum ssim, sum cs) of document d's tiles, added in a fixed order in f64, / count (the map's
 * pixels); out is [n,5,2] f32, scale 0..4. */
int dvd_ssim_finalize(const double* partials, int n, int tiles, long count, float* out_n52, int scale, void* stream);
/* Both planes [n,h,w] reduced by 2 to [n,ceil(h/2),ceil(w/2)] in one launch.  taps 2: out[i] = (x[2i] + x[min(2i+1,
 * n-1)]) / 2 per axis; taps 5: [1,4,6,4,1]/16 centred on 2i, indices clamped. */
int dvd_reduce2_pair(const float* x, const float* y, float* x_out, float* y_out, int n, int h, int w, int taps,
                     void* stream);
/* The five scales of n pairs of planes [n,h,w] (each side 176..32768, so that the fifth scale holds one full window):
 * out [n,5,2] f32 = per scale (mean ssim, mean cs).  workspace: dvd_msssim_workspace_bytes(h, w, n) bytes (tile partials
 * and the planes of scales 2..5; a negative DVD_E_* value for a bad shape or batch). */
long dvd_msssim_workspace_bytes(int h, int w, int n);
int dvd_msssim_scales(const float* x, const float* y, int n, int h, int w, int preset, void* workspace,
                      float* out_n52, void* stream);

/* ------------------------------------------------------------------------------------------
 * Lossless PNG of a dewarped page, encoded where the unwarp tail leaves it (the reference: Image.fromarray(...).save on
 * the host, utils_flow/visualization_utils.py:77-78).  The file is a pure function of (h, w, pixels) - DESIGN.md 4.4:
 *   signature, IHDR (w, h, depth 8, colour type 2, 0, 0, 0), one IDAT per segment, IEND.
 *   Filtered stream: h rows of 1 + 3w bytes; per row the filter None / Sub / Up / Average / Paeth with the least sum of
 *   |residual as a signed byte|, the lowest number on a tie.
 *   The stream is cut into segments of DVD_PNG_SEGMENT bytes (not tied to rows).  Each is compressed on its own: greedy LZ77
 *   (length 3..258, matches never reach before the segment's first byte or past its last), ONE fixed-Huffman block
 *   (BFINAL = 0), then an empty stored block (00 00 FF FF after padding to a byte), so the segments' bytes concatenate.
 *   The zlib stream is 78 01, the segments, the final empty fixed block 03 00 and the big-endian Adler-32 of the filtered
 *   stream (per-segment partials folded exactly mod 65521).  IDAT s holds segment s; the first also the two header bytes,
 *   the last also 03 00 and the Adler-32.  Each IDAT's CRC-32 covers that chunk only.
 * DVD_PNG_HUFFMAN_DYNAMIC changes the segment's block alone; filter choice, segmentation, the LZ77 tokens and the rest of
 * the container are the above.  Per segment: the histograms of the 286 literal/length symbols (one end-of-block included)
 * and the 30 distance symbols; for each a prefix code limited to 15 bits (lengths by Huffman on the symbols sorted by
 * (frequency, symbol); if the deepest leaf is beyond the limit, depths are clamped, the rarest symbols of the greatest depth
 * below the limit go down until the Kraft sum is at most 1, then symbols from the most frequent to the rarest come up one
 * level per pass while the gain fits, so the code is complete - DESIGN.md 4.4), codes canonical (RFC 1951 3.2.2).  No match
 * in the segment: HDIST = 1 with the single length 0; one used distance symbol: length 1.  Header: HLIT / HDIST trimmed of
 * trailing zeros (at least 257 / 1); the concatenated lengths run-length coded greedily (a zero run: 18s of up to 138, one 17
 * for 3..10, single zeros; another length: once, 16s of up to 6, single lengths); their code limited to 7 bits, a second
 * symbol given length 1 if only one is used; HCLEN trimmed in the permuted order (at least 4).  The exact bits of the dynamic
 * block (3 + header + tokens + end-of-block) and of the fixed block are computed from the histograms, and the dynamic block
 * is written only if it is strictly smaller: a segment, and so a file, is never longer than DVD_PNG_HUFFMAN_FIXED's, and
 * dvd_png_bound holds for both.
 * ---------------------------------------------------------------------------------------- */
#define DVD_PNG_SEGMENT 32768
#define DVD_PNG_HUFFMAN_FIXED 0
#define DVD_PNG_HUFFMAN_DYNAMIC 1
/* Worst-case file bytes and scratch bytes for an h x w image; host-only.  A negative DVD_E_* value for a bad shape
 * (h < 1, w < 1 or h * (3w + 1) >= 2^31). */
long dvd_png_bound(int h, int w);
long dvd_png_scratch_bytes(int h, int w);
/* img_hwc [h,w,3] u8 -> the complete file in out[0 .. *out_len), *out_len (a DEVICE uint64) <= dvd_png_bound(h, w).
 * cap = bytes writable at out: cap < dvd_png_bound(h, w) is DVD_E_ARG, checked before anything is launched, so no kernel
 * can write past out + cap.  scratch: dvd_png_scratch_bytes(h, w) device bytes, 16-byte aligned; its previous contents
 * do not matter.  Four launches on `stream`, no synchronisation, no read-back. */
int dvd_png_encode_rgb8(const uint8_t* img_hwc, int h, int w, uint8_t* out, long cap, unsigned long long* out_len,
                        void* scratch, void* stream);
/* The same with the block type chosen: huffman = DVD_PNG_HUFFMAN_FIXED is dvd_png_encode_rgb8 byte for byte,
 * DVD_PNG_HUFFMAN_DYNAMIC writes per segment the smaller of a dynamic and the fixed block; any other value is DVD_E_ARG,
 * checked before anything is launched.  scratch: dvd_png_scratch_bytes_huff(h, w, huffman) bytes (FIXED: what
 * dvd_png_scratch_bytes returns; DYNAMIC: 2 more bytes per stream byte for the tokens). */
long dvd_png_scratch_bytes_huff(int h, int w, int huffman);
int dvd_png_encode_rgb8_huff(const uint8_t* img_hwc, int h, int w, uint8_t* out, long cap, unsigned long long* out_len,
                             void* scratch, int huffman, void* stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG of a dewarped page, encoded where the unwarp tail leaves it.  The file is a pure function of (h, w, pixels,
 * quality, subsampling), integer arithmetic throughout - DESIGN.md 4.5:
 *   SOI, APP0 (JFIF 1.01), DQT (the Annex K.1 tables scaled by the usual quality rule), SOF0 (8 bit, Y Cb Cr), DHT (the four
 *   Annex K.3 tables), DRI, SOS, the entropy-coded data, EOI.
 *   One restart interval per MCU row (MCU 16 x 16 pixels in 4:2:0, 8 x 8 in 4:4:4): every interval starts with DC predictors
 *   0, ends padded with 1-bits to a byte and is followed by RSTm, m = interval mod 8 (the last by EOI).
 *   Pixels past the image repeat its last row / column.  RGB -> YCbCr in 16-bit fixed point, 4:2:0 chroma = the 2 x 2 average
 *   (a + b + c + d + 2) >> 2, DCT by the integer matrix round(2^13 C(u)/2 cos((2x+1) u pi/16)) (rows keep 2 fraction bits, the
 *   coefficient 3), quantisation by division rounded half away from zero.
 * ---------------------------------------------------------------------------------------- */
#define DVD_JPEG_420 0
#define DVD_JPEG_444 1
/* Worst-case file bytes and scratch bytes for an h x w image; host-only.  A negative DVD_E_* value for a bad shape (h or w
 * outside 1..65535, or 3 * h * w at 16-pixel granularity >= 2^31) or an unknown subsampling. */
long dvd_jpeg_bound(int h, int w, int subsampling);
long dvd_jpeg_scratch_bytes(int h, int w, int subsampling);
/* img_hwc [h,w,3] u8 (any byte alignment) -> the complete file in out[0 .. *out_len), *out_len (a DEVICE uint64) <=
 * dvd_jpeg_bound(h, w, subsampling).  quality 1..100.  cap = bytes writable at out: cap below the bound is DVD_E_ARG,
 * checked like every other argument before anything is launched, so no kernel can write past out + cap.  scratch:
 * dvd_jpeg_scratch_bytes(h, w, subsampling) device bytes, 16-byte aligned; its previous contents do not matter.  Four
 * launches on `stream`, no synchronisation, no read-back. */
int dvd_jpeg_encode_rgb8(const uint8_t* img_hwc, int h, int w, int quality, int subsampling, uint8_t* out, long cap,
                         unsigned long long* out_len, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG decoder for the input photograph: the FILE goes to the device, the [H,W,3] u8 RGB page (EXIF orientation
 * applied) is made there - DESIGN.md 4.6.  The pixels are libjpeg's for such a file, integer arithmetic throughout
 * (accurate integer IDCT, triangle chroma upsampling, 16-bit fixed-point colour), i.e. byte for byte what
 * ImageOps.exif_transpose(Image.open(f)).convert("RGB") returns.
 * Accepted: SOF0, 8-bit samples and tables, Huffman, ONE scan of all components, 3 components as 4:4:4 / 4:2:2 / 4:2:0 or
 * 1 component at 1x1, with or without DRI.  Everything else is REFUSED on the host with one of the codes below before
 * anything is launched; a refusal is a normal outcome (the caller decodes on the CPU).
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_JPEG_HEADER (-20)       /* no SOI, a truncated or malformed header, no SOF / SOS */
#define DVD_E_JPEG_PROGRESSIVE (-21)  /* SOF2 */
#define DVD_E_JPEG_EXTENDED (-22)     /* SOF1 */
#define DVD_E_JPEG_LOSSLESS (-23)     /* SOF3, 5..7: lossless, hierarchical */
#define DVD_E_JPEG_ARITHMETIC (-24)   /* SOF9..15, DAC */
#define DVD_E_JPEG_PRECISION (-25)    /* samples of other than 8 bits */
#define DVD_E_JPEG_COMPONENTS (-26)   /* not 1 or 3 components, or ids 'R','G','B' without JFIF / Adobe (an RGB file) */
#define DVD_E_JPEG_ADOBE (-27)        /* an Adobe APP14 segment with transform 0 (RGB) */
#define DVD_E_JPEG_SAMPLING (-28)     /* sampling other than 4:4:4, 4:2:2, 4:2:0 / gray 1x1 */
#define DVD_E_JPEG_SCANS (-29)        /* more than one SOS */
#define DVD_E_JPEG_QUANT16 (-30)      /* a 16-bit quantisation table */
#define DVD_E_JPEG_TABLE (-31)        /* a quantisation or Huffman table the scan names is missing (or has id > 1 / > 3) */
#define DVD_E_JPEG_SIZE (-32)         /* 3 h w >= 2^31 */
#define DVD_E_JPEG_ORIENTATION (-33)  /* no EXIF orientation but an XMP packet that names one */
#define DVD_E_JPEG_NOSYNC (-34)       /* the entropy decoder's fixpoint took more than max_iters iterations */
#define DVD_E_JPEG_DATA (-35)         /* the scan does not hold the blocks the header implies */
#define DVD_JPEGDEC_SUBSEQ 128        /* bytes of the scan per lane of the entropy decoder */
typedef struct dvd_jpegdec_info {
  int h, w;                /* as in SOF0 */
  int out_h, out_w;        /* after the EXIF orientation: swapped for orientations 5..8 */
  int components;          /* 1 or 3 */
  int hs, vs;              /* luma sampling factors: 1x1, 2x1 or 2x2 */
  int orientation;         /* 1..8 */
  int restart_interval;    /* MCUs, 0 = none */
  long scan_offset;        /* first byte of the entropy-coded data in the file */
  long scan_bytes;         /* its bytes, stuffing and RSTn markers included */
  long blocks;             /* 8 x 8 blocks of the scan */
  long scratch_bytes;      /* device bytes dvd_jpeg_decode_rgb8 needs */
} dvd_jpegdec_info;
/* Host only: parses the n bytes of the file at file_host; 0 and *info, or the refusal code (dvd_last_error says why). */
int dvd_jpegdec_probe(const uint8_t* file_host, long n, dvd_jpegdec_info* info);
/* file_host / file_dev: the same n bytes on the host (parsed there) and on the device (the kernels read the scan there).
 * out_hwc [out_h,out_w,3] u8, any byte alignment; cap = bytes writable at it: cap < 3 h w is DVD_E_ARG.  Every bad
 * argument and every refusal is decided before anything is launched.  scratch: info.scratch_bytes device bytes, 16-byte
 * aligned; its contents do not matter.  max_iters >= 1 (0 = the default, 1024) caps the fixpoint iterations; *iters_out
 * (host, may be null) receives how many ran.  SYNCHRONISES `stream` after every 16 iterations (a 4-byte read-back: the
 * last iteration that changed a state) and once after the count pass (a 4-byte read-back: the blocks found); from there
 * on - coefficients, DC sums, IDCT, upsampling + colour + orientation - the launches are asynchronous.  Returns 0, a
 * refusal code, DVD_E_JPEG_NOSYNC or DVD_E_JPEG_DATA (out_hwc is untouched then), DVD_E_ARG or DVD_E_LAUNCH. */
int dvd_jpeg_decode_rgb8(const uint8_t* file_host, const uint8_t* file_dev, long n, uint8_t* out_hwc, long cap,
                         int max_iters, int* iters_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * PNG decoder for input photographs and ground-truth scans: the FILE goes to the device, the [H,W,3] u8 RGB page is made
 * there - DESIGN.md 4.9.  Integer work throughout: byte for byte what
 * ImageOps.exif_transpose(Image.open(f)).convert("RGB") returns for an accepted file.
 * Accepted: bit depth 8, colour type 0 (gray, replicated), 2 (RGB) or 6 (RGBA, alpha dropped), no interlace, one or more
 * consecutive IDAT chunks of any lengths, a zlib header with CM = 8 and no preset dictionary, IEND; other ancillary chunks
 * are skipped.  Everything else is REFUSED on the host with one of the codes below before anything is launched; DATA and
 * NOSPLIT are found on the device and leave the output untouched.  A refusal is a normal outcome (the caller decodes on
 * the CPU).
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_PNG_HEADER (-36)     /* no signature, a truncated or malformed chunk layout, a bad IHDR */
#define DVD_E_PNG_INTERLACE (-37)  /* Adam7 */
#define DVD_E_PNG_DEPTH (-38)      /* bit depth other than 8 */
#define DVD_E_PNG_COLOUR (-39)     /* colour type 3 (palette) or 4 (gray + alpha) */
#define DVD_E_PNG_TRNS (-40)       /* a tRNS chunk */
#define DVD_E_PNG_APNG (-41)       /* an acTL chunk */
#define DVD_E_PNG_METADATA (-42)   /* eXIf, or a text chunk "Raw profile type..." / "XML:com.adobe.xmp": an orientation may hide there */
#define DVD_E_PNG_ZLIB (-43)       /* a bad zlib header or a preset dictionary */
#define DVD_E_PNG_SIZE (-44)       /* 3 h w >= 2^31, or 2^29 bytes of IDAT data */
#define DVD_E_PNG_DATA (-45)       /* an invalid block, code, length or distance; a wrong inflated length; a filter byte above 4;
                                      an Adler-32 or IDAT CRC-32 mismatch */
#define DVD_E_PNG_NOSPLIT (-46)    /* a lane of the inflate exceeded max_work (a long stream of fixed or stored blocks) */
typedef struct dvd_pngdec_info {
  int h, w;                /* as in IHDR */
  int colour_type;         /* 0, 2 or 6 */
  int bpp;                 /* bytes per pixel in the file: 1, 3 or 4 */
  long idat_chunks;        /* IDAT chunks, empty ones included */
  long payload_bytes;      /* their data together: zlib header, deflate stream, Adler-32 */
  long scratch_bytes;      /* device bytes dvd_png_decode_rgb8 needs */
} dvd_pngdec_info;
typedef struct dvd_pngdec_stats {
  int candidates;          /* block starts the finder kept, segment 0 included */
  int segments;            /* those of them on the chain from segment 0 */
  int rounds;              /* pointer-doubling rounds, the last one (which changed nothing) included */
  int bands;               /* runs of rows the unfilter handles independently */
} dvd_pngdec_stats;
/* Host only: parses the n bytes of the file at file_host; 0 and *info, or the refusal code (dvd_last_error says why). */
int dvd_pngdec_probe(const uint8_t* file_host, long n, dvd_pngdec_info* info);
/* file_host / file_dev: the same n bytes on the host (parsed there) and on the device.  out_hwc [h,w,3] u8, any byte
 * alignment; cap = bytes writable at it: cap < 3 h w is DVD_E_ARG.  Every bad argument and every header refusal is decided
 * before anything is launched.  scratch: info.scratch_bytes device bytes, 16-byte aligned; its contents do not matter.
 * max_work >= 1 (0 = the default, 2^20) is the symbols + stored bytes one lane of the inflate may spend.  *stats_out (host,
 * may be null) receives what ran.  SYNCHRONISES `stream`: after the block finder (the candidate count), after the count
 * pass (the candidate table), after every 4 doubling rounds (4 bytes) and once before the unfilter (the status word: both
 * checksums, the filter bytes, the band count).  Returns 0, a refusal code, DVD_E_PNG_DATA or DVD_E_PNG_NOSPLIT (out_hwc is
 * untouched then), DVD_E_ARG or DVD_E_LAUNCH. */
int dvd_png_decode_rgb8(const uint8_t* file_host, const uint8_t* file_dev, long n, uint8_t* out_hwc, long cap,
                        long max_work, dvd_pngdec_stats* stats_out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Local distortion (LD) of the evaluation tail: the mean length of a dense SIFT-flow field from the flat ground-truth scan
 * A to the dewarped page B, on the device where both planes already lie.  The reference leaves it to offline MATLAB and
 * Ce Liu's mex code; the definition is this project's own (integer statement: tests/sflow_model.py), written
 * in integers throughout, and parity with the MATLAB/mex pipeline is UNPINNED.  No kernel uses an atomic: the same inputs
 * give the same bits on every launch, and document d of a batch gets the bits it gets alone.
 * ---------------------------------------------------------------------------------------- */
typedef struct dvd_sflow_params {
  int levels;     /* pyramid levels, 1..6 (default 4) */
  int w_top;      /* half window of the top level, 1..10 (10) */
  int w;          /* half window of the levels below it, 1..10 (2) */
  int iters_top;  /* BP iterations on the top level, 1..1000 (60) */
  int iters;      /* BP iterations below it, 1..1000 (30) */
  int alpha;      /* slope of the smoothness term, 0..65535 (510) */
  int d;          /* its truncation per component; messages lie in 0..2d, so 2d <= 65535 (10200) */
  int gamma;      /* weight of |f|_1 in the data term, >= 0 (1) */
  int T;          /* truncation of the 128-byte L1 distance; T + gamma * (largest |f|_1) <= 65535 (8160) */
  int eps;        /* added to the descriptor norm, 1..2^30 (131072) */
} dvd_sflow_params;
#define DVD_SFLOW_MIN_TOP 12 /* least side of the top pyramid level: one 12 x 12 descriptor patch */
/* gray [n,h,w] f32 planes of integer values 0..255 -> out [n,h,w,128] u8 (16-byte aligned): central differences with clamped
 * indices, eight half-rectified orientation responses in units of 1/1024, 3 x 3 cell sums, the 4 x 4 cells at offsets
 * 3i - 5 (clamped), n = floor(sqrt(sum h^2)) exactly, bytes min(255, 512 h / (n + eps)).  Each side 1..8192. */
int dvd_dsift_u8(const float* gray, int n, int h, int w, int eps, uint8_t* out, void* stream);
/* One document, one level.  desc_a, desc_b [h,w,128] u8 (16-byte aligned), off [2,h,w] int16 (window centres u then v),
 * labels (lu, lv) in [-win, win]^2 at index (lv + win)(2 win + 1) + (lu + win):
 * cost [h,w,L] u16 = (q inside ? min(T, L1(desc_a(p), desc_b(q))) : T) + gamma (|f_u| + |f_v|), f = off(p) + l, q = p + f. */
int dvd_sflow_cost(const uint8_t* desc_a, const uint8_t* desc_b, const int16_t* off, int h, int w, int win,
                   const dvd_sflow_params* params, uint16_t* cost, void* stream);
/* One document, one level: the cost volume, `iters` synchronous min-sum BP iterations from zero messages, then the belief's
 * argmin (ties: the smallest label index) as the absolute flow [2,h,w] int16.  workspace: dvd_sflow_level_workspace_bytes
 * (h, w, win) bytes, 256-byte aligned (the cost volume and two message buffers [4,h,w,L] u16; a negative DVD_E_* value
 * for a bad shape).  ld_out (device, one f64, may be null) receives sum sqrt(f_u^2 + f_v^2) / (h w). */
long dvd_sflow_level_workspace_bytes(int h, int w, int win);
int dvd_sflow_level(const uint8_t* desc_a, const uint8_t* desc_b, const int16_t* off, int h, int w, int win, int iters,
                    const dvd_sflow_params* params, void* workspace, int16_t* flow, double* ld_out, void* stream);
/* The whole chain for n pairs of gray planes a (scan), b (prediction) [n,h,w] f32 of integer values 0..255: planes to u8,
 * the integer [1,4,6,4,1] pyramid ((sum + 128) >> 8, ceil(n/2) per axis), then coarse to fine: descriptors of both
 * planes, offsets (0 on the top level, twice the coarser flow of p >> 1 below it), cost, BP, argmin.  flow [n,2,h,w] int16,
 * ld [n] f64 (device).  The documents are enqueued one after the other in ONE document's workspace:
 * dvd_sflow_workspace_bytes(h, w, params) bytes, 256-byte aligned (DESIGN.md 4.7 has the formula).  Refused with DVD_E_ARG
 * before any launch: a side of the top level below 12 or a side above 8192, and every parameter outside its range above. */
long dvd_sflow_workspace_bytes(int h, int w, const dvd_sflow_params* params);
int dvd_sflow(const float* a, const float* b, int n, int h, int w, const dvd_sflow_params* params, void* workspace,
              int16_t* flow, double* ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * Aligned distortion (AD), the benchmark's third number: the SIFT-flow chain above from the scan A to the page B, a
 * least-squares fit of a translation and a scale per axis to that field, B resampled through the fit, a second flow from A to
 * the resampled page, and the mean length of the second field weighted by the gradient magnitude of A.  The reference leaves
 * it to offline MATLAB (evalAlignedUnwarp, not in its tree); the definition is this project's own (integer
 * statement: tests/adist_model.py) and parity with the MATLAB pipeline is UNPINNED.  No atomics; no host read-back inside
 * the chain.  Every plane is [h,w] with sides 1..8192; every batch n is 1..65535.
 * ---------------------------------------------------------------------------------------- */
/* flow [n,2,h,w] int16 -> sums [n,4] int64 = (sum f_u, sum X f_u, sum f_v, sum Y f_v) with X = 2x - (w-1), Y = 2y - (h-1),
 * exactly, and coef [n,4] int32 = (ax, bx, ay, by) in Q16: ax = Su / (h w), bx = 2 Sxu / (h w (w^2 - 1) / 3), likewise y; each
 * rint(num / den * 65536) in f64 (ties to even), 0 for a zero denominator, saturated to +-(2^31 - 1).  scratch: device,
 * 32 * ceil(h w / 256) bytes, 8-byte aligned (the partial sums; the documents follow each other in it). */
int dvd_ad_fit(const int16_t* flow, int n, int h, int w, void* scratch, int64_t* sums, int32_t* coef, void* stream);
/* b [n,h,w] f32 of integer values 0..255, coef [n,4] int32 ON THE DEVICE -> out [n,h,w] f32 (integer values): b at
 * cx = clamp((x << 16) + ax + ((bx X) >> 1), 0, (w-1) << 16) and cy likewise, bilinear with the 8-bit fractions (c >> 8) & 255,
 * (sum + 32768) >> 16.  All-zero coefficients copy b.  out must not overlap b. */
int dvd_ad_align(const float* b, const int32_t* coef, int n, int h, int w, float* out, void* stream);
/* a [n,h,w] f32 of integer values 0..255, flow [n,2,h,w] int16 -> ad [n] f64 (device): sum g |f| / sum g with g =
 * floor(sqrt(gx^2 + gy^2)) of a's clamped central differences; the plain mean of |f| when sum g = 0.  The f64 additions run
 * in the fixed order of the LD sum.  scratch: device, 24 * ceil(h w / 256) bytes, 8-byte aligned. */
int dvd_ad_weighted(const float* a, const int16_t* flow, int n, int h, int w, void* scratch, double* ad, void* stream);
/* The whole chain for n pairs a (scan), b (prediction) as in dvd_sflow: flow 1, fit, align, flow 2, weighted mean, enqueued
 * per document in ONE document's workspace of dvd_adist_workspace_bytes(h, w, params) bytes, 256-byte aligned (one
 * dvd_sflow workspace for both passes, the resampled plane, two flows, the partials).  ld [n] f64 = the first pass's LD (the
 * bits dvd_sflow gives), ad [n] f64; flow1, flow2 [n,2,h,w] int16, sums [n,4] int64, coef [n,4] int32 and aligned [n,h,w] f32
 * may each be null.  Refused with DVD_E_ARG before any launch like dvd_sflow. */
long dvd_adist_workspace_bytes(int h, int w, const dvd_sflow_params* params);
int dvd_adist(const float* a, const float* b, int n, int h, int w, const dvd_sflow_params* params, void* workspace, double* ld,
              double* ad, int16_t* flow1, int64_t* sums, int32_t* coef, float* aligned, int16_t* flow2, void* stream);

/* ------------------------------------------------------------------------------------------
 * Common corruptions of the network input (run_sampling.py --corruption): the benchmark numbering of Hendrycks & Dietterich,
 * 0 gaussian_noise .. 14 jpeg_compression, 15 speckle_noise .. 18 saturate, severities 1..5.  The definitions are this
 * project's own, in integer arithmetic (tests/corrupt_model.py states every kind byte for byte); parity with
 * the `imagecorruptions` package is UNPINNED.  A corrupted image is a function of (bytes, kind, severity, key) only.  No
 * scratch memory, no atomics, no host read-back.
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_CORRUPT_KIND (-47)     /* a kind outside 0..18, or one without a kernel (4, 7, 8, 9, 12, 17, 18; 14 = the JPEG codec) */
#define DVD_E_CORRUPT_SEVERITY (-48) /* a severity outside 1..5 */
#define DVD_E_CORRUPT_SIZE (-49)     /* a side outside 32..16384 */
/* 1: dvd_corrupt_rgb8 has a kernel for the kind; 2: the kind is delivered by other entry points (14: dvd_jpeg_encode_rgb8 with
 * 4:2:0 at quality 25 18 15 10 7, then dvd_jpeg_decode_rgb8); 0: refused, or no kind at all.  Host-only. */
int dvd_corrupt_supported(int kind);
/* The real-valued tables, built on the host in double and quantised once; host-only, `out` is HOST memory (null: only count).
 * Kind 1: [256][c] thresholds floor(CDF_Poisson(x c / 255)(j) 2^32) saturated to 2^32 - 1, c = 60 25 12 5 3.  Kinds 3, 5, 16:
 * [side][side] Q16 weights that sum to exactly 65536; `angle` (kind 5 only) in degrees, -45..45.  Returns the number of
 * entries (cap below it with a non-null out is DVD_E_ARG) or a DVD_E_CORRUPT_* code. */
int dvd_corrupt_table(int kind, int severity, int angle, uint32_t* out, int cap);
/* in, out [n,h,w,3] u8 (out must not be in), keys [n,2] u32 on the device: image i is corrupted with the Philox4x32-10 key
 * (keys[2i], keys[2i+1]).  n 1..65535, sides 32..16384.  One launch; the first call on a device that needs a table (kinds 1,
 * 3, 5, 16) also copies the tables there and waits for that copy.  Every argument is checked before anything is launched. */
int dvd_corrupt_rgb8(const uint8_t* in, uint8_t* out, int n, int h, int w, int kind, int severity, const uint32_t* keys,
                     void* stream);
/* The two ends of the stage in the document loop.  y [n,3,h,w] f32 in 0..1 (the network input: k / 255) -> bytes [n,h,w,3] =
 * clamp(rint(255 y), 0, 255), ties to even, NaN -> 0; and bytes -> y = k / 255, the correctly rounded division of dvd_ingest_u8.
 * 3 n h w below 2^31. */
int dvd_unit_to_rgb8(const float* y_nchw, uint8_t* out_nhwc, int n, int h, int w, void* stream);
int dvd_rgb8_to_unit(const uint8_t* in_nhwc, float* y_nchw, int n, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Keyed sampler noise and the map deviation (tests/noise_model.py states both bit for bit).
 * ---------------------------------------------------------------------------------------- */
/* keys [docs,2] u32 on the device -> out [docs*n_hyp,2,g,g] f32 standard normals.  Element e = (ch g + i) g + j of sample
 * doc n_hyp + h is lane e & 3 of Box-Muller on Philox4x32-10(key (keys[2 doc], keys[2 doc + 1]), counter (e >> 2, slot, h, 2)):
 * a function of the document's key, h, slot and e only.  slot 0 is x_T, slot 1 + i the noise of step index i.  The logarithm,
 * cosine and sine are written out in separately rounded f32 operations (no library call).  docs and n_hyp 0..65535 (a product
 * of 0 is a no-op), g 2..8192, at most 2^38 quads.  One launch; every argument is checked before it. */
int dvd_randn_keyed(const uint32_t* keys, int docs, int n_hyp, int g, uint32_t slot, float* out, void* stream);
/* a, b [docs,2,g,g] f32 on the device -> out [docs] f64 (device) = 0.987 * 511 * mean_j sqrt(dx_j^2 + dy_j^2) over the g^2 grid
 * points: how far, in pixels of the 512 x 512 network input, map b samples from where map a does.  The distances are f32
 * (separately rounded), their sum is f64 in a fixed order (no atomics), so equal maps give exactly 0.  ws: device,
 * dvd_map_deviation_workspace_bytes(docs, g) bytes (8 per 1024 grid points of a document, rounded up), 8-byte aligned; that
 * query returns DVD_E_ARG for a bad shape.  docs 0..65535 (0 is a no-op), g 2..8192.  Two launches. */
long dvd_map_deviation_workspace_bytes(int docs, int g);
int dvd_map_deviation(const float* a, const float* b, int docs, int g, double* out, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flow pictures and the .flo payload of a predicted map (tests/flowviz_model.py states every entry point byte
 * for byte).  A picture is the Middlebury colour-wheel image of a displacement field in pixels: hue = direction, saturation =
 * radius / rad_max.  Separately rounded f32 with a written-out angle; a pixel with a non-finite component is (0,0,0).
 * n 0..65535 (0 is a no-op), sides 1..16384, g 2..8192: anything else is DVD_E_FLOW_SHAPE, before any launch.  No scratch
 * memory, no atomics, no host read-back.
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_FLOW_SHAPE (-50)
#define DVD_FLOW_NORM_DIAG 0 /* rad_max = sqrt((w/2)^2 + (h/2)^2) + 1e-5, integer halves: datasets/utils/flow_viz.py */
#define DVD_FLOW_NORM_MAX 1  /* rad_max = the image's largest radius + 1e-5: the Middlebury rule */
/* bytes of `ws` for n images of h x w (4 per 4096 pixels of an image, rounded up), or DVD_E_FLOW_SHAPE */
long dvd_flow_workspace_bytes(int n, int h, int w);
/* field [n,h,w,2] f32 (u, v interleaved, 8-byte aligned) -> out [n] f32: per image the largest sqrt(u^2 + v^2) over its pixels
 * with finite components (0 if there is none), after the clip.  clip < 0: none; otherwise both components are clipped to
 * [0, clip] first (the reference's clip_flow).  Two launches in a fixed order. */
int dvd_flow_radius_max(const float* field, int n, int h, int w, float clip, float* out, void* ws, void* stream);
/* field [n,h,w,2] f32 -> out [n,h,w,3] u8 (4-byte aligned), RGB or, with bgr != 0, BGR.  norm DVD_FLOW_NORM_MAX runs
 * dvd_flow_radius_max first and needs `largest` [n] f32 (it receives the radii) and `ws`; with DVD_FLOW_NORM_DIAG both may be
 * null.  One launch, or three. */
int dvd_flow_to_image_rgb8(const float* field, int n, int h, int w, int norm, float clip, int bgr, uint8_t* out, float* largest,
                           void* ws, void* stream);
/* flow [n,2,g,g] f32, the coarse map -> out [n,h,w,2] f32: s = F.interpolate(flow, (h, w), bilinear, align_corners=True) in the
 * arithmetic of the unwarp tail, then u = s_x (w - 1), v = s_y (h - 1).  The payload of a Middlebury .flo file.  One launch. */
int dvd_flow_full_uv(const float* flow, int n, int g, int h, int w, float* out, void* stream);
/* The coarse map -> out [n,h,w,3] u8 in one pass: the bytes of dvd_flow_to_image_rgb8 (no clip) on dvd_flow_full_uv, without
 * writing the field.  norm, bgr, largest, ws as above (DVD_FLOW_NORM_MAX takes the maximum over the same recomputed field). */
int dvd_flow_picture_rgb8(const float* flow, int n, int g, int h, int w, int norm, int bgr, uint8_t* out, float* largest, void* ws,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * The map score: a predicted map against a ground-truth map (tests/mapscore_model.py is the definition).
 * One document per call.  The prediction flow [2,g,g] is evaluated at the ground truth's h x w with the arithmetic of
 * dvd_flow_full_uv.  A pixel is valid when both ground-truth components are finite and at most 1e9 in magnitude (the Middlebury
 * unknown-flow rule) and the prediction and every hypothesis are finite there; an invalid pixel enters nothing.
 * Sides 1..16384, g 2..8192, n_hyp 1..64: anything else is DVD_E_MAP_SHAPE; bad ranks are DVD_E_MAP_RANKS; both before any
 * launch.  No scratch memory, no atomics on floats, integer sums only where the order could matter.
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_MAP_SHAPE (-51)
#define DVD_E_MAP_RANKS (-52)
/* bytes of `ws` for a document of h x w, 256-byte aligned, or DVD_E_MAP_SHAPE.  Its parts in order: a head of one size for every
 * h x w (selection state, block histograms, block bins: dvd_select_u32 and dvd_sparsify_bins use nothing else, so
 * dvd_mapscore_workspace_bytes(1, 1) serves them for any n), the block partials of dvd_map_errors, and room for the two planes:
 * the last two parts, each 4 h w bytes rounded up to 256. */
long dvd_mapscore_workspace_bytes(int h, int w);
/* e [h w] and sigma [h w] f32 <- flow [2,g,g], the ground truth gt (gt_g = 0: a displacement field [h,w,2] in pixels, 8-byte
 * aligned, the layout of a .flo file; gt_g >= 2: a coarse map [2,gt_g,gt_g]) and hyps [n_hyp,2,g,g] (may be null with n_hyp 1).
 * g = 0: flow is itself such a field [h,w,2] (then n_hyp must be 1).
 * e = sqrt(du^2 + dv^2) in separately rounded f32; sigma = sqrt(mean_h |d_h - mean|^2) over the up-sampled hypotheses, 0 with
 * n_hyp = 1.  An invalid pixel gets the bit pattern 0xffffffff in both planes.  Also writes the block partials of the headline
 * numbers into ws.  One launch. */
int dvd_map_errors(const float* flow, int g, const float* gt, int gt_g, const float* hyps, int n_hyp, int h, int w, float* e,
                   float* sigma, void* ws, void* stream);
/* Adds the block partials a dvd_map_errors call of the same h x w left in ws: out (device, seven 8-byte words) = u64 n_valid,
 * #(e <= 1), #(e <= 3), #(e <= 5), #(e > 3 and e / |gt| > 0.05), then the f64 sums of e and of e^2, added in a fixed order. */
int dvd_map_metrics(const void* ws, int h, int w, void* out, void* stream);
/* out [k] (device) = the order statistics keys_sorted_ascending[ranks[i]] of n u32 keys on the device.  ranks: k = 1..50 values
 * on the HOST, non-decreasing, each below n.  MSD radix selection in four 8-bit levels, eight launches, no host read-back.
 * Non-negative finite f32 values select as their bit patterns. */
int dvd_select_u32(const uint32_t* keys, long n, const uint32_t* ranks, int k, uint32_t* out, void* ws, void* stream);
/* out [(k + 1) * 4] u64 (device): bin b = 0..k holds, over the pixels p with e[p] valid whose key[p] is <= exactly b of the k
 * thresholds thr (device, u32 bit patterns in non-increasing order), the count, #(e <= 1), #(e <= 5) and the sum of
 * rint(min(e, 2^15) 2^20): at most 2^63 over 2^28 pixels.  key and e are planes of dvd_map_errors (key = e or sigma). */
int dvd_sparsify_bins(const float* e, const float* key, long n, const uint32_t* thr, int k, unsigned long long* out, void* ws,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * The map inverse (tests/mapinv_model.py is the definition).  The predicted map flow [2,g,g] is a backward map:
 * page pixel -> photograph position, the position the unwarp tail samples (dvd_unwarp_grid, un-normalised with
 * align_corners=True).  Its inverse at the photograph's h x w comes from rasterising the page's triangle mesh - lattice rows and
 * columns 0, step, 2 step, .., h - 1 / w - 1 - on the photograph: vertices in Q8 integers, exact int64 edge functions, the
 * top-left rule, the smallest triangle id wins.  fwd [h,w,2] f32 holds the page position (u, v) of every covered photograph
 * pixel and the bit pattern 0xffffffff in both components elsewhere.
 * Sides 1..16384 and g 2..8192 (else DVD_E_INV_SHAPE), step 1..16384 (DVD_E_INV_STEP), lines 2..16384 and thickness 1..3
 * (DVD_E_INV_LINES), 0..2^28 points (DVD_E_INV_POINTS): all refused before any launch.  No scratch memory; the one atomic is an
 * integer minimum.
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_INV_SHAPE (-53)
#define DVD_E_INV_STEP (-54)
#define DVD_E_INV_LINES (-55)
#define DVD_E_INV_POINTS (-56)
/* bytes of `ws` for a photograph of h x w and a mesh of `step`, 256-byte aligned, or a status above */
long dvd_map_invert_workspace_bytes(int h, int w, int step);
/* fwd [h,w,2] f32 (8-byte aligned) and stats (device, six u64: covered, fold_px, flipped_tris, degenerate_tris, skipped_tris,
 * tris) <- flow [2,g,g].  A triangle with an invalid vertex (not finite, or beyond 2^22 px) or whose clipped bounding box holds
 * more than max(1024, 64 step^2) pixels is skipped; one of area 0 is degenerate; one of negative area is rasterised with two
 * vertices swapped and counted as flipped.  fold_px = the pixels covered by two or more triangles.  Five launches. */
int dvd_map_invert(const float* flow, int g, int h, int w, int step, float scale, float* fwd, unsigned long long* stats, void* ws,
                   void* stream);
/* out (device, three 8-byte words) = n, the bits of the f64 sum and the bits of the f32 maximum of |backward(fwd(p)) - p| over
 * the covered pixels p where it is finite; the sum is added in a fixed order.  ws: a workspace of the same h x w, any step. */
int dvd_map_cycle_error(const float* flow, int g, const float* fwd, int h, int w, float scale, unsigned long long* out, void* ws,
                        void* stream);
/* out [h,w,3] u8 <- src [h,w,3] u8 (another buffer) with the page's grid drawn on it: `lines` lines per axis in `color`, the
 * page's outline in `outline_color` (both 0x00BBGGRR), widened to `thickness`; dim != 0 halves the uncovered pixels. */
int dvd_mesh_overlay_rgb8(const uint8_t* src, const float* fwd, int h, int w, int lines, int thickness, uint32_t color,
                          uint32_t outline_color, int dim, uint8_t* out, void* stream);
/* out [n,2] f32 (u, v on the page) <- pts [n,2] f32 (x, y on the photograph): fwd sampled bilinearly; 0xffffffff in both
 * components where the point is outside the photograph or a tap is uncovered. */
int dvd_transfer_points(const float* fwd, int h, int w, const float* pts, long n, float* out, void* stream);
/* out [n,2] f32 (x, y on the photograph) <- pts [n,2] f32 (u, v on the page, clamped to it): the backward map, bilinear over the
 * four surrounding page pixels' positions; 0xffffffff where a component is not finite. */
int dvd_map_points(const float* flow, int g, int h, int w, float scale, const float* pts, long n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic documents (tests/synth_model.py is the definition).  A flat scan [hs,ws,3] u8 is drawn on a
 * photograph of h x w through fwd [h,w,2] f32, exactly what dvd_map_invert writes: the page position (u, v) in page pixels of
 * every covered photograph pixel, the bit pattern 0xffffffff elsewhere.  Per covered pixel: the Q8 scan position
 * floor(u (ws - 1) / (w - 1) 256 + 1/2); integer radii rx, ry = 1..8 from the first differences over the covered 4-neighbours;
 * a separable integer tent of that half-width (rx = ry = 1 is Q8 bilinear sampling), rounded exactly; optional shading in Q16;
 * and a blend with the background by the covered share of the 3 x 3 window.  An uncovered pixel takes the background.
 * Sides 1..16384 (else DVD_E_SYNTH_SHAPE), finite shading parameters and, with shading on, a_ref > 0 (DVD_E_SYNTH_PARAM): all
 * refused before any launch.  No atomics, no scratch memory; equal calls give equal bytes.
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_SYNTH_SHAPE (-57)
#define DVD_E_SYNTH_PARAM (-58)
/* Shading: each channel c becomes min(255, (c Lq + 32768) >> 16), Lq = clamp(rint(65536 L), 0, 131072),
 * L = l0 + lgx (px / (w - 1) - 1/2) + lgy (py / (h - 1) - 1/2) + k (A / a_ref - 1), A = the scan area under the photograph pixel.
 * All of l0, lgx, lgy, k zero: no shading, and a_ref is not read. */
typedef struct {
  float l0, lgx, lgy, k;
  float a_ref; /* the mean scan area per covered photograph pixel: hs ws / covered */
} dvd_synth_params;
/* out [h,w,3] u8 <- scan [hs,ws,3] u8 through fwd (8-byte aligned).  bg [h,w,3] u8, or NULL for the colour bg_color
 * (0x00BBGGRR) everywhere.  Where w is a multiple of 4 the picture is stored as whole dwords and out must be 4-byte aligned.
 * out must be another buffer than scan and bg.  One launch. */
int dvd_synth_render_rgb8(const uint8_t* scan, int hs, int ws, const float* fwd, int h, int w, const uint8_t* bg, uint32_t bg_color,
                          const dvd_synth_params* params, uint8_t* out, void* stream);
/* out [h,w,2] u8 <- the radii (rx, ry) the render uses at every covered pixel, 0 at the others.  One launch. */
int dvd_synth_footprint(const float* fwd, int h, int w, int hs, int ws, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pages at a chosen size (tests/sized_model.py is the definition).  The photograph src [hs,ws,3] u8 is unwarped
 * through flow [2,g,g] to a page of hp x wp, any size 1..16384.  Per page pixel (i, j): the grid value of dvd_unwarp_grid at
 * the page's size (at hp = hs, wp = ws the native tail's own, bit for bit); the signed Q8 position floor(256 x + 1/2) of
 * x = (gx + 1) ((ws - 1) / 2) on the photograph, moved to 17 pixels outside it where it is further out; integer radii
 * rx, ry = 1..max_radius from the doubled first differences of those positions over the page's 4-neighbours; and the separable
 * integer tent of dvd_synth_render_rgb8 with that half-width over the PHOTOGRAPH (rx = ry = 1 is Q8 bilinear sampling).  A tap
 * outside the photograph contributes zero and its weight still counts (padding_mode='zeros'), so the divisor is the constant
 * 65536 rx^2 ry^2 and the byte is ROUNDED once - the native u8 tail truncates.  A pixel whose grid value is not finite is
 * black and its neighbours' differences go without it.
 * stats (device, DVD_SIZED_STATS 8-byte words per document, or NULL): the page pixels whose uncapped radius exceeded max_radius,
 * whose centre lies outside the photograph, and whose grid value is not finite - exact integers, added with integer atomics.
 * Sides 1..16384 and g 2..8192 (else DVD_E_SIZED_SHAPE), a finite scale and max_radius 1..16 (DVD_E_SIZED_PARAM), no null
 * pointer and a page that shares no byte with its photograph (DVD_E_ARG): all refused before any HIP call.  No scratch
 * memory; equal calls give equal bytes.
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_SIZED_SHAPE (-59)
#define DVD_E_SIZED_PARAM (-60)
#define DVD_SIZED_STATS 3
/* out [hp,wp,3] u8, any byte alignment.  One launch (and one memset of stats). */
int dvd_unwarp_u8_sized(const float* flow, int g, const uint8_t* src, int hs, int ws, uint8_t* out, int hp, int wp, float scale,
                        int max_radius, unsigned long long* stats, void* stream);
/* One document of dvd_unwarp_u8_sized_ragged: device pointers to its photograph and its page, and their sizes. */
typedef struct {
  const uint8_t* src; /* [hs,ws,3] uint8 */
  uint8_t* out;       /* [hp,wp,3] uint8 */
  int hs, ws, hp, wp;
} dvd_sized_image;
/* flow [n,2,g,g], stats [n,DVD_SIZED_STATS] or NULL: docs[d].out and the counts of document d equal those of
 * dvd_unwarp_u8_sized(flow + d*2*g*g, g, docs[d]..., scale, max_radius, stats + d*DVD_SIZED_STATS) byte for byte.  docs is a
 * HOST array read during the call only; at most DVD_RAGGED_CAP documents and 2^23 tiles of 64 x 16 page pixels go into one
 * launch (a larger batch is cut into several).  Documents may share a photograph; a page may share no byte with any photograph
 * or any other page of its launch (DVD_E_ARG, before any HIP call). */
int dvd_unwarp_u8_sized_ragged(const float* flow, int g, const dvd_sized_image* docs, int n, float scale, int max_radius,
                               unsigned long long* stats, void* stream);
/* out [hp,wp] u16 <- rx | ry << 8, the radii dvd_unwarp_u8_sized uses at every page pixel for a photograph of hs x ws, 0 where
 * the grid value is not finite.  A radius equal to max_radius may be the cap.  One launch; no photograph is read. */
int dvd_sized_footprint(const float* flow, int g, int hs, int ws, int hp, int wp, float scale, int max_radius, uint16_t* out,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Scan-like pages (tests/clean_model.py is the definition).  All integer arithmetic; equal calls give equal
 * bytes.  A page is img [h,w,3] u8, sides 1..16384 (else DVD_E_CLEAN_SHAPE).
 *   background  cell s in {4,8,16,32,64}: the coarse plane has hc = ceil(h/s) x wc = ceil(w/s) cells.  Per channel: the maximum
 *               of every cell (cut at the page's edge); a closing with a (2 close + 1)^2 window, close 0..8 (maximum, then
 *               minimum, windows clipped to the plane); a separable tent 1, 2, .., smooth + 1, .., 2, 1, smooth 0..8, over the
 *               clipped window, bg = (2 num + den) / (2 den) rounded once.  neutral == 0: the plane (R + 2 G + B + 2) >> 2 of
 *               that result stands for all three channels (the colour cast stays).
 *   flatten     bg is sampled bilinearly between cell centres (i + 1/2) s - 1/2 in units of 1/(2s), clamped at the plane's edge:
 *               bgQ = 4 s^2 x the sample, raised to at least 4 s^2; q = (v white 4 s^2 + bgQ / 2) / bgQ, out = min(255, q),
 *               white 1..255.  Counts: samples with q > 255 (saturated) and samples whose bgQ was raised (floored).
 *   binarise    Sauvola's rule on g = (R + 2 G + B + 2) >> 2 over the (2 radius + 1)^2 window clipped to the page, radius 1..63,
 *               kq = round(256 k) in 0..256, R = 128: with N, S1 = sum g, S2 = sum g^2 and sN = floor(sqrt(N S2 - S1^2)) the
 *               pixel is ink (0) iff g N (256 R N) <= S1 (256 R N) + kq S1 (sN - R N), else 255.  Count: the ink pixels.
 * A parameter outside its range is DVD_E_CLEAN_PARAM; a null pointer, a misaligned count pointer or an output that shares bytes
 * with an input is DVD_E_ARG: all refused before any HIP call.  The counts are exact integers (DVD_CLEAN_STATS 8-byte words in
 * the order saturated, floored, ink), added with integer atomics; an entry point zeroes the words it counts into.  No scratch
 * memory.
 * ---------------------------------------------------------------------------------------- */
#define DVD_E_CLEAN_SHAPE (-61)
#define DVD_E_CLEAN_PARAM (-62)
#define DVD_CLEAN_STATS 3
/* bytes of `ws` for a page of h x w at cell size `cell`, 256-byte aligned pieces in this order: the cell maxima [3,hc,wc], the
 * background [3,hc,wc] and the gray plane [h,w]; DVD_E_CLEAN_SHAPE / DVD_E_CLEAN_PARAM for a bad size or cell.  Host only. */
long dvd_page_clean_workspace_bytes(int h, int w, int cell);
/* bg [3,hc,wc] u8 <- img.  ws: dvd_page_clean_workspace_bytes(h, w, cell) bytes (the cell maxima are kept there).  Two
 * launches. */
int dvd_page_background(const uint8_t* img, int h, int w, int cell, int close, int smooth, int neutral, uint8_t* bg, void* ws,
                        void* stream);
/* out [h,w,3] u8 (any byte alignment) <- img flattened by bg [3,hc,wc] u8.  gray [h,w] u8 or NULL: the plane g of OUT.
 * stats: 2 words (saturated, floored) or NULL.  One launch (and one memset of stats). */
int dvd_page_flatten_rgb8(const uint8_t* img, int h, int w, const uint8_t* bg, int cell, int white, uint8_t* out, uint8_t* gray,
                          unsigned long long* stats, void* stream);
/* out [h,w] u8 (0 ink, 255 paper) <- img [h,w,channels] u8, channels 3 (RGB) or 1 (a gray plane, taken as g).  ink: 1 word or
 * NULL.  One launch (and one memset of ink). */
int dvd_page_binarize_u8(const uint8_t* img, int channels, int h, int w, int radius, int kq, uint8_t* out, unsigned long long* ink,
                         void* stream);
/* The chain in one workspace: the background and the flattened page (flatten != 0: page [h,w,3] u8), then the Sauvola plane of
 * that page - or of img where flatten == 0 - (binarize != 0: plane [h,w] u8).  At least one of the two; the output that is not
 * asked for may be NULL.  stats: DVD_CLEAN_STATS words or NULL; a count of a stage that does not run is 0.  The flattened
 * page's gray plane goes through ws, so binarising reads no RGB page again. */
int dvd_page_clean_rgb8(const uint8_t* img, int h, int w, int cell, int close, int smooth, int neutral, int white, int flatten,
                        int binarize, int radius, int kq, uint8_t* page, uint8_t* plane, unsigned long long* stats, void* ws,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVD_HIP_H */
