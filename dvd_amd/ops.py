"""Thin torch-tensor wrappers over the op-level entry points of libdvd_hip.so.

PyTorch supplies device memory and the current HIP stream; every computation happens in the
HIP library.  These wrappers mirror the reference callables they replace:
  grid_sample  <- register_model2(size,'bilinear')([img, grid])   datasets/utils/warping.py:14-23
  unwarp_*     <- evaluation.py:301-306 + visualization_utils.py:75-77
  sched_step   <- GaussianDiffusion.ddim_sample arithmetic         idf/gaussian_diffusion.py:470-489
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np
import torch

from . import lib, run_options
from .lib import ptr, stream_ptr
from .run_options import either


def _chk(t: torch.Tensor, dtype, name):
    if not t.is_cuda:
        raise lib.DvdError(f"{name}: expected a device tensor (the DvD engine has no CPU path)")
    if t.dtype != dtype or not t.is_contiguous():
        raise lib.DvdError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")


def _warp_mode(mode, name):
    """The interpolation of a warp: checked before anything is allocated or launched."""
    if mode not in run_options.WARP_MODES:
        raise ValueError(f"{name}: mode must be {either(run_options.WARP_MODES)}, got {mode!r}")
    return mode == "bicubic"


def grid_sample(src: torch.Tensor, grid_nchw: torch.Tensor, src_batch_div: int = 1, mode: str = "bilinear") -> torch.Tensor:
    """F.grid_sample(src, grid, mode, padding_mode='zeros', align_corners=True); mode 'bilinear' | 'bicubic'."""
    cubic = _warp_mode(mode, "grid_sample")
    _chk(src, torch.float32, "src")
    _chk(grid_nchw, torch.float32, "grid")
    n, two, h, w = grid_nchw.shape
    ns, c, hin, win = src.shape
    assert two == 2 and ns * src_batch_div == n
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=src.device)
    lib.call("dvd_grid_sample_bicubic_zeros_ac" if cubic else "dvd_grid_sample_bilinear_zeros_ac", ptr(src), ptr(grid_nchw),
             ptr(out), n, c, hin, win, h, w, src_batch_div, stream_ptr())
    return out


def unwarp_grid(flow: torch.Tensor, h: int, w: int, scale: float = 0.987) -> torch.Tensor:
    _chk(flow, torch.float32, "flow")
    g = flow.shape[-1]
    out = torch.empty((1, 2, h, w), dtype=torch.float32, device=flow.device)
    lib.call("dvd_unwarp_grid", ptr(flow), g, ptr(out), h, w, C.c_float(scale), stream_ptr())
    return out


def unwarp_f32(flow: torch.Tensor, src_chw: torch.Tensor, scale: float = 0.987) -> torch.Tensor:
    """flow [1,2,G,G] (or [2,G,G]); src [1,3,H,W] f32 0..255 -> [H,W,3] f32."""
    _chk(flow, torch.float32, "flow")
    _chk(src_chw, torch.float32, "src")
    h, w = src_chw.shape[-2:]
    out = torch.empty((h, w, 3), dtype=torch.float32, device=src_chw.device)
    lib.call("dvd_unwarp_f32", ptr(flow), flow.shape[-1], ptr(src_chw), ptr(out), h, w, C.c_float(scale), stream_ptr())
    return out


def unwarp_u8(flow: torch.Tensor, src_hwc: torch.Tensor, scale: float = 0.987, mode: str = "bilinear") -> torch.Tensor:
    """flow [1,2,G,G]; src [H,W,3] uint8 -> [H,W,3] uint8 (truncated like numpy astype; mode='bicubic': clamped to 0..255
    first, np.clip(a, 0, 255).astype(uint8))."""
    cubic = _warp_mode(mode, "unwarp_u8")
    _chk(flow, torch.float32, "flow")
    _chk(src_hwc, torch.uint8, "src")
    h, w = src_hwc.shape[:2]
    out = torch.empty_like(src_hwc)
    if cubic:
        lib.call("dvd_unwarp_u8_bicubic_batch", ptr(flow), flow.shape[-1], ptr(src_hwc), ptr(out), 1, h, w, C.c_float(scale),
                 stream_ptr())
    else:
        lib.call("dvd_unwarp_u8", ptr(flow), flow.shape[-1], ptr(src_hwc), ptr(out), h, w, C.c_float(scale), stream_ptr())
    return out


def unwarp_u8_batch(flow: torch.Tensor, src_nhwc: torch.Tensor, scale: float = 0.987, mode: str = "bilinear") -> torch.Tensor:
    """flow [B,2,G,G]; src [B,H,W,3] uint8 -> [B,H,W,3] uint8: the batch's documents in ONE launch."""
    cubic = _warp_mode(mode, "unwarp_u8_batch")
    _chk(flow, torch.float32, "flow")
    _chk(src_nhwc, torch.uint8, "src")
    b, h, w, three = src_nhwc.shape
    assert three == 3 and flow.shape[0] == b and flow.shape[1] == 2
    out = torch.empty_like(src_nhwc)
    lib.call("dvd_unwarp_u8_bicubic_batch" if cubic else "dvd_unwarp_u8_batch", ptr(flow), flow.shape[-1], ptr(src_nhwc),
             ptr(out), b, h, w, C.c_float(scale), stream_ptr())
    return out


def _carve(sizes, device, align=256):
    """One uint8 allocation cut into len(sizes) pieces, each starting on an `align`-byte boundary."""
    offs, total = [], 0
    for sz in sizes:
        offs.append(total)
        total += -(-sz // align) * align
    buf = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    return [buf[o:o + sz] for o, sz in zip(offs, sizes)]


def _ragged_table(srcs, outs):
    tab = (lib.RaggedImage * max(len(srcs), 1))()
    for d, (s, o) in enumerate(zip(srcs, outs)):
        tab[d].src, tab[d].out = s.data_ptr(), (None if o is None else o.data_ptr())
        tab[d].h, tab[d].w = s.shape[0], s.shape[1]
    return tab


def unwarp_u8_ragged(flow: torch.Tensor, srcs, scale: float = 0.987, mode: str = "bilinear"):
    """flow [n,2,G,G]; srcs: n [h_d,w_d,3] uint8 tensors of ANY sizes -> n uint8 tensors, each the bytes of
    unwarp_u8(flow[d:d+1], srcs[d], mode=mode): the batch's documents in ONE launch (per lib.RAGGED_CAP documents).  The
    outputs are views of one allocation."""
    cubic = _warp_mode(mode, "unwarp_u8_ragged")
    _chk(flow, torch.float32, "flow")
    srcs = list(srcs)
    assert flow.dim() == 4 and flow.shape[0] == len(srcs) and flow.shape[1] == 2
    for d, s in enumerate(srcs):
        _chk(s, torch.uint8, f"srcs[{d}]")
        assert s.dim() == 3 and s.shape[2] == 3, f"srcs[{d}]: expected [H,W,3]"
    if not srcs:
        return []
    outs = [o.view(s.shape) for o, s in zip(_carve([s.numel() for s in srcs], flow.device), srcs)]
    lib.call("dvd_unwarp_u8_bicubic_ragged" if cubic else "dvd_unwarp_u8_ragged", ptr(flow), flow.shape[-1],
             _ragged_table(srcs, outs), len(srcs), C.c_float(scale), stream_ptr())
    return outs


def unwarp_f32_batch(flow: torch.Tensor, src_nchw: torch.Tensor, scale: float = 0.987) -> torch.Tensor:
    """flow [B,2,G,G]; src [B,3,H,W] f32 0..255 -> [B,H,W,3] f32."""
    _chk(flow, torch.float32, "flow")
    _chk(src_nchw, torch.float32, "src")
    b, three, h, w = src_nchw.shape
    assert three == 3 and flow.shape[0] == b and flow.shape[1] == 2
    out = torch.empty((b, h, w, 3), dtype=torch.float32, device=src_nchw.device)
    lib.call("dvd_unwarp_f32_batch", ptr(flow), flow.shape[-1], ptr(src_nchw), ptr(out), b, h, w, C.c_float(scale),
             stream_ptr())
    return out


def ingest_u8(img_hwc: torch.Tensor, swap_rb: bool = False, out_size: int = 512, want_rgb: bool = False):
    """Decoded image [H,W,3] uint8 on the device -> source_image [3,out,out] f32 in 0..1 (cv2.resize INTER_LINEAR / 255,
    doc_benchmark.py:84-88) and, if asked, the full-resolution RGB image (doc_benchmark.py:76)."""
    _chk(img_hwc, torch.uint8, "img")
    h, w, three = img_hwc.shape
    assert three == 3
    y = torch.empty((3, out_size, out_size), dtype=torch.float32, device=img_hwc.device)
    rgb_out = torch.empty_like(img_hwc) if (want_rgb and swap_rb) else None
    scratch = torch.empty(lib.raw().dvd_ingest_scratch_bytes(out_size), dtype=torch.uint8, device=img_hwc.device)
    lib.call("dvd_ingest_u8", ptr(img_hwc), h, w, int(swap_rb), ptr(y), out_size, ptr(rgb_out), ptr(scratch), stream_ptr())
    return (y, rgb_out if swap_rb else img_hwc) if want_rgb else y


def ingest_u8_ragged(imgs, swap_rb: bool = False, out_size: int = 512, want_rgb: bool = False):
    """n decoded images [h_d,w_d,3] uint8 of ANY sizes -> y [n,3,out,out] f32, y[d] the bits of ingest_u8(imgs[d]), in one
    launch per stage for the batch; with want_rgb also the list of full-resolution RGB images (the inputs themselves when
    swap_rb is off, views of one allocation otherwise)."""
    imgs = list(imgs)
    for d, im in enumerate(imgs):
        _chk(im, torch.uint8, f"imgs[{d}]")
        assert im.dim() == 3 and im.shape[2] == 3, f"imgs[{d}]: expected [H,W,3]"
    if not imgs:
        raise lib.DvdError("ingest_u8_ragged: no image (the device of the result is the images')")
    n, dev = len(imgs), imgs[0].device
    y = torch.empty((n, 3, out_size, out_size), dtype=torch.float32, device=dev)
    if want_rgb and swap_rb:
        rgbs = [o.view(im.shape) for o, im in zip(_carve([im.numel() for im in imgs], dev), imgs)]
    else:
        rgbs = [None] * n
    scratch = torch.empty(lib.raw().dvd_ingest_ragged_scratch_bytes(out_size, n), dtype=torch.uint8, device=dev)
    lib.call("dvd_ingest_u8_ragged", _ragged_table(imgs, rgbs), n, int(swap_rb), ptr(y), out_size, ptr(scratch), stream_ptr())
    return (y, rgbs if swap_rb else imgs) if want_rgb else y


def sched_step(coef: lib.SchedCoef, x_t, x0, noise=None, want_grid=False, out=None, clip=False):
    """clip=True is process_xstart's clamp fused in front (dvd_sched_step_clip): `x0` is clamped to [-1, 1] IN PLACE and
    the step (and the grid) are computed from the clamped value, in the one launch."""
    _chk(x_t, torch.float32, "x_t")
    _chk(x0, torch.float32, "x0")
    n, _, g, _ = x_t.shape
    if out is None:
        out = torch.empty_like(x_t)
    else:
        _chk(out, torch.float32, "out")
        assert out.shape == x_t.shape and out.data_ptr() != x_t.data_ptr()
    ngrid = torch.empty_like(x_t) if want_grid else None
    if noise is not None:
        _chk(noise, torch.float32, "noise")
    if clip and x0.data_ptr() in (x_t.data_ptr(), out.data_ptr(), None if noise is None else noise.data_ptr()):
        raise lib.DvdError("sched_step(clip=True) updates x0 in place: it must not share memory with x_t, noise or out")
    lib.call("dvd_sched_step_clip" if clip else "dvd_sched_step", C.byref(coef), ptr(x_t), ptr(x0), ptr(noise), ptr(out),
             ptr(ngrid), n, g, stream_ptr())
    return (out, ngrid) if want_grid else out


def hyp_mean_clamp(x0: torch.Tensor, n_hyp: int) -> torch.Tensor:
    _chk(x0, torch.float32, "x0")
    n, _, g, _ = x0.shape
    docs = n // n_hyp
    out = torch.empty((docs, 2, g, g), dtype=torch.float32, device=x0.device)
    lib.call("dvd_hyp_mean_clamp", ptr(x0), ptr(out), docs, n_hyp, g, stream_ptr())
    return out


def dither_f16(hi: torch.Tensor, lo: torch.Tensor, step: int, elem0: int = 0, out=None) -> torch.Tensor:
    """W = hi + lo (both f16) re-rounded to ONE f16 with the step-dependent sub-ulp offset of dvd_dither_f16."""
    _chk(hi, torch.float16, "hi")
    _chk(lo, torch.float16, "lo")
    if out is None:
        out = torch.empty_like(hi)
    lib.call("dvd_dither_f16", ptr(hi), ptr(lo), ptr(out), hi.numel(), C.c_uint(elem0 & 0xFFFFFFFF),
             C.c_uint(step & 0xFFFFFFFF), stream_ptr())
    return out


def selftest_mfma(a16, b16, vt16):
    out = torch.empty(3072, dtype=torch.float32, device=a16.device)
    lib.call("dvd_selftest_mfma", ptr(a16), ptr(b16), ptr(vt16), ptr(out), stream_ptr())
    return out


def _addr(t):
    return None if t is None else t.data_ptr()


def gemm_nt(a, b, *, out32=None, out16=None, bias=None, bias_row=False, act=0, pos=None, gate=None,
            gate_rows=0, res=None, batch=1, strides=None, M=None, N=None, K=None, lda=None, ldb=None, b_lo=None,
            a_lo=None, lo_scale=2.0 ** -11, small_tiles=False):
    """C = epi(A . B^T).  a [M,K] / b [N,K] f16 or f32 device tensors (2-D views may be strided in rows).
    strides: dict of batch strides in elements (A,B,C32,C16,bias,gate,res)."""
    assert a.dtype == b.dtype and a.dtype in (torch.float16, torch.float32)
    d = lib.GemmDesc()
    d.dtype = 1 if a.dtype == torch.float32 else 0
    d.M = M if M is not None else a.shape[-2]
    d.N = N if N is not None else b.shape[-2]
    d.K = K if K is not None else a.shape[-1]
    d.batch = batch
    st = strides or {}
    d.A, d.lda, d.strideA = _addr(a), (lda if lda is not None else a.stride(-2)), st.get("A", 0)
    d.B, d.ldb, d.strideB = _addr(b), (ldb if ldb is not None else b.stride(-2)), st.get("B", 0)
    if b_lo is not None:
        d.B_lo, d.lo_scale = _addr(b_lo), lo_scale
    if a_lo is not None:
        d.A_lo, d.lo_scale = _addr(a_lo), lo_scale
    if out32 is not None:
        d.C32, d.ldc, d.strideC32 = _addr(out32), out32.stride(-2), st.get("C32", 0)
    if out16 is not None:
        d.C16, d.ldc16, d.strideC16 = _addr(out16), out16.stride(-2), st.get("C16", 0)
    if bias is not None:
        d.bias, d.bias_row, d.strideBias = _addr(bias), int(bias_row), st.get("bias", 0)
    d.act = act
    if pos is not None:
        d.pos, d.ldpos, d.pos_rows = _addr(pos), pos.stride(-2), pos.shape[-2]
    if gate is not None:
        d.gate, d.ldgate, d.gate_rows, d.strideGate = _addr(gate), gate.stride(-2), gate_rows, st.get("gate", 0)
    if res is not None:
        d.res, d.ldres, d.strideRes = _addr(res), res.stride(-2), st.get("res", 0)
    d.small_tiles = int(small_tiles)
    lib.call("dvd_gemm_nt", C.byref(d), stream_ptr())


def flash_attn(q, k, vt, out, heads, head_dim, scale, kv_batch_div=1):
    """q [B,Tq,*] k [Bkv,Tk,*] (row-strided views ok), vt [Bkv, heads*hd, Tk], out [B,Tq,heads*hd]; all f16."""
    d = lib.AttnDesc()
    d.head_dim, d.heads, d.batch, d.tq, d.tk = head_dim, heads, q.shape[0], q.shape[1], k.shape[1]
    d.kv_batch_div = kv_batch_div
    d.Q, d.ldq, d.strideQ = q.data_ptr(), q.stride(1), q.stride(0)
    d.K, d.ldk, d.strideK = k.data_ptr(), k.stride(1), k.stride(0)
    d.Vt, d.ldvt, d.strideVt = vt.data_ptr(), vt.stride(1), vt.stride(0)
    d.O, d.ldo, d.strideO = out.data_ptr(), out.stride(1), out.stride(0)
    d.scale = scale
    lib.call("dvd_flash_attn", C.byref(d), stream_ptr())
    return out


# ---- token-side kernels (thin wrappers used by the parity tests; the engine calls them from C++) ----------------
def layernorm_rows(x, c, gamma=None, beta=None, shift=None, scale=None, mod_rows=1, eps=1e-6):
    rows = x.shape[0]
    out = torch.empty(rows, c, dtype=torch.float16, device=x.device)
    lib.call("dvd_layernorm_rows", ptr(x), x.stride(0), 0, ptr(out), c, 0, 1, rows, c, ptr(gamma), ptr(beta), ptr(shift),
             ptr(scale), (shift.stride(0) if shift is not None and shift.dim() > 1 else 0), mod_rows, C.c_float(eps),
             stream_ptr())
    return out


def dwconv3x3(x16, w9c, b, n, side):
    out = torch.empty_like(x16)
    lib.call("dvd_dwconv3x3", ptr(x16), ptr(out), ptr(w9c), ptr(b), n, side, x16.shape[-1], stream_ptr())
    return out


def embed_obs_ln(x, w, b, pos):
    n, _, g, _ = x.shape
    T = (g // 2) ** 2
    tok = torch.empty(n * T, 384, dtype=torch.float32, device=x.device)
    ln = torch.empty(n * T, 384, dtype=torch.float16, device=x.device)
    lib.call("dvd_embed_obs_ln", ptr(x), ptr(w), ptr(b), ptr(pos), ptr(tok), ptr(ln), n, g, stream_ptr())
    return tok, ln


def small_linear(x, w, b, act_in=0, act_out=0, kmod=None):
    m = x.shape[0]
    n, k = w.shape
    y = torch.empty(m, n, dtype=torch.float32, device=x.device)
    lib.call("dvd_small_linear", ptr(x), x.stride(0), ptr(w), ptr(b), ptr(y), n, m, k, n, kmod or k, act_in, act_out,
             stream_ptr())
    return y


def final_tokens(z, gamma, beta, shift, scale, w8, b8, init_flow, n, g):
    x0 = torch.empty(n, 2, g, g, dtype=torch.float32, device=z.device)
    tok8 = torch.empty(z.shape[0], 8, dtype=torch.float32, device=z.device)
    lib.call("dvd_final_tokens", ptr(z), ptr(gamma), ptr(beta), ptr(shift), ptr(scale), 0, z.shape[0], ptr(w8), ptr(b8),
             ptr(init_flow), ptr(x0), ptr(tok8), n, g, stream_ptr())
    return x0, tok8


def posenc(z, hs, ws, htab, wtab, n, side):
    c = z.shape[-1]
    chunks = 8
    part = torch.empty(n * chunks * c, dtype=torch.float32, device=z.device)
    pooled = torch.empty(n, c, dtype=torch.float32, device=z.device)
    lib.call("dvd_colmean", ptr(z), ptr(part), ptr(pooled), n, side * side, c, chunks, stream_ptr())
    lib.call("dvd_posenc_add", ptr(z), ptr(hs), ptr(ws), ptr(htab), ptr(wtab), n, side, c, stream_ptr())
    return pooled


def build_r_rows(feat_nhwc, flow, n_hyp, mode, init_feat=None):
    n, _, g, _ = flow.shape
    T = (g // 2) ** 2
    out = torch.empty(n * T, 1088, dtype=torch.float16, device=flow.device)
    lib.call("dvd_build_r_rows", ptr(feat_nhwc), ptr(init_feat), ptr(flow), ptr(out), 1088, n, g, n_hyp, mode, stream_ptr())
    return out


def conv3x3_relu_nhwc(x_nhwc, w_packed, bias, cin, cout, h, w):
    """One pyramid layer the way the engine runs it: im2col + exact-f32 GEMM (+bias, ReLU)."""
    kp = w_packed.shape[1]
    col = torch.empty(h * w, kp, dtype=torch.float32, device=x_nhwc.device)
    lib.call("dvd_im2col3x3", ptr(x_nhwc), 1, w * cin, cin, ptr(col), kp, cin, h, w, stream_ptr())
    out = torch.empty(h * w, cout, dtype=torch.float32, device=x_nhwc.device)
    gemm_nt(col, w_packed, out32=out, bias=bias, act=2)
    return out


def conv3x3_relu_nhwc_implicit(x_nhwc, w_packed, bias, cin, cout, h, w):
    """The same layer without the im2col matrix (cin % 16 == 0): what the engine runs for every pyramid layer but the first."""
    out = torch.empty(h * w, cout, dtype=torch.float32, device=x_nhwc.device)
    lib.call("dvd_conv3x3_nhwc", ptr(x_nhwc), cin, ptr(w_packed), w_packed.shape[1], ptr(bias), ptr(out), cout, h, w, 1,
             stream_ptr())
    return out


def maxpool2_nhwc(x, c, h, w):
    out = torch.empty((h // 2) * (w // 2), c, dtype=torch.float32, device=x.device)
    lib.call("dvd_maxpool2_nhwc", ptr(x), ptr(out), c, h, w, stream_ptr())
    return out


def resize_bilinear_nhwc(x, c, hin, win, hout, wout):
    out = torch.empty(hout * wout, c, dtype=torch.float32, device=x.device)
    lib.call("dvd_resize_bilinear_nhwc", ptr(x), ptr(out), c, hin, win, hout, wout, stream_ptr())
    return out


# ---- MS-SSIM against a ground-truth scan (dvd_amd/csrc/metrics.hip; definition: DESIGN.md 4.3) -----------------------------
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MSSSIM_MIN_SIDE = 176          # the fifth scale must still hold one full 11 x 11 window
MSSSIM_AREA = 598400           # working size of the DocUNet benchmark protocol, in pixels
_SSIM_PRESETS = dict(zip(run_options.METRIC_PRESETS, (lib.MSSSIM_DOCUNET, lib.MSSSIM_WANG)))


def _ssim_preset(preset, name):
    """The metric's preset: checked before anything is allocated or launched."""
    if preset not in _SSIM_PRESETS:
        raise ValueError(f"{name}: preset must be {either(_SSIM_PRESETS)}, got {preset!r}")
    return _SSIM_PRESETS[preset]


def _size_query(name, *args):
    """A byte count from the library (a negative value is a DVD_E_* status)."""
    nbytes = getattr(lib.raw(), name)(*args)
    if nbytes < 0:
        raise lib.DvdError(f"{name} failed ({nbytes}): {lib.raw().dvd_last_error().decode()}")
    return nbytes


def resize_gray_u8(img_nhwc_u8: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """[N,H,W,3] uint8 RGB -> [N,out_h,out_w] f32 gray (integers 0..255): anti-aliased triangle resize, one rounding to
    u8, round(0.2989 R + 0.5870 G + 0.1140 B) - the metric's preparation in one launch for the N images."""
    if img_nhwc_u8.dim() != 4 or img_nhwc_u8.shape[0] < 1 or img_nhwc_u8.shape[3] != 3:
        raise ValueError(f"resize_gray_u8: expected [N,H,W,3] with N >= 1, got {tuple(img_nhwc_u8.shape)}")
    n, h, w, _ = img_nhwc_u8.shape
    if min(h, w, out_h, out_w) < 1:
        raise ValueError(f"resize_gray_u8: bad shape {h}x{w} -> {out_h}x{out_w}")
    _chk(img_nhwc_u8, torch.uint8, "img")
    out = torch.empty((n, out_h, out_w), dtype=torch.float32, device=img_nhwc_u8.device)
    scratch = torch.empty(_size_query("dvd_resize_gray_scratch_bytes", h, w, out_h, out_w), dtype=torch.uint8,
                          device=img_nhwc_u8.device)
    lib.call("dvd_resize_gray_u8", ptr(img_nhwc_u8), n, h, w, ptr(out), out_h, out_w, ptr(scratch), stream_ptr())
    return out


def ssim_scales(x: torch.Tensor, y: torch.Tensor, preset: str = "docunet") -> torch.Tensor:
    """Gray planes x, y [N,H,W] f32 (0..255) of one size -> [N,5,2] f32: per scale (mean ssim, mean cs)."""
    flag = _ssim_preset(preset, "ssim_scales")
    if x.dim() != 3 or x.shape[0] < 1 or tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"ssim_scales: expected two [N,H,W] planes of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    n, h, w = x.shape
    if min(h, w) < MSSSIM_MIN_SIDE:
        raise ValueError(f"ssim_scales: each side must be >= {MSSSIM_MIN_SIDE} (five scales of an 11x11 window), got {h}x{w}")
    _chk(x, torch.float32, "x")
    _chk(y, torch.float32, "y")
    out = torch.empty((n, 5, 2), dtype=torch.float32, device=x.device)
    work = torch.empty(_size_query("dvd_msssim_workspace_bytes", h, w, n), dtype=torch.uint8, device=x.device)
    lib.call("dvd_msssim_scales", ptr(x), ptr(y), n, h, w, flag, ptr(work), ptr(out), stream_ptr())
    return out


def msssim_combine(scales, preset: str = "docunet") -> float:
    """The ten numbers of one document ([5][2]: per scale (ssim, cs)) -> MS-SSIM, in Python floats."""
    _ssim_preset(preset, "msssim_combine")
    s = [[float(v) for v in row] for row in scales]
    if preset == "wang":
        terms = [s[0][1], s[1][1], s[2][1], s[3][1], s[4][0]]
        if min(terms) < 0.0:                      # a negative mean has no real fractional power (numpy gives nan too)
            return float("nan")
        val = 1.0
        for t, wk in zip(terms, MSSSIM_WEIGHTS):
            val *= t ** wk
        return val
    return sum(wk * s[k][0] for k, wk in enumerate(MSSSIM_WEIGHTS))


def ms_ssim(x: torch.Tensor, y: torch.Tensor, preset: str = "docunet") -> np.ndarray:
    """MS-SSIM of N pairs of gray planes [N,H,W] -> [N] float64 (the per-scale numbers are combined on the host)."""
    scales = ssim_scales(x, y, preset).cpu().tolist()
    return np.array([msssim_combine(s, preset) for s in scales], dtype=np.float64)


def msssim_target_size(h: int, w: int, area: int = MSSSIM_AREA):
    """(rows, columns) the ground truth [h,w] is resized to: (round(h s), round(w s)), s = sqrt(area / (h w))."""
    s = (area / (h * w)) ** 0.5
    return int(round(h * s)), int(round(w * s))


def ms_ssim_u8(pred_hwc_u8: torch.Tensor, gt_hwc_u8: torch.Tensor, preset: str = "docunet", area: int = MSSSIM_AREA) -> float:
    """The whole protocol for one pair of uint8 RGB images [H,W,3] of any two sizes: the ground truth is resized to `area`
    pixels, the prediction to the ground truth's resized size, both go to gray, then MS-SSIM."""
    _ssim_preset(preset, "ms_ssim_u8")
    x, y = _metric_planes("ms_ssim_u8", pred_hwc_u8, gt_hwc_u8, area, MSSSIM_MIN_SIDE)
    return float(ms_ssim(x, y, preset)[0])


# ---- PNG of a dewarped page, encoded on the device (dvd_amd/csrc/png.hip; format: DESIGN.md 4.4) ------------------------------
def _rgb8_input(img, name):
    """(h, w) of an encoder's input, a contiguous uint8 [H,W,3] tensor: checked before anything is allocated or launched."""
    if not torch.is_tensor(img) or img.dim() != 3 or img.shape[2] != 3 or min(img.shape[:2]) < 1:
        raise ValueError(f"{name}: expected a [H,W,3] tensor, got {tuple(img.shape) if torch.is_tensor(img) else type(img)}")
    if img.dtype != torch.uint8 or not img.is_contiguous():
        raise ValueError(f"{name}: expected contiguous uint8, got {img.dtype} contiguous={img.is_contiguous()}")
    return int(img.shape[0]), int(img.shape[1])


def _scratch(scratch, need, dev, name):
    """The caller's optional scratch buffer, checked, or a fresh one of `need` bytes on `dev`."""
    if scratch is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need or scratch.device != dev:
        raise ValueError(f"{name}: scratch must be a contiguous uint8 buffer of >= {need} bytes on {dev}")
    return scratch


def _device_bytes_to_file(data, path):
    """Write a uint8 device tensor to `path`: only these bytes cross to the host.  Returns their number."""
    data = data.cpu().numpy()
    with open(path, "wb") as f:
        f.write(data.tobytes())
    return int(data.size)


def png_bound(h: int, w: int) -> int:
    """Worst-case bytes of the PNG file of an h x w RGB image (dvd_png_bound)."""
    return _size_query("dvd_png_bound", h, w)


PNG_HUFFMAN = dict(zip(run_options.PNG_HUFFMAN, (lib.PNG_HUFFMAN_FIXED, lib.PNG_HUFFMAN_DYNAMIC)))


def png_huffman_flag(huffman, name="png_encode"):
    """The library's DVD_PNG_HUFFMAN_* flag of 'fixed' | 'dynamic', or ValueError."""
    if not isinstance(huffman, str) or huffman not in PNG_HUFFMAN:
        raise ValueError(f"{name}: huffman must be {either(PNG_HUFFMAN)}, got {huffman!r}")
    return PNG_HUFFMAN[huffman]


def png_encode(img_hwc_u8: torch.Tensor, scratch: torch.Tensor = None, huffman: str = "fixed") -> torch.Tensor:
    """[H,W,3] uint8 on the device -> the complete PNG file as uint8 [nbytes] on the device: four launches, then ONE read-back
    (the file's length) to trim the worst-case buffer.  The bytes depend on (H, W, pixels, huffman) only.  huffman: 'fixed'
    (one fixed-Huffman block per segment) | 'dynamic' (per segment the smaller of a dynamic and the fixed block: never a longer
    file).  scratch (optional): a uint8 device buffer of at least dvd_png_scratch_bytes_huff(H, W, huffman) bytes to reuse
    between calls; its contents do not matter."""
    flag = png_huffman_flag(huffman)
    h, w = _rgb8_input(img_hwc_u8, "png_encode")
    if h * (3 * w + 1) >= 2 ** 31:
        raise ValueError(f"png_encode: image {h}x{w} too large (h * (3w + 1) must be below 2^31)")
    _chk(img_hwc_u8, torch.uint8, "img")
    dev = img_hwc_u8.device
    need = _size_query("dvd_png_scratch_bytes_huff", h, w, flag)
    scratch = _scratch(scratch, need, dev, "png_encode")
    cap = png_bound(h, w)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    nbytes = torch.zeros(1, dtype=torch.int64, device=dev)
    lib.call("dvd_png_encode_rgb8_huff", ptr(img_hwc_u8), h, w, ptr(out), cap, ptr(nbytes), ptr(scratch), flag, stream_ptr())
    return out[:int(nbytes.item())]


def png_encode_to_file(img_hwc_u8: torch.Tensor, path: str, huffman: str = "fixed") -> int:
    """Encode on the device and write `path`: only the compressed bytes cross to the host.  Returns the file's bytes."""
    return _device_bytes_to_file(png_encode(img_hwc_u8, huffman=huffman), path)


# ---- JPEG of a dewarped page, encoded on the device (dvd_amd/csrc/jpeg.hip; format: DESIGN.md 4.5) ----------------------------
JPEG_SUBSAMPLINGS = dict(zip(run_options.JPEG_SUBSAMPLINGS, (lib.JPEG_420, lib.JPEG_444)))


def jpeg_settings(quality, subsampling, name="jpeg_encode"):
    """(quality, the library's subsampling flag), or ValueError: quality an integer 1..100, subsampling '420' | '444'."""
    if not run_options.is_jpeg_quality(quality):
        raise ValueError(f"{name}: quality must be an integer 1..100, got {quality!r}")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"{name}: subsampling must be {either(JPEG_SUBSAMPLINGS)}, got {subsampling!r}")
    return int(quality), JPEG_SUBSAMPLINGS[subsampling]


def jpeg_bound(h: int, w: int, subsampling: str = "420") -> int:
    """Worst-case bytes of the JPEG file of an h x w RGB image (dvd_jpeg_bound)."""
    return _size_query("dvd_jpeg_bound", h, w, jpeg_settings(90, subsampling, "jpeg_bound")[1])


def jpeg_encode(img_hwc_u8: torch.Tensor, quality: int = 90, subsampling: str = "420", scratch: torch.Tensor = None) -> torch.Tensor:
    """[H,W,3] uint8 on the device -> the complete baseline JPEG file as uint8 [nbytes] on the device: four launches, then ONE
    read-back (the file's length) to trim the worst-case buffer.  The bytes depend on (H, W, pixels, quality, subsampling) only.
    The tensor's first byte may lie at any address.  scratch (optional): a uint8 device buffer of at least
    dvd_jpeg_scratch_bytes(H, W, subsampling) bytes to reuse between calls; its contents do not matter."""
    h, w = _rgb8_input(img_hwc_u8, "jpeg_encode")
    if max(h, w) > 65535 or 3 * (-(-h // 16) * 16) * (-(-w // 16) * 16) >= 2 ** 31:
        raise ValueError(f"jpeg_encode: image {h}x{w} too large (h, w <= 65535 and the padded planes below 2^31 bytes)")
    quality, flag = jpeg_settings(quality, subsampling)
    _chk(img_hwc_u8, torch.uint8, "img")
    dev = img_hwc_u8.device
    need = _size_query("dvd_jpeg_scratch_bytes", h, w, flag)
    scratch = _scratch(scratch, need, dev, "jpeg_encode")
    cap = _size_query("dvd_jpeg_bound", h, w, flag)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    nbytes = torch.zeros(1, dtype=torch.int64, device=dev)
    lib.call("dvd_jpeg_encode_rgb8", ptr(img_hwc_u8), h, w, quality, flag, ptr(out), cap, ptr(nbytes), ptr(scratch), stream_ptr())
    return out[:int(nbytes.item())]


def jpeg_encode_to_file(img_hwc_u8: torch.Tensor, path: str, quality: int = 90, subsampling: str = "420") -> int:
    """Encode on the device and write `path`: only the compressed bytes cross to the host.  Returns the file's bytes."""
    return _device_bytes_to_file(jpeg_encode(img_hwc_u8, quality, subsampling), path)


# ---- decoders for the input photograph and the ground-truth scans: JPEG (dvd_amd/csrc/jpegdec.hip; definition: DESIGN.md 4.6) and
# ---- PNG (dvd_amd/csrc/pngdec.hip; definition: DESIGN.md 4.9) ---------------------------------------------------------------
PNG_SIGNATURE = lib.PNG_SIGNATURE


class DecodeUnsupported(ValueError):
    """A device decoder hands the file back.  `code` is the name of the library's code.  A normal outcome: decode_image falls
    back to PIL."""

    def __init__(self, code: str, message: str):
        super().__init__(f"{code}: {message}")
        self.code = code


class JpegUnsupported(DecodeUnsupported):
    """A refusal of the host-side header check (progressive, 4 components, ...), or NOSYNC / DATA after the entropy decoder
    ran.  `code` names a DVD_E_JPEG_* code."""


class PngUnsupported(DecodeUnsupported):
    """A refusal of the host-side chunk check (interlace, palette, tRNS, ...), or DATA / NOSPLIT after the inflate ran.
    `code` names a DVD_E_PNG_* code."""


class _Codec(NamedTuple):
    """What tells the two decoders apart: the probe's struct (its name in lib), the library's entry points, the codes that
    mean 'handed back' and their exception, and the probe's fields that give the decoded image's height and width."""
    info: str
    probe: str
    decode: str
    codes: dict
    unsupported: type
    dims: tuple


_JPEG = _Codec("JpegDecInfo", "dvd_jpegdec_probe", "dvd_jpeg_decode_rgb8", lib.JPEG_DECODE_CODES, JpegUnsupported, ("out_h", "out_w"))
_PNG = _Codec("PngDecInfo", "dvd_pngdec_probe", "dvd_png_decode_rgb8", lib.PNG_DECODE_CODES, PngUnsupported, ("h", "w"))


def _image_file(data, name):
    """The file as (host uint8 array, the caller's device tensor or None)."""
    if torch.is_tensor(data):
        if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous 1-D uint8 tensor, got {data.dtype} {tuple(data.shape)}")
        host = data.cpu().numpy()
        dev = data if data.is_cuda else None
    elif isinstance(data, (bytes, bytearray, memoryview)):
        host, dev = np.frombuffer(bytearray(data), dtype=np.uint8), None   # a writable copy: torch.from_numpy takes it
    elif isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 1:
        host, dev = np.ascontiguousarray(data), None
    else:
        raise ValueError(f"{name}: expected bytes or a 1-D uint8 tensor, got {type(data)}")
    if host.size < 1:
        raise ValueError(f"{name}: an empty file")
    return host, dev


def _decode_status(codec, name, rc):
    if rc == 0:
        return
    message = lib.raw().dvd_last_error().decode()
    if rc in codec.codes:
        raise codec.unsupported(codec.codes[rc], message)
    raise lib.DvdError(f"{name} failed ({rc}): {message}")


def _probe(codec, host, name):
    info = getattr(lib, codec.info)()
    _decode_status(codec, name, getattr(lib.raw(), codec.probe)(C.c_void_p(host.ctypes.data), host.size, C.byref(info)))
    return info


def _fields(struct) -> dict:
    return {k: int(getattr(struct, k)) for k, _ in struct._fields_}


def _decode(codec, name, data, device, cap, cap_name, result, scratch, out):
    """What jpeg_decode and png_decode share: the file argument, the check of the cap (a positive integer or None), the probe,
    the file on the device, the scratch and `out` checks, the library call - which fills `result`, a ctypes object - and the
    [H,W,3] view of `out`."""
    host, dev_file = _image_file(data, name)
    if cap is not None and (isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 1):
        raise ValueError(f"{name}: {cap_name} must be a positive integer or None, got {cap!r}")
    info = _probe(codec, host, name)
    if dev_file is None:
        dev_file = torch.from_numpy(host).to(torch.device("cuda") if device is None else device)
    elif device is not None and torch.device(device) != dev_file.device:
        dev_file = dev_file.to(device)
    dev = dev_file.device
    _chk(dev_file, torch.uint8, "file")
    need, numel = int(info.scratch_bytes), 3 * info.h * info.w
    scratch = _scratch(scratch, need, dev, name)
    if out is None:
        out = torch.empty(numel, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < numel or out.device != dev:
        raise ValueError(f"{name}: out must be a contiguous uint8 tensor of >= {numel} elements on {dev}")
    with torch.cuda.device(dev):
        rc = getattr(lib.raw(), codec.decode)(C.c_void_p(host.ctypes.data), ptr(dev_file), host.size, ptr(out), out.numel(),
                                              0 if cap is None else int(cap), C.byref(result), ptr(scratch), stream_ptr())
    _decode_status(codec, codec.decode, rc)
    return out.view(-1)[:numel].view(*(getattr(info, k) for k in codec.dims), 3)


def jpeg_probe(data) -> dict:
    """What the decoder reads from the header of a JPEG file (bytes or a 1-D uint8 tensor), on the host: h, w, out_h, out_w
    (after the EXIF orientation), components, hs, vs, orientation, restart_interval, scan_offset, scan_bytes, blocks,
    scratch_bytes.  Raises JpegUnsupported for a file the device decoder refuses."""
    return _fields(_probe(_JPEG, _image_file(data, "jpeg_probe")[0], "jpeg_probe"))


def jpeg_decode(data, device=None, max_iters: int = None, scratch: torch.Tensor = None, out: torch.Tensor = None,
                return_iters: bool = False):
    """A baseline JPEG file (bytes or a 1-D uint8 tensor, on the host or already on the device) -> [H,W,3] uint8 RGB on the
    device with the EXIF orientation applied: the bytes ImageOps.exif_transpose(Image.open(f)).convert("RGB") gives.  Only
    the file crosses to the device.  max_iters caps the entropy decoder's fixpoint iterations (None: the library's 1024).
    scratch (optional): a uint8 device buffer of at least jpeg_probe(data)['scratch_bytes'] bytes to reuse between calls.
    out (optional): a contiguous uint8 device tensor of >= 3 H W elements, at any byte address, to decode into.
    return_iters: also return how many iterations ran.  Raises JpegUnsupported (a ValueError) for a file the decoder
    refuses, for 'NOSYNC' (max_iters reached) and for 'DATA' (the scan does not hold the header's blocks).  The call
    synchronises its stream (dvd_hip.h: every 16 iterations and once after the count pass)."""
    iters = C.c_int(0)
    img = _decode(_JPEG, "jpeg_decode", data, device, max_iters, "max_iters", iters, scratch, out)
    return (img, int(iters.value)) if return_iters else img


def jpeg_decode_from_file(path: str, device=None, max_iters: int = None) -> torch.Tensor:
    """Read `path` and decode it on the device (jpeg_decode)."""
    with open(path, "rb") as f:
        return jpeg_decode(f.read(), device=device, max_iters=max_iters)


def pil_decode_rgb8(path_or_bytes) -> np.ndarray:
    """The host decoder every route falls back to: PIL, EXIF orientation applied, RGB, [H,W,3] uint8."""
    import io
    from PIL import Image, ImageOps
    src = path_or_bytes if isinstance(path_or_bytes, (str, os.PathLike)) else io.BytesIO(bytes(path_or_bytes))
    im = ImageOps.exif_transpose(Image.open(src))
    return np.array(im.convert("RGB"), dtype=np.uint8)       # a writable, contiguous copy


def png_probe(data) -> dict:
    """What the decoder reads from the chunks of a PNG file (bytes or a 1-D uint8 tensor), on the host: h, w, colour_type,
    bpp, idat_chunks, payload_bytes, scratch_bytes.  Raises PngUnsupported for a file the device decoder refuses."""
    return _fields(_probe(_PNG, _image_file(data, "png_probe")[0], "png_probe"))


def png_decode(data, device=None, max_work: int = None, scratch: torch.Tensor = None, out: torch.Tensor = None,
               return_stats: bool = False):
    """A PNG file (bytes or a 1-D uint8 tensor, on the host or already on the device) -> [H,W,3] uint8 RGB on the device:
    the bytes ImageOps.exif_transpose(Image.open(f)).convert("RGB") gives.  Only the file crosses to the device.
    max_work caps the symbols + stored bytes one lane of the inflate may spend (None: the library's 2^20).
    scratch (optional): a uint8 device buffer of at least png_probe(data)['scratch_bytes'] bytes to reuse between calls.
    out (optional): a contiguous uint8 device tensor of >= 3 H W elements, at any byte address, to decode into.
    return_stats: also return {'candidates', 'segments', 'rounds', 'bands'}.  Raises PngUnsupported (a ValueError) for a
    file the decoder refuses, for 'DATA' (damaged data, a checksum mismatch) and for 'NOSPLIT' (max_work reached); `out` is
    untouched then.  The call synchronises its stream (dvd_hip.h says where)."""
    stats = lib.PngDecStats()
    img = _decode(_PNG, "png_decode", data, device, max_work, "max_work", stats, scratch, out)
    return (img, _fields(stats)) if return_stats else img


def png_decode_from_file(path: str, device=None, max_work: int = None) -> torch.Tensor:
    """Read `path` and decode it on the device (png_decode)."""
    with open(path, "rb") as f:
        return png_decode(f.read(), device=device, max_work=max_work)


def decode_image(path_or_bytes, device=None, max_iters: int = None, log=None, png: bool = False):
    """An image file (a path, bytes or a 1-D uint8 tensor) -> ([H,W,3] uint8 RGB on the device, the route that ran): 'hip'
    = the device decoder, 'pil' = PIL on the host plus an upload of the pixels, for every file the device decoder hands back
    (JpegUnsupported / PngUnsupported) - with ONE line to `log` (default: dvd_amd.logger.info) that names the reason.  The
    pixels are the same on both routes.  png=True sends a file that starts with the PNG signature to png_decode; by default
    only the JPEG decoder is tried (which hands a PNG file back as 'HEADER')."""
    if isinstance(path_or_bytes, (str, os.PathLike)):
        with open(path_or_bytes, "rb") as f:
            data, what = f.read(), str(path_or_bytes)
    else:
        data = path_or_bytes.cpu().numpy().tobytes() if torch.is_tensor(path_or_bytes) else bytes(path_or_bytes)
        what = f"<{len(data)} bytes>"
    try:
        if png and data[:8] == PNG_SIGNATURE:
            return png_decode(data, device=device), "hip"
        return jpeg_decode(data, device=device, max_iters=max_iters), "hip"
    except (JpegUnsupported, PngUnsupported) as e:
        if log is None:
            from . import logger
            log = logger.info
        log(f"{what}: decoded by PIL, not on the device: {e}")
    pixels = torch.from_numpy(pil_decode_rgb8(data))
    return pixels.to(torch.device("cuda") if device is None else device), "pil"


# ---- local distortion: dense SIFT + SIFT-flow (dvd_amd/csrc/sflow.hip; definition: DESIGN.md 4.7) --------------------------
SFLOW_DEFAULTS = dict(lib.SFLOW_DEFAULTS)
SFLOW_MAX_SIDE = 8192


def sflow_top_size(h: int, w: int, levels: int):
    """(rows, columns) of the top pyramid level: ceil(n / 2) per axis and level."""
    for _ in range(levels - 1):
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def sflow_params(name: str = "sift_flow", **params) -> lib.SflowParams:
    """The chain's parameters (defaults: SFLOW_DEFAULTS) as the C struct; every range is checked here, before anything is
    allocated or launched, and again by the library."""
    unknown = sorted(set(params) - set(SFLOW_DEFAULTS))
    if unknown:
        raise ValueError(f"{name}: unknown parameter(s) {unknown}; known: {sorted(SFLOW_DEFAULTS)}")
    p = dict(SFLOW_DEFAULTS, **params)
    for key, value in p.items():
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError(f"{name}: {key} must be an integer, got {value!r}")
    if not 1 <= p["levels"] <= 6:
        raise ValueError(f"{name}: levels must be 1..6, got {p['levels']}")
    for key in ("w_top", "w"):
        if not 1 <= p[key] <= 10:
            raise ValueError(f"{name}: {key} must be 1..10, got {p[key]}")
    for key in ("iters_top", "iters"):
        if not 1 <= p[key] <= 1000:
            raise ValueError(f"{name}: {key} must be 1..1000, got {p[key]}")
    if not 0 <= p["alpha"] <= 65535:
        raise ValueError(f"{name}: alpha must be 0..65535, got {p['alpha']}")
    if not 0 <= 2 * p["d"] <= 65535:
        raise ValueError(f"{name}: d must keep a message in 16 bits (0 <= 2 d <= 65535), got {p['d']}")
    bound = p["w_top"]
    for _ in range(p["levels"] - 1):
        bound = 2 * bound + p["w"]
    if p["gamma"] < 0 or p["T"] < 0 or p["T"] + 2 * p["gamma"] * bound > 65535:
        raise ValueError(f"{name}: T and gamma must keep a cost in 16 bits (T + gamma |f|_1 <= 65535 with |f|_1 <= "
                         f"{2 * bound}), got T {p['T']}, gamma {p['gamma']}")
    if not 1 <= p["eps"] <= 1 << 30:
        raise ValueError(f"{name}: eps must be 1..2^30, got {p['eps']}")
    return lib.SflowParams(**{k: int(v) for k, v in p.items()})


def _sflow_check_size(name, h, w, pr):
    th_, tw_ = sflow_top_size(h, w, pr.levels)
    if min(th_, tw_) < lib.SFLOW_MIN_TOP or max(h, w) > SFLOW_MAX_SIDE:
        raise ValueError(f"{name}: {h}x{w} with {pr.levels} levels has a top level of {th_}x{tw_}: each side must be >= "
                         f"{lib.SFLOW_MIN_TOP} (and no side above {SFLOW_MAX_SIDE})")


def dense_sift_u8(gray: torch.Tensor, eps: int = SFLOW_DEFAULTS["eps"]) -> torch.Tensor:
    """Gray planes [N,H,W] f32 of integer values 0..255 -> dense descriptors [N,H,W,128] uint8."""
    if gray.dim() != 3 or gray.shape[0] < 1 or min(gray.shape[1:]) < 1 or max(gray.shape[1:]) > SFLOW_MAX_SIDE:
        raise ValueError(f"dense_sift_u8: expected [N,H,W] with N >= 1 and sides 1..{SFLOW_MAX_SIDE}, got {tuple(gray.shape)}")
    if isinstance(eps, bool) or not isinstance(eps, (int, np.integer)) or not 1 <= eps <= 1 << 30:
        raise ValueError(f"dense_sift_u8: eps must be an integer 1..2^30, got {eps!r}")
    _chk(gray, torch.float32, "gray")
    n, h, w = gray.shape
    out = torch.empty((n, h, w, 128), dtype=torch.uint8, device=gray.device)
    lib.call("dvd_dsift_u8", ptr(gray), n, h, w, int(eps), ptr(out), stream_ptr())
    return out


def _sflow_level_args(name, desc_a, desc_b, off, win):
    if desc_a.dim() != 3 or desc_a.shape[2] != 128 or tuple(desc_a.shape) != tuple(desc_b.shape):
        raise ValueError(f"{name}: expected two [H,W,128] descriptor planes of one shape, got {tuple(desc_a.shape)} and "
                         f"{tuple(desc_b.shape)}")
    h, w = desc_a.shape[:2]
    if tuple(off.shape) != (2, h, w):
        raise ValueError(f"{name}: off must be [2,{h},{w}], got {tuple(off.shape)}")
    if isinstance(win, bool) or not isinstance(win, (int, np.integer)) or not 1 <= win <= 10:
        raise ValueError(f"{name}: win must be an integer 1..10, got {win!r}")
    _chk(desc_a, torch.uint8, "desc_a")
    _chk(desc_b, torch.uint8, "desc_b")
    _chk(off, torch.int16, "off")
    return h, w


def sflow_cost(desc_a: torch.Tensor, desc_b: torch.Tensor, off: torch.Tensor, win: int, **params) -> torch.Tensor:
    """The cost volume of one level of one document: descriptors [H,W,128] uint8, window centres off [2,H,W] int16 ->
    [H,W,(2 win + 1)^2] as int32 values 0..65535 (the kernel's u16)."""
    pr = sflow_params("sflow_cost", **params)
    h, w = _sflow_level_args("sflow_cost", desc_a, desc_b, off, win)
    cost = torch.empty((h, w, (2 * win + 1) ** 2), dtype=torch.int16, device=desc_a.device)
    lib.call("dvd_sflow_cost", ptr(desc_a), ptr(desc_b), ptr(off), h, w, int(win), C.byref(pr), ptr(cost), stream_ptr())
    return cost.to(torch.int32) & 0xFFFF


def sflow_level(desc_a: torch.Tensor, desc_b: torch.Tensor, off: torch.Tensor, win: int, iters: int, **params) -> torch.Tensor:
    """One level of one document: cost volume, `iters` BP iterations, argmin -> the absolute flow [2,H,W] int16."""
    pr = sflow_params("sflow_level", **params)
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= iters <= 1000:
        raise ValueError(f"sflow_level: iters must be an integer 1..1000, got {iters!r}")
    h, w = _sflow_level_args("sflow_level", desc_a, desc_b, off, win)
    flow = torch.empty((2, h, w), dtype=torch.int16, device=desc_a.device)
    work = torch.empty(_size_query("dvd_sflow_level_workspace_bytes", h, w, int(win)), dtype=torch.uint8, device=desc_a.device)
    lib.call("dvd_sflow_level", ptr(desc_a), ptr(desc_b), ptr(off), h, w, int(win), int(iters), C.byref(pr), ptr(work),
             ptr(flow), None, stream_ptr())
    return flow


def sift_flow(a: torch.Tensor, b: torch.Tensor, **params):
    """SIFT-flow from the gray planes a (the scan) to b (the prediction), [N,H,W] f32 of integer values 0..255 ->
    (flow int16 [N,2,H,W], ld float64 [N]: the mean flow length of every pair).  The documents of a batch follow each other
    in one document's workspace."""
    pr = sflow_params("sift_flow", **params)
    if a.dim() != 3 or a.shape[0] < 1 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"sift_flow: expected two [N,H,W] planes of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, h, w = a.shape
    _sflow_check_size("sift_flow", h, w, pr)
    _chk(a, torch.float32, "a")
    _chk(b, torch.float32, "b")
    flow = torch.empty((n, 2, h, w), dtype=torch.int16, device=a.device)
    ld = torch.empty((n,), dtype=torch.float64, device=a.device)
    work = torch.empty(_size_query("dvd_sflow_workspace_bytes", h, w, C.byref(pr)), dtype=torch.uint8, device=a.device)
    lib.call("dvd_sflow", ptr(a), ptr(b), n, h, w, C.byref(pr), ptr(work), ptr(flow), ptr(ld), stream_ptr())
    return flow, ld.cpu().numpy()


def local_distortion(a: torch.Tensor, b: torch.Tensor, **params) -> np.ndarray:
    """LD of N pairs of gray planes [N,H,W] -> [N] float64."""
    return sift_flow(a, b, **params)[1]


def _metric_size(name, pred_hwc_u8, gt_hwc_u8, area, min_side):
    """The working size of the benchmark's preparation, (rows, columns): the ground truth resized to `area` pixels."""
    for who, t in (("pred", pred_hwc_u8), ("gt", gt_hwc_u8)):
        if t.dim() != 3 or t.shape[2] != 3 or min(t.shape[:2]) < 1:
            raise ValueError(f"{name}: {who}: expected [H,W,3], got {tuple(t.shape)}")
    if area < 1:
        raise ValueError(f"{name}: area must be positive, got {area}")
    th_, tw_ = msssim_target_size(gt_hwc_u8.shape[0], gt_hwc_u8.shape[1], area)
    if min(th_, tw_) < min_side:
        raise ValueError(f"{name}: the working size {th_}x{tw_} has a side below {min_side}")
    return th_, tw_


def _metric_planes(name, pred_hwc_u8, gt_hwc_u8, area, min_side, pr=None):
    """The benchmark's preparation, shared by MS-SSIM and LD: the ground truth resized to `area` pixels, the prediction to the
    ground truth's resized size, both to gray -> (pred plane, gt plane), each [1,h,w] f32.  pr: the SIFT-flow parameters the
    working size must suit."""
    th_, tw_ = _metric_size(name, pred_hwc_u8, gt_hwc_u8, area, min_side)
    if pr is not None:
        _sflow_check_size(name, th_, tw_, pr)
    _chk(pred_hwc_u8, torch.uint8, "pred")
    _chk(gt_hwc_u8, torch.uint8, "gt")
    return resize_gray_u8(pred_hwc_u8[None], th_, tw_), resize_gray_u8(gt_hwc_u8[None], th_, tw_)


def ld_u8(pred_hwc_u8: torch.Tensor, gt_hwc_u8: torch.Tensor, area: int = MSSSIM_AREA, **params) -> float:
    """LD for one pair of uint8 RGB images [H,W,3] of any two sizes, prepared like ms_ssim_u8: the flow runs from the
    ground-truth scan to the prediction."""
    pr = sflow_params("ld_u8", **params)
    x, y = _metric_planes("ld_u8", pred_hwc_u8, gt_hwc_u8, area, 1, pr)
    return float(local_distortion(y, x, **params)[0])


# ---- aligned distortion (the AD kernels of dvd_amd/csrc/sflow.hip; definition: DESIGN.md 4.8) --------------------------------
def _ad_planes(name, t, dtype, what, lead=()):
    """[N,*lead,H,W] with N >= 1 and sides 1..8192 -> (n, h, w)"""
    if t.dim() != 3 + len(lead) or t.shape[0] < 1 or tuple(t.shape[1:1 + len(lead)]) != tuple(lead) or min(t.shape[-2:]) < 1 \
            or max(t.shape[-2:]) > SFLOW_MAX_SIDE:
        shape = ",".join(["N"] + [str(v) for v in lead] + ["H", "W"])
        raise ValueError(f"{name}: {what}: expected [{shape}] with N >= 1 and sides 1..{SFLOW_MAX_SIDE}, got {tuple(t.shape)}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: {what} must be {dtype}, got {t.dtype}")
    return t.shape[0], t.shape[-2], t.shape[-1]


def ad_fit(flow: torch.Tensor):
    """The least-squares translation and scale per axis of flow fields [N,2,H,W] int16 -> (sums int64 [N,4] = (sum f_u,
    sum X f_u, sum f_v, sum Y f_v) with X = 2x - (W-1), Y = 2y - (H-1); coef int32 [N,4] = (ax, bx, ay, by) in Q16), both on the
    device."""
    n, h, w = _ad_planes("ad_fit", flow, torch.int16, "flow", (2,))
    _chk(flow, torch.int16, "flow")
    sums = torch.empty((n, 4), dtype=torch.int64, device=flow.device)
    coef = torch.empty((n, 4), dtype=torch.int32, device=flow.device)
    scratch = torch.empty((-(-h * w // 256) * 4,), dtype=torch.int64, device=flow.device)
    lib.call("dvd_ad_fit", ptr(flow), n, h, w, ptr(scratch), ptr(sums), ptr(coef), stream_ptr())
    return sums, coef


def ad_align(b: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """Gray planes b [N,H,W] f32 of integer values 0..255 resampled through the fitted maps coef [N,4] int32 (ad_fit's, read
    on the device) -> [N,H,W] f32 of integer values."""
    n, h, w = _ad_planes("ad_align", b, torch.float32, "b")
    if tuple(coef.shape) != (n, 4) or coef.dtype != torch.int32:
        raise ValueError(f"ad_align: coef must be int32 [{n},4], got {coef.dtype} {tuple(coef.shape)}")
    _chk(b, torch.float32, "b")
    _chk(coef, torch.int32, "coef")
    out = torch.empty_like(b)
    lib.call("dvd_ad_align", ptr(b), ptr(coef), n, h, w, ptr(out), stream_ptr())
    return out


def ad_weighted(a: torch.Tensor, flow: torch.Tensor) -> np.ndarray:
    """The mean length of flow [N,2,H,W] int16 weighted by the gradient magnitude of the gray planes a [N,H,W] f32 -> float64
    [N] (the plain mean for a plane without a gradient)."""
    n, h, w = _ad_planes("ad_weighted", a, torch.float32, "a")
    if tuple(flow.shape) != (n, 2, h, w) or flow.dtype != torch.int16:
        raise ValueError(f"ad_weighted: flow must be int16 [{n},2,{h},{w}], got {flow.dtype} {tuple(flow.shape)}")
    _chk(a, torch.float32, "a")
    _chk(flow, torch.int16, "flow")
    ad = torch.empty((n,), dtype=torch.float64, device=a.device)
    scratch = torch.empty((-(-h * w // 256) * 3,), dtype=torch.int64, device=a.device)
    lib.call("dvd_ad_weighted", ptr(a), ptr(flow), n, h, w, ptr(scratch), ptr(ad), stream_ptr())
    return ad.cpu().numpy()


def aligned_distortion(a: torch.Tensor, b: torch.Tensor, intermediates: bool = False, **params):
    """AD and LD of N pairs of gray planes a (the scan), b (the prediction), [N,H,W] f32 of integer values 0..255 ->
    (ad float64 [N], ld float64 [N]); ld is the first pass's, the value sift_flow gives.  intermediates=True adds a dict of
    device tensors: flow1, flow2 int16 [N,2,H,W], sums int64 [N,4], coef int32 [N,4], aligned f32 [N,H,W].  The two flows, the
    fit, the resampling and the weighted mean are enqueued together; the only read-back is the 16 N bytes at the end."""
    pr = sflow_params("aligned_distortion", **params)
    if a.dim() != 3 or a.shape[0] < 1 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"aligned_distortion: expected two [N,H,W] planes of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, h, w = a.shape
    _sflow_check_size("aligned_distortion", h, w, pr)
    _chk(a, torch.float32, "a")
    _chk(b, torch.float32, "b")
    dev = a.device
    res = torch.empty((2, n), dtype=torch.float64, device=dev)          # ld, ad
    extra = {}
    if intermediates:
        extra = dict(flow1=torch.empty((n, 2, h, w), dtype=torch.int16, device=dev), sums=torch.empty((n, 4), dtype=torch.int64, device=dev),
                     coef=torch.empty((n, 4), dtype=torch.int32, device=dev), aligned=torch.empty((n, h, w), dtype=torch.float32, device=dev),
                     flow2=torch.empty((n, 2, h, w), dtype=torch.int16, device=dev))
    work = torch.empty(_size_query("dvd_adist_workspace_bytes", h, w, C.byref(pr)), dtype=torch.uint8, device=dev)
    lib.call("dvd_adist", ptr(a), ptr(b), n, h, w, C.byref(pr), ptr(work), ptr(res[0]), ptr(res[1]),
             *[ptr(extra.get(k)) for k in ("flow1", "sums", "coef", "aligned", "flow2")], stream_ptr())
    host = res.cpu().numpy()
    return (host[1], host[0], extra) if intermediates else (host[1], host[0])


def ad_u8(pred_hwc_u8: torch.Tensor, gt_hwc_u8: torch.Tensor, area: int = MSSSIM_AREA, **params) -> float:
    """AD for one pair of uint8 RGB images [H,W,3] of any two sizes, prepared like ms_ssim_u8 and ld_u8: the flows run from
    the ground-truth scan to the prediction."""
    pr = sflow_params("ad_u8", **params)
    x, y = _metric_planes("ad_u8", pred_hwc_u8, gt_hwc_u8, area, 1, pr)
    return float(aligned_distortion(y, x, **params)[0][0])


GT_METRIC_NAMES = tuple(kind.name for kind in run_options.SCORES if kind.switch is None)     # ms_ssim, ld, ad


def gt_metrics_u8(pred_hwc_u8: torch.Tensor, gt_hwc_u8: torch.Tensor, metrics, preset: str = "docunet",
                  area: int = MSSSIM_AREA, **params) -> dict:
    """The metrics named in `metrics` ('ms_ssim', 'ld', 'ad') for one pair of uint8 RGB images, on planes prepared once:
    {name: float}.  Each value is what ms_ssim_u8 / ld_u8 / ad_u8 gives alone; with 'ld' and 'ad' the chain runs once and LD is
    its first pass's."""
    metrics = tuple(metrics)
    unknown = [m for m in metrics if m not in GT_METRIC_NAMES]
    if unknown or not metrics:
        raise ValueError(f"gt_metrics_u8: metrics must name 'ms_ssim', 'ld' and / or 'ad', got {metrics!r}")
    _ssim_preset(preset, "gt_metrics_u8")
    pr = sflow_params("gt_metrics_u8", **params)
    flows = "ld" in metrics or "ad" in metrics
    x, y = _metric_planes("gt_metrics_u8", pred_hwc_u8, gt_hwc_u8, area, MSSSIM_MIN_SIDE if "ms_ssim" in metrics else 1,
                          pr if flows else None)
    out = {}
    if "ms_ssim" in metrics:
        out["ms_ssim"] = float(ms_ssim(x, y, preset)[0])
    if "ad" in metrics:
        ad, ld = aligned_distortion(y, x, **params)
        out["ad"] = float(ad[0])
        if "ld" in metrics:
            out["ld"] = float(ld[0])
    elif "ld" in metrics:
        out["ld"] = float(local_distortion(y, x, **params)[0])
    return {m: out[m] for m in GT_METRIC_NAMES if m in out}


# ---- common corruptions of the network input (dvd_amd/csrc/corrupt.hip; definition: DESIGN.md 4.10, tests/corrupt_model.py) -----
CORRUPTIONS = ("gaussian_noise", "shot_noise", "impulse_noise", "defocus_blur", "glass_blur", "motion_blur", "zoom_blur", "snow",
               "frost", "fog", "brightness", "contrast", "elastic_transform", "pixelate", "jpeg_compression", "speckle_noise",
               "gaussian_blur", "spatter", "saturate")
CORRUPT_JPEG = CORRUPTIONS.index("jpeg_compression")
CORRUPT_JPEG_QUALITY = (25, 18, 15, 10, 7)
CORRUPT_MIN_SIDE, CORRUPT_MAX_SIDE = 32, 16384


class CorruptionUnsupported(ValueError):
    """A corruption of the benchmark's list that has no device kernel here.  `kind` is its number, `name` its name."""

    def __init__(self, kind):
        self.kind, self.name = kind, CORRUPTIONS[kind]
        super().__init__(f"corruption {kind} ({self.name}): no device kernel")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def corruption_number(kind, name="corruption_number") -> int:
    """The number 0..18 of a corruption given by number or by name, or ValueError naming `name`."""
    if isinstance(kind, str):
        if kind not in CORRUPTIONS:
            raise ValueError(f"{name} must be one of {', '.join(CORRUPTIONS)}, got {kind!r}")
        return CORRUPTIONS.index(kind)
    if not _is_int(kind) or not 0 <= kind < len(CORRUPTIONS):
        raise ValueError(f"{name} must be an integer 0..{len(CORRUPTIONS) - 1} or a corruption's name, got {kind!r}")
    return int(kind)


def corruption_severity(severity, name="severity") -> int:
    """The severity 0..5 (0: nothing is corrupted), or ValueError naming `name`."""
    if not _is_int(severity) or not 0 <= severity <= 5:
        raise ValueError(f"{name} must be an integer 0..5, got {severity!r}")
    return int(severity)


def corruption_supported(kind) -> bool:
    """Whether corrupt_rgb8 delivers the kind (number or name)."""
    return lib.raw().dvd_corrupt_supported(corruption_number(kind, "kind")) != 0


def corruption_key(seed, path):
    """The 64-bit key of one document's corruption: (seed & 0xffffffff, crc32(path)).  It names the document, not its place in
    a batch."""
    import zlib
    if not _is_int(seed):
        raise ValueError(f"corruption_key: seed must be an integer, got {seed!r}")
    return int(seed) & 0xffffffff, zlib.crc32(str(path).encode())


def unit_to_rgb8(y_nchw: torch.Tensor) -> torch.Tensor:
    """The network input y [B,3,h,w] f32 = k / 255 -> its bytes [B,h,w,3] uint8: clamp(rint(255 y), 0, 255)."""
    if not torch.is_tensor(y_nchw) or y_nchw.dim() != 4 or y_nchw.shape[1] != 3:
        raise ValueError(f"unit_to_rgb8: expected a [B,3,h,w] tensor, got {tuple(y_nchw.shape) if torch.is_tensor(y_nchw) else type(y_nchw)}")
    _chk(y_nchw, torch.float32, "y")
    n, _, h, w = (int(v) for v in y_nchw.shape)
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=y_nchw.device)
    lib.call("dvd_unit_to_rgb8", ptr(y_nchw), ptr(out), n, h, w, stream_ptr())
    return out


def rgb8_to_unit(img_nhwc_u8: torch.Tensor) -> torch.Tensor:
    """Bytes [B,h,w,3] uint8 -> y [B,3,h,w] f32 = k / 255, the correctly rounded division of ingest_u8."""
    if not torch.is_tensor(img_nhwc_u8) or img_nhwc_u8.dim() != 4 or img_nhwc_u8.shape[3] != 3:
        raise ValueError("rgb8_to_unit: expected a [B,h,w,3] tensor, got "
                         f"{tuple(img_nhwc_u8.shape) if torch.is_tensor(img_nhwc_u8) else type(img_nhwc_u8)}")
    _chk(img_nhwc_u8, torch.uint8, "img")
    n, h, w, _ = (int(v) for v in img_nhwc_u8.shape)
    out = torch.empty(n, 3, h, w, dtype=torch.float32, device=img_nhwc_u8.device)
    lib.call("dvd_rgb8_to_unit", ptr(img_nhwc_u8), ptr(out), n, h, w, stream_ptr())
    return out


def corrupt_rgb8(img_u8: torch.Tensor, kind, severity, key) -> torch.Tensor:
    """[h,w,3] or [B,h,w,3] uint8 on the device -> the corrupted image(s), a new tensor of the same shape.  kind: a number 0..18
    or a name of CORRUPTIONS; severity 1..5; key: (k0, k1) of 32 bits each for one image, a sequence of B such pairs for a
    batch (corruption_key).  The result is a function of (bytes, kind, severity, key) only: an image in a batch gives what it
    gives alone.  One launch; jpeg_compression goes through jpeg_encode / jpeg_decode per image.  Every argument is checked
    before anything is launched; a kind without a kernel raises CorruptionUnsupported."""
    kind = corruption_number(kind, "corrupt_rgb8: kind")
    if not _is_int(severity) or not 1 <= severity <= 5:
        raise ValueError(f"corrupt_rgb8: severity must be an integer 1..5, got {severity!r}")
    if not corruption_supported(kind):
        raise CorruptionUnsupported(kind)
    if not torch.is_tensor(img_u8) or img_u8.dim() not in (3, 4) or img_u8.shape[-1] != 3:
        raise ValueError("corrupt_rgb8: expected a [h,w,3] or [B,h,w,3] tensor, got "
                         f"{tuple(img_u8.shape) if torch.is_tensor(img_u8) else type(img_u8)}")
    if img_u8.dtype != torch.uint8 or not img_u8.is_contiguous():
        raise ValueError(f"corrupt_rgb8: expected contiguous uint8, got {img_u8.dtype} contiguous={img_u8.is_contiguous()}")
    single = img_u8.dim() == 3
    batch = img_u8[None] if single else img_u8
    n, h, w = (int(v) for v in batch.shape[:3])
    if not (CORRUPT_MIN_SIDE <= min(h, w) and max(h, w) <= CORRUPT_MAX_SIDE):
        raise ValueError(f"corrupt_rgb8: image {h}x{w}: every side must be {CORRUPT_MIN_SIDE}..{CORRUPT_MAX_SIDE}")
    if not 1 <= n <= 65535:
        raise ValueError(f"corrupt_rgb8: a batch of {n} images (1..65535)")
    keys = np.asarray([key] if single else key)
    if keys.shape != (n, 2) or keys.dtype.kind not in "iu" or keys.min() < 0 or keys.max() > 0xffffffff:
        raise ValueError(f"corrupt_rgb8: key must be {'a pair' if single else f'{n} pairs'} of integers below 2^32, got {key!r}")
    _chk(img_u8, torch.uint8, "img")
    if kind == CORRUPT_JPEG:
        quality = CORRUPT_JPEG_QUALITY[severity - 1]
        out = torch.stack([jpeg_decode(jpeg_encode(im, quality, "420")) for im in batch])
    else:
        out = torch.empty_like(batch)
        keys_dev = torch.from_numpy(keys.astype(np.uint32).view(np.int32)).to(img_u8.device)
        lib.call("dvd_corrupt_rgb8", ptr(batch), ptr(out), n, h, w, kind, int(severity), ptr(keys_dev), stream_ptr())
    return out[0] if single else out


# ---- keyed sampler noise and the map deviation (dvd_amd/csrc/noise.hip; definition: DESIGN.md 4.11, tests/noise_model.py) --------
NOISE_MIN_GRID, NOISE_MAX_GRID = 2, 8192
MAP_DEV_PX = 0.987 * 511          # pixels of the 512 x 512 network input per unit of flow


def noise_keys(keys, docs=None, name="noise_keys"):
    """A sequence of (k0, k1) pairs of 32-bit integers (corruption_key) as an int64 array [docs, 2], or ValueError naming
    `name`: not a sequence of pairs, a value outside 0 .. 2^32 - 1, or - where `docs` is given - another length."""
    try:
        arr = np.asarray(list(keys))
    except (TypeError, ValueError):                # no sequence, or pairs of different lengths
        arr = np.asarray(None)
    if arr.ndim == 1 and arr.size == 0:            # no document
        arr = np.zeros((0, 2), np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind not in "iu" or (arr.size and (arr.min() < 0 or arr.max() > 0xffffffff)):
        raise ValueError(f"{name} must be a sequence of (k0, k1) pairs of integers below 2^32, got {keys!r}")
    if docs is not None and arr.shape[0] != docs:
        raise ValueError(f"{name} must hold one (k0, k1) pair per document: {docs}, got {arr.shape[0]}")
    return arr.astype(np.int64)


def noise_keys_tensor(keys, device, docs=None, name="noise_keys") -> torch.Tensor:
    """The keys on the device as randn_keyed takes them ([docs, 2] int32 holding the 32-bit patterns): one small copy, so a
    sampling loop uploads its keys once."""
    arr = noise_keys(keys, docs, name)
    return torch.from_numpy(arr.astype(np.uint32).view(np.int32)).to(device)


def randn_keyed(keys, n_hyp: int, g: int, slot: int, device=None, out: torch.Tensor = None) -> torch.Tensor:
    """Standard normals [docs*n_hyp, 2, g, g] f32 keyed per document: sample doc * n_hyp + h is a function of (keys[doc], h, slot,
    element) only - not of the batch, of the order of the documents or of torch's generator.  keys: a sequence of (k0, k1) pairs
    (corruption_key), or what noise_keys_tensor made of one.  slot 0 is x_T, slot 1 + i the noise of step index i.  out: a
    contiguous f32 device tensor of that shape, filled in place and returned.  One launch."""
    if not _is_int(n_hyp) or not 0 <= n_hyp <= 65535:
        raise ValueError(f"randn_keyed: n_hyp must be an integer 0..65535, got {n_hyp!r}")
    if not _is_int(g) or not NOISE_MIN_GRID <= g <= NOISE_MAX_GRID:
        raise ValueError(f"randn_keyed: g must be an integer {NOISE_MIN_GRID}..{NOISE_MAX_GRID}, got {g!r}")
    if not _is_int(slot) or not 0 <= slot <= 0xffffffff:
        raise ValueError(f"randn_keyed: slot must be an integer 0..2^32-1, got {slot!r}")
    if torch.is_tensor(keys):
        if keys.dim() != 2 or keys.shape[1] != 2 or keys.dtype != torch.int32 or not keys.is_contiguous():
            raise ValueError(f"randn_keyed: a key tensor must be contiguous [docs, 2] int32 (noise_keys_tensor), got {tuple(keys.shape)} {keys.dtype}")
        keys_dev = keys
        device = keys.device if device is None else torch.device(device)
    else:
        arr = noise_keys(keys, name="randn_keyed: keys")
        device = torch.device("cuda" if device is None else device)
        keys_dev = torch.from_numpy(arr.astype(np.uint32).view(np.int32)).to(device)
    docs = int(keys_dev.shape[0])
    if docs > 65535 or docs * int(n_hyp) * ((2 * g * g + 3) // 4) > 1 << 38:
        raise ValueError(f"randn_keyed: {docs} documents x {n_hyp} hypotheses at g = {g} (65535 documents and 2^38 quads at most)")
    shape = (docs * int(n_hyp), 2, int(g), int(g))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    elif not torch.is_tensor(out) or tuple(out.shape) != shape:
        raise ValueError(f"randn_keyed: out must be a tensor of shape {shape}, got {tuple(out.shape) if torch.is_tensor(out) else type(out)}")
    if out.numel() == 0:
        return out
    _chk(keys_dev, torch.int32, "keys")
    _chk(out, torch.float32, "out")
    if out.device != keys_dev.device:
        raise ValueError(f"randn_keyed: out is on {out.device}, the keys on {keys_dev.device}")
    lib.call("dvd_randn_keyed", ptr(keys_dev), docs, int(n_hyp), int(g), int(slot), ptr(out), stream_ptr())
    return out


def map_deviation(a: torch.Tensor, b: torch.Tensor) -> list:
    """Two stacks of maps [docs,2,g,g] f32 on the device -> per document MAP_DEV_PX * mean over the g^2 grid points of
    sqrt(dx^2 + dy^2): how far, in pixels of the 512 x 512 network input, b samples from where a does.  f32 distances, an f64
    sum in a fixed order: equal maps give exactly 0.0, and a document in a batch gives what it gives alone.  One read-back."""
    for t, name in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 2 or t.shape[2] != t.shape[3]:
            raise ValueError(f"map_deviation: {name} must be a [docs,2,g,g] tensor, got {tuple(t.shape) if torch.is_tensor(t) else type(t)}")
    if a.shape != b.shape:
        raise ValueError(f"map_deviation: a is {tuple(a.shape)}, b is {tuple(b.shape)}")
    docs, g = int(a.shape[0]), int(a.shape[2])
    if docs > 65535 or not NOISE_MIN_GRID <= g <= NOISE_MAX_GRID:
        raise ValueError(f"map_deviation: {docs} documents at g = {g} (65535 documents at most, g {NOISE_MIN_GRID}..{NOISE_MAX_GRID})")
    if docs == 0:
        return []
    _chk(a, torch.float32, "a")
    _chk(b, torch.float32, "b")
    if a.device != b.device:
        raise ValueError(f"map_deviation: a is on {a.device}, b on {b.device}")
    ws = torch.empty(_size_query("dvd_map_deviation_workspace_bytes", docs, g) // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(docs, dtype=torch.float64, device=a.device)
    lib.call("dvd_map_deviation", ptr(a), ptr(b), docs, g, ptr(out), ptr(ws), stream_ptr())
    return [float(v) for v in out.cpu()]


# ---- flow pictures and .flo files of a predicted map (dvd_amd/csrc/flowviz.hip; definition: DESIGN.md 4.12, tests/flowviz_model.py)
FLOW_NORMS = {"diag": lib.FLOW_NORM_DIAG, "max": lib.FLOW_NORM_MAX}
FLOW_MAX_SIDE, FLOW_MAX_IMAGES = 16384, 65535
FLO_TAG = 202021.25               # the f32 that opens a Middlebury .flo file ('PIEH' as bytes)


def _flow_norm(norm, name):
    if not isinstance(norm, str) or norm not in FLOW_NORMS:
        raise ValueError(f"{name}: norm must be {either(FLOW_NORMS)}, got {norm!r}")
    return FLOW_NORMS[norm]


def _flow_clip(clip_flow, name):
    """clip_flow as the library takes it: None -> -1 (no clip), otherwise a finite number >= 0."""
    if clip_flow is None:
        return -1.0
    if isinstance(clip_flow, bool) or not isinstance(clip_flow, (int, float, np.integer, np.floating)) \
            or not np.isfinite(clip_flow) or clip_flow < 0:
        raise ValueError(f"{name}: clip_flow must be None or a finite number >= 0, got {clip_flow!r}")
    return float(clip_flow)


def _flow_size(h, w, n, name):
    if not _is_int(h) or not _is_int(w) or not 1 <= h <= FLOW_MAX_SIDE or not 1 <= w <= FLOW_MAX_SIDE:
        raise ValueError(f"{name}: h and w must be integers 1..{FLOW_MAX_SIDE}, got {h!r} x {w!r}")
    if n > FLOW_MAX_IMAGES:
        raise ValueError(f"{name}: {n} images ({FLOW_MAX_IMAGES} at most)")
    return int(h), int(w)


def _flow_field(field, name):
    """(the field as [n,h,w,2], n, h, w, whether it came as [h,w,2]) of a displacement field, checked."""
    if not torch.is_tensor(field) or field.dim() not in (3, 4) or field.shape[-1] != 2:
        raise ValueError(f"{name}: expected a [H,W,2] or [N,H,W,2] tensor, got {tuple(field.shape) if torch.is_tensor(field) else type(field)}")
    single = field.dim() == 3
    n = 1 if single else int(field.shape[0])
    h, w = _flow_size(int(field.shape[-3]), int(field.shape[-2]), n, name)
    if field.dtype != torch.float32 or not field.is_contiguous():
        raise ValueError(f"{name}: expected contiguous float32, got {field.dtype} contiguous={field.is_contiguous()}")
    return field, n, h, w, single


def _flow_coarse(flow, name):
    """(n, g, whether it came as [2,g,g]) of a coarse map [n,2,g,g] or [2,g,g], checked."""
    if not torch.is_tensor(flow) or flow.dim() not in (3, 4) or flow.shape[-3] != 2 or flow.shape[-1] != flow.shape[-2]:
        raise ValueError(f"{name}: expected a [2,G,G] or [N,2,G,G] tensor, got {tuple(flow.shape) if torch.is_tensor(flow) else type(flow)}")
    g = int(flow.shape[-1])
    if not NOISE_MIN_GRID <= g <= NOISE_MAX_GRID:
        raise ValueError(f"{name}: G must be {NOISE_MIN_GRID}..{NOISE_MAX_GRID}, got {g}")
    if flow.dtype != torch.float32 or not flow.is_contiguous():
        raise ValueError(f"{name}: expected contiguous float32, got {flow.dtype} contiguous={flow.is_contiguous()}")
    return (1 if flow.dim() == 3 else int(flow.shape[0])), g, flow.dim() == 3


def _flow_workspace(n, h, w, dev):
    """(largest [n] f32, ws) for norm 'max'."""
    ws = torch.empty(max(_size_query("dvd_flow_workspace_bytes", n, h, w) // 4, 1), dtype=torch.float32, device=dev)
    return torch.empty(n, dtype=torch.float32, device=dev), ws


def flow_radius_max(flow: torch.Tensor, clip_flow=None) -> torch.Tensor:
    """A displacement field [N,H,W,2] (or [H,W,2]) f32 in pixels on the device -> [N] (or a 0-d) f32 tensor: per image the largest
    sqrt(u^2 + v^2) over its pixels with finite components, after the clip - rad_max of norm 'max' less its 1e-5.  Two launches
    in a fixed order without atomics: the value is a function of the field alone."""
    clip = _flow_clip(clip_flow, "flow_radius_max")
    field, n, h, w, single = _flow_field(flow, "flow_radius_max")
    _chk(field, torch.float32, "flow")
    out, ws = _flow_workspace(n, h, w, field.device)
    if n:
        lib.call("dvd_flow_radius_max", ptr(field), n, h, w, C.c_float(clip), ptr(out), ptr(ws), stream_ptr())
    return out[0] if single else out


def flow_to_image(flow: torch.Tensor, clip_flow=None, convert_to_bgr: bool = False, norm: str = "diag") -> torch.Tensor:
    """datasets/utils/flow_viz.py flow_to_image on the device: a displacement field [H,W,2] (or [N,H,W,2]) f32 in pixels ->
    the colour-wheel picture [H,W,3] (or [N,H,W,3]) uint8.  norm 'diag' (the reference): rad_max = sqrt((W//2)^2 + (H//2)^2) +
    1e-5; 'max' (the Middlebury rule): the image's largest radius + 1e-5.  clip_flow as the reference has it: both components
    clipped to [0, clip_flow].  A pixel with a non-finite component is black."""
    code = _flow_norm(norm, "flow_to_image")
    clip = _flow_clip(clip_flow, "flow_to_image")
    field, n, h, w, single = _flow_field(flow, "flow_to_image")
    _chk(field, torch.float32, "flow")
    out = torch.empty((h, w, 3) if single else (n, h, w, 3), dtype=torch.uint8, device=field.device)
    if n == 0:
        return out
    largest, ws = _flow_workspace(n, h, w, field.device) if norm == "max" else (None, None)
    lib.call("dvd_flow_to_image_rgb8", ptr(field), n, h, w, code, C.c_float(clip), int(bool(convert_to_bgr)), ptr(out), ptr(largest),
             ptr(ws), stream_ptr())
    return out


def flow_full_uv(flow: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """The coarse map [N,2,G,G] (or [2,G,G]) f32 -> its full-resolution pixel displacement [N,h,w,2] (or [h,w,2]) f32:
    F.interpolate(flow, (h, w), bilinear, align_corners=True) in the arithmetic of the unwarp tail, then u = s_x (w - 1),
    v = s_y (h - 1).  The payload of a .flo file.  One launch."""
    n, g, single = _flow_coarse(flow, "flow_full_uv")
    h, w = _flow_size(h, w, n, "flow_full_uv")
    _chk(flow, torch.float32, "flow")
    out = torch.empty((h, w, 2) if single else (n, h, w, 2), dtype=torch.float32, device=flow.device)
    if n:
        lib.call("dvd_flow_full_uv", ptr(flow), n, g, h, w, ptr(out), stream_ptr())
    return out


def flow_picture(flow: torch.Tensor, h: int, w: int, norm: str = "diag", convert_to_bgr: bool = False, return_radius: bool = False):
    """The coarse map [N,2,G,G] (or [2,G,G]) -> its picture [N,h,w,3] (or [h,w,3]) uint8 in ONE pass: the bytes of
    flow_to_image(flow_full_uv(flow, h, w), norm=norm) without the 8 B/px field ever being written.  return_radius: also the
    [N] (or 0-d) f32 tensor of flow_radius_max of that field (norm 'max' only; None otherwise)."""
    code = _flow_norm(norm, "flow_picture")
    n, g, single = _flow_coarse(flow, "flow_picture")
    h, w = _flow_size(h, w, n, "flow_picture")
    _chk(flow, torch.float32, "flow")
    out = torch.empty((h, w, 3) if single else (n, h, w, 3), dtype=torch.uint8, device=flow.device)
    largest, ws = _flow_workspace(n, h, w, flow.device) if norm == "max" else (None, None)
    if n:
        lib.call("dvd_flow_picture_rgb8", ptr(flow), n, g, h, w, code, int(bool(convert_to_bgr)), ptr(out), ptr(largest), ptr(ws),
                 stream_ptr())
    if not return_radius:
        return out
    return out, (None if largest is None else (largest[0] if single else largest))


def _one_map(flow, name):
    n, _, single = _flow_coarse(flow, name)
    if n != 1:
        raise ValueError(f"{name}: one map per file, got {n}")
    return flow if single else flow[0]


def flow_picture_to_file(flow: torch.Tensor, h: int, w: int, path: str, norm: str = "max", huffman: str = "fixed",
                         return_radius: bool = False):
    """The picture of ONE coarse map [2,G,G] (or [1,2,G,G]) as a PNG file: flow_picture, then png_encode_to_file - only the
    compressed file crosses to the host.  Returns the file's bytes; with return_radius (the file's bytes, the largest radius as
    a float or None)."""
    png_huffman_flag(huffman, "flow_picture_to_file")
    img, largest = flow_picture(_one_map(flow, "flow_picture_to_file"), h, w, norm=norm, return_radius=True)
    nbytes = png_encode_to_file(img, path, huffman)
    return (nbytes, None if largest is None else float(largest)) if return_radius else nbytes


def flo_write(field, path: str) -> int:
    """A host field [h,w,2] float32 as a Middlebury .flo file: the f32 tag 202021.25, int32 w, int32 h, then h w interleaved
    (u, v) f32, little endian.  Returns the file's bytes."""
    field = np.asarray(field)
    if field.ndim != 3 or field.shape[2] != 2 or min(field.shape[:2]) < 1 or field.dtype != np.float32:
        raise ValueError(f"flo_write: expected a [h,w,2] float32 array, got {field.shape} {field.dtype}")
    h, w = field.shape[:2]
    with open(path, "wb") as f:
        f.write(np.asarray([FLO_TAG], "<f4").tobytes())
        f.write(np.asarray([w, h], "<i4").tobytes())
        f.write(field.astype("<f4", copy=False).tobytes())
    return 12 + field.nbytes


def flow_write_flo(flow: torch.Tensor, h: int, w: int, path: str) -> int:
    """The full-resolution displacement of ONE coarse map [2,G,G] (or [1,2,G,G]), flow_full_uv, as a Middlebury .flo file
    (flo_write).  Returns the file's bytes."""
    return flo_write(flow_full_uv(_one_map(flow, "flow_write_flo"), h, w).cpu().numpy(), path)


def flow_read_flo(path: str) -> np.ndarray:
    """A Middlebury .flo file -> the field [h,w,2] float32 (host).  A wrong tag, size or length is a ValueError naming the file."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or np.frombuffer(data, "<f4", 1)[0] != np.float32(FLO_TAG):
        raise ValueError(f"{path}: not a .flo file (it does not open with the tag {FLO_TAG})")
    w, h = (int(v) for v in np.frombuffer(data, "<i4", 2, 4))
    if h < 1 or w < 1 or len(data) != 12 + 8 * h * w:
        raise ValueError(f"{path}: a .flo file of {w} x {h} holds {12 + 8 * max(h, 0) * max(w, 0)} bytes, this one {len(data)}")
    return np.frombuffer(data, "<f4", 2 * h * w, 12).reshape(h, w, 2).astype(np.float32)


# ---- the map score: a predicted map against a ground-truth map (dvd_amd/csrc/mapscore.hip; definition: DESIGN.md 4.13,
# tests/mapscore_model.py)
MAP_MAX_SIDE, MAP_MAX_HYP, MAP_RANKS = 16384, 64, 50
MAP_INTERVALS = 50                  # the reference's compute_aucs(intervals=50)
MAP_INVALID = -1                    # the planes' int32 value at a pixel that enters nothing (the bit pattern 0xffffffff)
MAP_CURVES = ("EPE", "PCK1", "PCK5")
MAP_NO_PIXELS = {"EPE": 0.0, "PCK1": 1.0, "PCK5": 1.0}
MAP_FIX_SCALE = 1048576.0           # the fixed point of the curves' sums: rint(min(e, 2^15) 2^20)


def _map_device(t, shape_text, name, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name}: {what} must be a {shape_text} float32 tensor on the device, got "
                         f"{t.device if torch.is_tensor(t) else type(t)}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous float32, got {t.dtype} contiguous={t.is_contiguous()}")


def _map_args(flow, gt, hyps, size, name):
    """(g, gt_g, n_hyp, h, w) of a scoring call, every shape checked: no launch follows a bad one."""
    _map_device(flow, "[2,G,G] or [h,w,2]", name, "flow")
    field = flow.dim() == 3 and flow.shape[2] == 2 and tuple(flow.shape) != (2, 2, 2)       # [2,2,2] is the coarse map G = 2
    if not field and (flow.dim() != 3 or flow.shape[0] != 2 or flow.shape[1] != flow.shape[2]
                      or not NOISE_MIN_GRID <= flow.shape[1] <= NOISE_MAX_GRID):
        raise ValueError(f"{name}: flow must be a coarse map [2,G,G] with G {NOISE_MIN_GRID}..{NOISE_MAX_GRID} or a field [h,w,2], "
                         f"got {tuple(flow.shape)}")
    g = 0 if field else int(flow.shape[1])
    _map_device(gt, "[h,w,2] or [2,g,g]", name, "gt")
    if gt.device != flow.device:
        raise ValueError(f"{name}: flow is on {flow.device}, gt on {gt.device}")
    if size is None:
        if gt.dim() != 3 or gt.shape[2] != 2:
            raise ValueError(f"{name}: gt must be a displacement field [h,w,2] (or, with size=(h, w), a coarse map [2,g,g]), got {tuple(gt.shape)}")
        h, w, gt_g = int(gt.shape[0]), int(gt.shape[1]), 0
    else:
        if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(v) for v in size):
            raise ValueError(f"{name}: size must be (h, w), got {size!r}")
        h, w = int(size[0]), int(size[1])
        if gt.dim() != 3 or gt.shape[0] != 2 or gt.shape[1] != gt.shape[2] or not NOISE_MIN_GRID <= gt.shape[1] <= NOISE_MAX_GRID:
            raise ValueError(f"{name}: with size given gt must be a coarse map [2,g,g], g {NOISE_MIN_GRID}..{NOISE_MAX_GRID}, got {tuple(gt.shape)}")
        gt_g = int(gt.shape[1])
    if not 1 <= h <= MAP_MAX_SIDE or not 1 <= w <= MAP_MAX_SIDE:
        raise ValueError(f"{name}: h and w must be 1..{MAP_MAX_SIDE}, got {h} x {w}")
    if field and (tuple(flow.shape) != (h, w, 2) or hyps is not None):
        raise ValueError(f"{name}: a field as flow must be [{h},{w},2] like the ground truth and comes without hyps, got {tuple(flow.shape)}")
    n_hyp = 1
    if hyps is not None:
        _map_device(hyps, "[H,2,G,G]", name, "hyps")
        if hyps.dim() != 4 or tuple(hyps.shape[1:]) != (2, g, g) or not 1 <= hyps.shape[0] <= MAP_MAX_HYP:
            raise ValueError(f"{name}: hyps must be [H,2,{g},{g}] with H 1..{MAP_MAX_HYP}, got {tuple(hyps.shape)}")
        if hyps.device != flow.device:
            raise ValueError(f"{name}: flow is on {flow.device}, hyps on {hyps.device}")
        n_hyp = int(hyps.shape[0])
    return g, gt_g, n_hyp, h, w


def _map_workspace(h, w, dev):
    """(ws, e [h,w], sigma [h,w]): the planes are the last two parts of the workspace."""
    total = _size_query("dvd_mapscore_workspace_bytes", h, w)
    plane = (4 * h * w + 255) & ~255
    ws = torch.empty(total, dtype=torch.uint8, device=dev)
    e = ws[total - 2 * plane:total - 2 * plane + 4 * h * w].view(torch.float32).view(h, w)
    sigma = ws[total - plane:total - plane + 4 * h * w].view(torch.float32).view(h, w)
    return ws, e, sigma


def _map_errors(flow, gt, hyps, size, name):
    g, gt_g, n_hyp, h, w = _map_args(flow, gt, hyps, size, name)
    ws, e, sigma = _map_workspace(h, w, flow.device)
    lib.call("dvd_map_errors", ptr(flow), g, ptr(gt), gt_g, ptr(hyps) if n_hyp >= 2 else None, n_hyp, h, w, ptr(e), ptr(sigma), ptr(ws),
             stream_ptr())
    return ws, e, sigma, n_hyp, h, w


def map_errors(flow: torch.Tensor, gt: torch.Tensor, hyps: torch.Tensor = None, size=None):
    """The planes of one document: flow [2,G,G] (the predicted map; or its displacement field [h,w,2]) against gt - a displacement field [h,w,2] in pixels, the
    layout of a .flo file, or with size=(h, w) a coarse map [2,g,g] - both evaluated at h x w with flow_full_uv's arithmetic.
    Returns (e, sigma), [h,w] f32 each: the end-point error and the spread sqrt(mean_h |d_h - mean|^2) of the hypotheses hyps
    [H,2,G,G] (0 without them or with H = 1).  A pixel whose ground truth is not finite or exceeds 1e9 in a component (or whose
    prediction is not finite) holds the bit pattern 0xffffffff in both planes and enters nothing.  One launch."""
    _, e, sigma, _, _, _ = _map_errors(flow, gt, hyps, size, "map_errors")
    return e, sigma


def _map_metrics(ws, h, w):
    out = torch.empty(7, dtype=torch.int64, device=ws.device)
    lib.call("dvd_map_metrics", ptr(ws), h, w, ptr(out), stream_ptr())
    words = out.cpu().numpy()
    n, n1, n3, n5, nfl = (int(v) for v in words[:5])
    se, se2 = (float(v) for v in words[5:].view(np.float64))
    nan = float("nan")
    if n == 0:
        return {"epe": nan, "epe_std": nan, "pck1": nan, "pck3": nan, "pck5": nan, "fl": nan, "n_valid": 0, "sum_e": 0.0, "sum_e2": 0.0}
    var = max(se2 - se * se / n, 0.0) / (n - 1) if n > 1 else nan
    return {"epe": se / n, "epe_std": float(np.sqrt(var)), "pck1": n1 / n, "pck3": n3 / n, "pck5": n5 / n, "fl": nfl / n,
            "n_valid": n, "sum_e": se, "sum_e2": se2}


def map_metrics(flow: torch.Tensor, gt: torch.Tensor, hyps: torch.Tensor = None, size=None) -> dict:
    """The headline numbers of one document (arguments as map_errors), the reference's definitions over the valid pixels: epe
    (mean of e), epe_std (unbiased, torch.std), pck1 / pck3 / pck5 (share with e <= 1, 3, 5 px), fl (share with e > 3 and
    e / |gt| > 0.05), n_valid, and the f64 sums sum_e, sum_e2 they come from (added in a fixed order; counts are exact).
    Two launches, one read-back of seven words."""
    ws, _, _, _, h, w = _map_errors(flow, gt, hyps, size, "map_metrics")
    return _map_metrics(ws, h, w)


def _map_plane(t, name, what):
    _map_device(t, "[n]", name, what)
    n = int(t.numel())
    if not 1 <= n <= MAP_MAX_SIDE * MAP_MAX_SIDE:
        raise ValueError(f"{name}: {what} must hold 1..{MAP_MAX_SIDE * MAP_MAX_SIDE} values, got {n}")
    return n


def _map_head(dev):
    """The part of the workspace that the selection and the bins use: one size for every plane."""
    return torch.empty(_size_query("dvd_mapscore_workspace_bytes", 1, 1), dtype=torch.uint8, device=dev)


def _map_bins(e, key, thr, ws):
    k = int(thr.numel())
    out = torch.empty((k + 1, 4), dtype=torch.int64, device=e.device)
    lib.call("dvd_sparsify_bins", ptr(e), ptr(key), int(e.numel()), ptr(thr), k, ptr(out), ptr(ws), stream_ptr())
    return out


def map_valid_count(e: torch.Tensor, ws=None) -> int:
    """How many pixels of a plane of map_errors are valid: the bins kernel with one threshold above every valid key."""
    _map_plane(e, "map_valid_count", "e")
    thr = torch.full((1,), 0x7fffffff, dtype=torch.int32, device=e.device)        # above every non-negative float, below invalid
    return int(_map_bins(e, e, thr, _map_head(e.device) if ws is None else ws)[1, 0])


def select_kth_desc(keys: torch.Tensor, ranks, n_valid: int = None, ws=None) -> torch.Tensor:
    """keys: a plane of non-negative finite f32 on the device (invalid pixels: the pattern 0xffffffff) -> the f32 tensor
    keys_sorted_descending[ranks] over its valid values.  ranks: 1..50 integers in 0..n_valid-1, in any order, repeats allowed.
    Exact: an MSD radix selection on the bit patterns, all ranks at once, eight launches and no read-back."""
    n = _map_plane(keys, "select_kth_desc", "keys")
    ranks = list(ranks) if isinstance(ranks, (list, tuple, np.ndarray)) else None
    if not ranks or len(ranks) > MAP_RANKS or not all(_is_int(r) for r in ranks):
        raise ValueError(f"select_kth_desc: ranks must be 1..{MAP_RANKS} integers, got {ranks!r}")
    ws = _map_head(keys.device) if ws is None else ws
    if n_valid is None:
        n_valid = map_valid_count(keys, ws)
    if not _is_int(n_valid) or not 1 <= n_valid <= n or min(ranks) < 0 or max(ranks) >= n_valid:
        raise ValueError(f"select_kth_desc: ranks must lie in 0..n_valid-1 with n_valid 1..{n}, got n_valid = {n_valid!r}, "
                         f"ranks {min(ranks)}..{max(ranks)}")
    asc = sorted({int(n_valid) - 1 - int(r) for r in ranks})
    out = torch.empty(len(asc), dtype=torch.float32, device=keys.device)
    host = (C.c_uint32 * len(asc))(*asc)
    lib.call("dvd_select_u32", ptr(keys), n, host, len(asc), ptr(out), ptr(ws), stream_ptr())
    if len(asc) == len(ranks) and all(int(n_valid) - 1 - int(r) == a for r, a in zip(reversed(ranks), asc)):
        return out.flip(0)                                       # distinct ranks in ascending order: the common case
    return out[torch.tensor([asc.index(int(n_valid) - 1 - int(r)) for r in ranks], device=keys.device)]


def map_ranks(n_valid: int, intervals: int = MAP_INTERVALS):
    """hi = ceil(q (N - 1) / 100) for q = 0, 100 / intervals, ..: the descending rank whose key closes the kept set of q."""
    return [(q * (n_valid - 1) + 99) // 100 for q in range(0, 100, 100 // intervals)]


def _map_curves(bins):
    """[51,4] integer bins (host) -> {metric: 51 float64 values}: suffix sums give the kept sets; the value for no pixel is
    appended as the reference appends it."""
    kept = np.cumsum(bins[::-1].astype(np.uint64), axis=0, dtype=np.uint64)[::-1][1:]
    cnt = kept[:, 0].astype(np.float64)
    vals = {"EPE": kept[:, 3].astype(np.float64) / MAP_FIX_SCALE / cnt, "PCK1": kept[:, 1] / cnt, "PCK5": kept[:, 2] / cnt}
    return {m: np.append(vals[m], MAP_NO_PIXELS[m]) for m in MAP_CURVES}


def sparsification(e: torch.Tensor, sigma: torch.Tensor, n_valid: int = None) -> dict:
    """The reference's compute_aucs(intervals=50) from the planes of map_errors: for q = 0, 2, .., 98 the kept set is
    {p : key(p) <= key_desc[ceil(q (N - 1) / 100)]}, all ties kept; key = sigma gives sparse_curve, key = e the oracle's
    opt_curve, each {EPE, PCK1, PCK5: 51 values} over max(opt) + 1e-6 with 0, 1, 1 appended; AUSE = |trapz(sparse) - trapz(opt)|.
    The thresholds are selected and the kept sets summed on the device in integers (e as rint(min(e, 2^15) 2^20)); the 153
    numbers are made on the host in float64.  The reference's np.percentile keeps one pixel more where its float32 interpolation
    rounds down onto the lower order statistic."""
    n = _map_plane(e, "sparsification", "e")
    if _map_plane(sigma, "sparsification", "sigma") != n or sigma.device != e.device:
        raise ValueError(f"sparsification: e holds {n} values on {e.device}, sigma {sigma.numel()} on {sigma.device}")
    ws = _map_head(e.device)
    if n_valid is None:
        n_valid = map_valid_count(e, ws)
    if not _is_int(n_valid) or not 1 <= n_valid <= n:
        raise ValueError(f"sparsification: n_valid must be 1..{n} (a plane without a valid pixel has no curve), got {n_valid!r}")
    ranks = map_ranks(int(n_valid))
    bins = [_map_bins(e, key, select_kth_desc(key, ranks, n_valid, ws).view(torch.int32), ws) for key in (sigma, e)]
    sparse, opt = (_map_curves(b.view(np.uint64)) for b in torch.stack(bins).cpu().numpy())
    k = len(ranks)
    plotx = np.asarray([1.0 / k * t for t in range(k + 1)], np.float64)
    out = {"sparse_curve": {}, "opt_curve": {}, "AUSE": {}}
    for m in MAP_CURVES:
        top = np.asarray(opt[m]).max() + 1e-6
        area = [float(((y[1:] + y[:-1]) * 0.5 * np.diff(plotx)).sum()) for y in (sparse[m] / top, opt[m] / top)]
        out["AUSE"][m] = abs(area[0] - area[1])
        out["sparse_curve"][m], out["opt_curve"][m] = sparse[m] / top, opt[m] / top
    return out


def map_score(flow: torch.Tensor, gt: torch.Tensor, hyps: torch.Tensor = None, size=None) -> dict:
    """Everything of one document (arguments as map_errors): map_metrics' numbers and, with H >= 2 hypotheses and a valid pixel,
    sparsification's sparse_curve, opt_curve and AUSE plus ause_epe, ause_pck1, ause_pck5.  A map scored against the .flo file
    written from it gives epe == 0.0 exactly."""
    ws, e, sigma, n_hyp, h, w = _map_errors(flow, gt, hyps, size, "map_score")
    out = _map_metrics(ws, h, w)
    if n_hyp >= 2 and out["n_valid"] > 0:
        sp = sparsification(e, sigma, out["n_valid"])
        out.update(sp)
        out.update({f"ause_{m.lower()}": sp["AUSE"][m] for m in MAP_CURVES})
    return out


# ---- the map inverse: mesh overlay, point transfer, fold count (dvd_amd/csrc/mapinv.hip; definition: DESIGN.md 4.14,
# tests/mapinv_model.py)
INV_MAX_SIDE, INV_MAX_POINTS = 16384, 1 << 28
INV_STATS = ("covered", "fold_px", "flipped_tris", "degenerate_tris", "skipped_tris", "tris")
FLO_UNKNOWN = 1e10                  # the .flo format's own "unknown" value: map_errors counts such a pixel as invalid


def _inv_size(h, w, name):
    if not _is_int(h) or not _is_int(w) or not 1 <= h <= INV_MAX_SIDE or not 1 <= w <= INV_MAX_SIDE:
        raise ValueError(f"{name}: h and w must be integers 1..{INV_MAX_SIDE}, got {h!r} x {w!r}")
    return int(h), int(w)


def _inv_flow(flow, name):
    """g of the coarse map [2,G,G] (or [1,2,G,G]) on the device, checked."""
    _map_device(flow, "[2,G,G]", name, "flow")
    if flow.dim() == 4 and flow.shape[0] == 1:
        flow = flow[0]
    if flow.dim() != 3 or flow.shape[0] != 2 or flow.shape[1] != flow.shape[2] or not NOISE_MIN_GRID <= flow.shape[1] <= NOISE_MAX_GRID:
        raise ValueError(f"{name}: flow must be a coarse map [2,G,G] with G {NOISE_MIN_GRID}..{NOISE_MAX_GRID}, got {tuple(flow.shape)}")
    return flow, int(flow.shape[1])


def _inv_fwd(fwd, name):
    """(h, w) of a forward map [h,w,2] f32 on the device, checked."""
    _map_device(fwd, "[h,w,2]", name, "fwd")
    if fwd.dim() != 3 or fwd.shape[2] != 2:
        raise ValueError(f"{name}: fwd must be [h,w,2], got {tuple(fwd.shape)}")
    return _inv_size(int(fwd.shape[0]), int(fwd.shape[1]), name)


def _inv_scale(scale, name):
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not np.isfinite(scale):
        raise ValueError(f"{name}: scale must be a finite number, got {scale!r}")
    return C.c_float(scale)


def _inv_out(out, shape, dtype, dev, name):
    """The caller's optional output tensor, checked, or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"{name}: out must be a contiguous {dtype} tensor {tuple(shape)} on {dev}")
    return out


def _inv_points(pts, dev, name):
    _map_device(pts, "[N,2]", name, "pts")
    if pts.dim() != 2 or pts.shape[1] != 2 or pts.shape[0] > INV_MAX_POINTS:
        raise ValueError(f"{name}: pts must be [N,2] with N at most {INV_MAX_POINTS}, got {tuple(pts.shape)}")
    if pts.device != dev:
        raise ValueError(f"{name}: pts is on {pts.device}, the map on {dev}")
    return int(pts.shape[0])


def _inv_color(color, name, what):
    if not isinstance(color, (tuple, list)) or len(color) != 3 or not all(_is_int(c) and 0 <= c <= 255 for c in color):
        raise ValueError(f"{name}: {what} must be three integers 0..255, got {color!r}")
    return int(color[0]) | int(color[1]) << 8 | int(color[2]) << 16


def _inv_workspace(h, w, step, dev):
    return torch.empty(_size_query("dvd_map_invert_workspace_bytes", h, w, step), dtype=torch.uint8, device=dev)


def map_invert(flow: torch.Tensor, h: int, w: int, step: int = 8, scale: float = 0.987, out: torch.Tensor = None, lattice: bool = False):
    """The inverse of the predicted map at the photograph's h x w.  flow [2,G,G] is a backward map (page pixel -> photograph
    position, what unwarp_u8 samples); the page's triangle mesh - lattice rows and columns 0, step, 2 step, .., the last pixel -
    is rasterised on the photograph with exact integer edge tests, the smallest triangle id winning where the map folds.
    Returns (fwd, stats): fwd [h,w,2] f32 holds the page position (u, v) of every covered photograph pixel and the bit pattern
    0xffffffff (MAP_INVALID as int32) in both components elsewhere; stats = {covered, fold_px, flipped_tris, degenerate_tris,
    skipped_tris, tris}, exact integers (fold_px: pixels covered by two or more triangles).  lattice=True: also the lattice's
    Q8 vertices [rows,cols,2] int32 and validity flags [rows,cols] uint8.  Five launches; equal calls give equal bytes."""
    flow, g = _inv_flow(flow, "map_invert")
    h, w = _inv_size(h, w, "map_invert")
    if not _is_int(step) or not 1 <= step <= INV_MAX_SIDE:
        raise ValueError(f"map_invert: step must be an integer 1..{INV_MAX_SIDE}, got {step!r}")
    cscale = _inv_scale(scale, "map_invert")
    dev = flow.device
    fwd = _inv_out(out, (h, w, 2), torch.float32, dev, "map_invert")
    ws = _inv_workspace(h, w, int(step), dev)
    words = torch.empty(len(INV_STATS), dtype=torch.int64, device=dev)
    lib.call("dvd_map_invert", ptr(flow), g, h, w, int(step), cscale, ptr(fwd), ptr(words), ptr(ws), stream_ptr())
    stats = dict(zip(INV_STATS, (int(v) for v in words.cpu().numpy())))
    if not lattice:
        return fwd, stats
    rows, cols = ((n - 1) // step + 1 + ((n - 1) % step != 0) for n in (h, w))
    up = lambda x: (x + 255) & ~255                                                      # noqa: E731
    blocks = (h * w + 1023) // 1024
    verts_at = up(up(up(up(blocks * 24) + blocks * 16) + 4 * h * w) + h * w)              # mapinv_core.h's layout
    valid_at = up(verts_at + 8 * rows * cols)
    verts = ws[verts_at:verts_at + 8 * rows * cols].view(torch.int32).view(rows, cols, 2).clone()
    return fwd, stats, verts, ws[valid_at:valid_at + rows * cols].view(rows, cols).clone()


def map_cycle_error(flow: torch.Tensor, fwd: torch.Tensor, scale: float = 0.987) -> dict:
    """How well fwd inverts the map: at every covered photograph pixel p the f32 distance |backward(fwd(p)) - p|, the backward
    map evaluated bilinearly between the page pixels.  Returns {cycle_mean, cycle_max, n}: the f64 sum, added in a fixed order,
    over the count n; NaN without a covered pixel.  Two launches."""
    flow, g = _inv_flow(flow, "map_cycle_error")
    h, w = _inv_fwd(fwd, "map_cycle_error")
    if fwd.device != flow.device:
        raise ValueError(f"map_cycle_error: flow is on {flow.device}, fwd on {fwd.device}")
    cscale = _inv_scale(scale, "map_cycle_error")
    ws = torch.empty(max((((h * w + 1023) // 1024) * 24 + 255) & ~255, 256), dtype=torch.uint8, device=flow.device)
    words = torch.empty(3, dtype=torch.int64, device=flow.device)
    lib.call("dvd_map_cycle_error", ptr(flow), g, ptr(fwd), h, w, cscale, ptr(words), ptr(ws), stream_ptr())
    host = words.cpu().numpy()
    n = int(host[0])
    if n == 0:
        return {"cycle_mean": float("nan"), "cycle_max": float("nan"), "n": 0}
    return {"cycle_mean": float(host[1:2].view(np.float64)[0]) / n, "cycle_max": float(host[2:3].view(np.uint32)[:1].view(np.float32)[0]), "n": n}


def mesh_overlay(src_u8: torch.Tensor, fwd: torch.Tensor, lines: int = 17, thickness: int = 1, color=(255, 0, 0),
                 outline_color=(0, 255, 0), dim: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """The predicted page mesh drawn on the photograph src_u8 [h,w,3] uint8: `lines` grid lines per axis of the page in `color`,
    the page's outline in `outline_color`, both widened to `thickness` 1..3; dim=True halves the pixels the page does not cover.
    Returns a new [h,w,3] uint8 tensor.  One launch."""
    h, w = _inv_fwd(fwd, "mesh_overlay")
    if _rgb8_input(src_u8, "mesh_overlay") != (h, w) or not src_u8.is_cuda or src_u8.device != fwd.device:
        raise ValueError(f"mesh_overlay: src_u8 must be [{h},{w},3] on {fwd.device} like fwd, got {tuple(src_u8.shape)} on {src_u8.device}")
    if not _is_int(lines) or not 2 <= lines <= INV_MAX_SIDE:
        raise ValueError(f"mesh_overlay: lines must be an integer 2..{INV_MAX_SIDE}, got {lines!r}")
    if not _is_int(thickness) or not 1 <= thickness <= 3:
        raise ValueError(f"mesh_overlay: thickness must be 1, 2 or 3, got {thickness!r}")
    c0, c1 = _inv_color(color, "mesh_overlay", "color"), _inv_color(outline_color, "mesh_overlay", "outline_color")
    out = _inv_out(out, (h, w, 3), torch.uint8, fwd.device, "mesh_overlay")
    if out.data_ptr() == src_u8.data_ptr():
        raise ValueError("mesh_overlay: out must be another buffer than src_u8 (a line pixel reads its neighbours' source)")
    lib.call("dvd_mesh_overlay_rgb8", ptr(src_u8), ptr(fwd), h, w, int(lines), int(thickness), c0, c1, int(bool(dim)), ptr(out),
             stream_ptr())
    return out


def mesh_overlay_to_file(src_u8: torch.Tensor, fwd: torch.Tensor, path: str, huffman: str = "fixed", **kwargs) -> int:
    """mesh_overlay as a PNG file through the device encoder: only the compressed file crosses to the host.  Returns its bytes."""
    png_huffman_flag(huffman, "mesh_overlay_to_file")
    return png_encode_to_file(mesh_overlay(src_u8, fwd, **kwargs), path, huffman)


def transfer_points(fwd: torch.Tensor, pts: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """Photograph -> page: pts [N,2] f32 (x, y) on the photograph -> [N,2] f32 (u, v) on the dewarped page, fwd sampled
    bilinearly.  A point outside the photograph, or with an uncovered pixel among its four taps, gives the bit pattern
    0xffffffff in both components."""
    h, w = _inv_fwd(fwd, "transfer_points")
    n = _inv_points(pts, fwd.device, "transfer_points")
    out = _inv_out(out, (n, 2), torch.float32, fwd.device, "transfer_points")
    lib.call("dvd_transfer_points", ptr(fwd), h, w, ptr(pts), n, ptr(out), stream_ptr())
    return out


def map_points(flow: torch.Tensor, pts: torch.Tensor, h: int, w: int, scale: float = 0.987, out: torch.Tensor = None) -> torch.Tensor:
    """Page -> photograph: pts [N,2] f32 (u, v) on the page of h x w -> [N,2] f32 (x, y) on the photograph, the backward map
    evaluated bilinearly between the page pixels (a position outside the page is clamped to it); 0xffffffff where a component
    is not finite."""
    flow, g = _inv_flow(flow, "map_points")
    h, w = _inv_size(h, w, "map_points")
    cscale = _inv_scale(scale, "map_points")
    n = _inv_points(pts, flow.device, "map_points")
    out = _inv_out(out, (n, 2), torch.float32, flow.device, "map_points")
    lib.call("dvd_map_points", ptr(flow), g, h, w, cscale, ptr(pts), n, ptr(out), stream_ptr())
    return out


def inverse_displacement(fwd) -> np.ndarray:
    """fwd [h,w,2] (a device tensor or a host array) -> the host field fwd(p) - p, [h,w,2] float32, with FLO_UNKNOWN at every
    uncovered pixel."""
    host = fwd.cpu().numpy() if torch.is_tensor(fwd) else np.asarray(fwd)
    if host.ndim != 3 or host.shape[2] != 2 or host.dtype != np.float32:
        raise ValueError(f"inverse_displacement: fwd must be [h,w,2] float32, got {host.shape} {host.dtype}")
    h, w = host.shape[:2]
    covered = np.ascontiguousarray(host).view(np.int32)[..., 0] != MAP_INVALID
    with np.errstate(invalid="ignore"):
        d = np.stack([host[..., 0] - np.arange(w, dtype=np.float32)[None, :], host[..., 1] - np.arange(h, dtype=np.float32)[:, None]],
                     axis=-1).astype(np.float32)
    d[~covered] = np.float32(FLO_UNKNOWN)
    return d


def inverse_write_flo(fwd, path: str) -> int:
    """The forward displacement fwd(p) - p as a Middlebury .flo file (flo_write); uncovered pixels hold 1e10, the format's own
    "unknown" value, which map_errors treats as invalid.  Returns the file's bytes."""
    return flo_write(inverse_displacement(fwd), path)


def coverage_mask(fwd: torch.Tensor) -> torch.Tensor:
    """[h,w,3] uint8 on the device: 255 where fwd is covered, 0 elsewhere (the input of png_encode)."""
    h, w = _inv_fwd(fwd, "coverage_mask")
    covered = fwd.view(torch.int32)[..., 0] != MAP_INVALID
    return (covered.to(torch.uint8) * 255)[..., None].expand(h, w, 3).contiguous()


# ---- synthetic documents: a flat scan drawn through a known map (dvd_amd/csrc/synth.hip; definition: DESIGN.md 4.15,
# tests/synth_model.py)
SYNTH_MAX_SIDE, SYNTH_MAX_RADIUS = 16384, 8
SYNTH_SHADING = ("l0", "lgx", "lgy", "k", "a_ref")


def _synth_device(t, dtype, shape_text, name, what):
    """A host tensor is a lib.DvdError (there is no CPU path); a wrong type or layout a ValueError."""
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: {what} must be a {shape_text} tensor, got {type(t)}")
    if not t.is_cuda:
        raise lib.DvdError(f"{name}: {what} must be on the device (the render has no CPU path), got {t.device}")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")


def _synth_sides(h, w, name, what):
    if not 1 <= h <= SYNTH_MAX_SIDE or not 1 <= w <= SYNTH_MAX_SIDE:
        raise ValueError(f"{name}: the sides of {what} must be 1..{SYNTH_MAX_SIDE}, got {h} x {w}")
    return int(h), int(w)


def _synth_fwd(fwd, name):
    _synth_device(fwd, torch.float32, "[h,w,2] float32", name, "fwd")
    if fwd.dim() != 3 or fwd.shape[2] != 2:
        raise ValueError(f"{name}: fwd must be [h,w,2], got {tuple(fwd.shape)}")
    return _synth_sides(int(fwd.shape[0]), int(fwd.shape[1]), name, "fwd")


def _synth_scan(scan_u8, name):
    _synth_device(scan_u8, torch.uint8, "[hs,ws,3] uint8", name, "scan_u8")
    if scan_u8.dim() != 3 or scan_u8.shape[2] != 3:
        raise ValueError(f"{name}: scan_u8 must be [hs,ws,3], got {tuple(scan_u8.shape)}")
    return _synth_sides(int(scan_u8.shape[0]), int(scan_u8.shape[1]), name, "scan_u8")


def synth_shading(shading, name="synth_render", need_a_ref=False) -> dict:
    """shading (None, or a dict with some of l0, lgx, lgy, k, a_ref) -> all five as floats, checked.  None, or all of l0, lgx,
    lgy and k zero, is no shading.  a_ref stays None where it is not given (synth_render then counts fwd's covered pixels)."""
    if shading is None:
        return dict(l0=0.0, lgx=0.0, lgy=0.0, k=0.0, a_ref=1.0)
    if not isinstance(shading, dict) or set(shading) - set(SYNTH_SHADING):
        raise ValueError(f"{name}: shading must be None or a dict with keys among {SYNTH_SHADING}, got {shading!r}")
    out = dict(l0=1.0, lgx=0.0, lgy=0.0, k=0.0, a_ref=None)
    out.update(shading)
    for key, v in out.items():
        if key == "a_ref" and v is None and not need_a_ref:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or abs(v) > float(np.finfo(np.float32).max):
            raise ValueError(f"{name}: shading[{key!r}] must be a finite number, got {v!r}")
        out[key] = float(v)
    if out["a_ref"] is not None and not out["a_ref"] > 0:
        raise ValueError(f"{name}: shading['a_ref'] must be positive, got {out['a_ref']!r}")
    return out


def synth_render(scan_u8: torch.Tensor, fwd: torch.Tensor, background=(255, 255, 255), shading=None, out: torch.Tensor = None) -> torch.Tensor:
    """The photograph [h,w,3] uint8 of a flat scan [hs,ws,3] uint8 seen through fwd [h,w,2] f32, the forward field map_invert
    returns (photograph pixel -> page position).  A covered pixel samples the scan with an integer tent filter whose radii 1..8
    follow fwd's first differences (radius 1: Q8 bilinear); an uncovered pixel takes the background, an RGB triple or a
    [h,w,3] uint8 tensor; the page's edge blends by the covered share of the 3 x 3 window.  shading: None or a dict with l0
    (default 1), lgx, lgy, k and a_ref (default: scan pixels per covered pixel of fwd).  One launch; equal calls, equal bytes."""
    name = "synth_render"
    hs, ws = _synth_scan(scan_u8, name)
    h, w = _synth_fwd(fwd, name)
    dev = fwd.device
    if scan_u8.device != dev:
        raise ValueError(f"{name}: scan_u8 is on {scan_u8.device}, fwd on {dev}")
    bg, color = None, 0
    if torch.is_tensor(background):
        _synth_device(background, torch.uint8, f"[{h},{w},3] uint8", name, "background")
        if tuple(background.shape) != (h, w, 3) or background.device != dev:
            raise ValueError(f"{name}: background must be [{h},{w},3] on {dev}, got {tuple(background.shape)} on {background.device}")
        bg = background
    else:
        color = _inv_color(background, name, "background")
    prm = synth_shading(shading, name)
    if prm["a_ref"] is None:
        covered = int((fwd.view(torch.int32)[..., 0] != MAP_INVALID).sum())
        prm["a_ref"] = hs * ws / covered if covered else 1.0
    out = _inv_out(out, (h, w, 3), torch.uint8, dev, name)
    if out.data_ptr() == scan_u8.data_ptr() or (bg is not None and out.data_ptr() == bg.data_ptr()):
        raise ValueError(f"{name}: out must be another buffer than scan_u8 and background")
    if w % 4 == 0 and out.data_ptr() % 4:
        raise ValueError(f"{name}: out must be 4-byte aligned where w is a multiple of 4")
    cprm = lib.SynthParams(*(prm[k] for k in SYNTH_SHADING))
    lib.call("dvd_synth_render_rgb8", ptr(scan_u8), hs, ws, ptr(fwd), h, w, ptr(bg), color, C.byref(cprm), ptr(out), stream_ptr())
    return out


def synth_footprint(scan_hw, fwd: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """[h,w,2] uint8: the radii (rx, ry) synth_render uses at every covered pixel of fwd for a scan of scan_hw = (hs, ws), 0 at
    the uncovered ones.  A radius of 8 is the cap: the scan is minified further there than the filter follows."""
    name = "synth_footprint"
    if not isinstance(scan_hw, (tuple, list)) or len(scan_hw) != 2 or not all(_is_int(v) for v in scan_hw):
        raise ValueError(f"{name}: scan_hw must be two integers (hs, ws), got {scan_hw!r}")
    hs, ws = _synth_sides(scan_hw[0], scan_hw[1], name, "the scan")
    h, w = _synth_fwd(fwd, name)
    out = _inv_out(out, (h, w, 2), torch.uint8, fwd.device, name)
    lib.call("dvd_synth_footprint", ptr(fwd), h, w, hs, ws, ptr(out), stream_ptr())
    return out


def synth_document(scan_u8: torch.Tensor, flow: torch.Tensor, h: int, w: int, step: int = 8, scale: float = 0.987,
                   background=(255, 255, 255), shading=None):
    """A photograph of h x w whose map is known: flow [2,G,G] is the backward map (what unwarp_u8 samples), map_invert turns it
    round and synth_render draws the scan through the result.  Returns (photo [h,w,3] uint8, fwd [h,w,2] f32, stats): the
    stats are map_invert's, and the shading's a_ref is hs ws / stats['covered'] unless the caller gives one."""
    name = "synth_document"
    hs, ws = _synth_scan(scan_u8, name)
    _synth_device(flow, torch.float32, "[2,G,G] float32", name, "flow")
    prm = synth_shading(shading, name)
    if not torch.is_tensor(background):
        _inv_color(background, name, "background")
    fwd, stats = map_invert(flow, h, w, step=step, scale=scale)
    if shading is not None and prm["a_ref"] is None:
        prm["a_ref"] = hs * ws / stats["covered"] if stats["covered"] else 1.0
    return synth_render(scan_u8, fwd, background=background, shading=None if shading is None else prm), fwd, stats


# ---- pages at a chosen size: the unwarp tail at any page size, filtered by its footprint (dvd_amd/csrc/sized.hip; definition:
# DESIGN.md 4.16, tests/sized_model.py)
SIZED_MAX_SIDE, SIZED_MAX_RADIUS = 16384, 16
SIZED_STATS = ("capped", "outside", "invalid")


def _size_error(spec, why):
    return ValueError(f"page_size: {spec!r}: {why} (an (hp, wp) tuple, 'HxW', 'long:N' or 'xFACTOR'; sides 1..{SIZED_MAX_SIDE})")


def parse_page_size(spec):
    """A size request, checked without a photograph: ('size', hp, wp), ('long', N) or ('scale', factor).  Anything that is no
    request is a ValueError that names the value; whether the sides it gives for a photograph are 1..16384 is page_size's to say."""
    if isinstance(spec, (tuple, list)):
        if len(spec) != 2 or not all(_is_int(v) for v in spec):
            raise _size_error(spec, "a tuple must hold two integers")
        return "size", int(spec[0]), int(spec[1])
    if isinstance(spec, str):
        import re
        text = spec.strip()
        if m := re.fullmatch(r"(\d{1,6})[xX](\d{1,6})", text):
            return "size", int(m.group(1)), int(m.group(2))
        if m := re.fullmatch(r"long:(\d{1,6})", text):
            if int(m.group(1)) < 1:
                raise _size_error(spec, "the long side must be at least 1")
            return "long", int(m.group(1))
        if m := re.fullmatch(r"[xX](\d{1,6}(?:\.\d{0,9})?|\.\d{1,9})", text):
            if not float(m.group(1)) > 0:
                raise _size_error(spec, "the factor must be positive")
            return "scale", float(m.group(1))
    raise _size_error(spec, "not a size request")


def page_size(h: int, w: int, spec):
    """The page size (hp, wp) a request asks for of a photograph of h x w.  spec: an (hp, wp) tuple of integers, or a string:
    'HxW' - that size; 'long:N' - the long side becomes N and the other side round(N short / long), at least 1; 'x0.5' - both
    sides times the factor, rounded, at least 1 (a half rounds up in both forms).  Every side must end in 1..16384; anything
    else is a ValueError that names the value.  Host only."""
    if not _is_int(h) or not _is_int(w) or h < 1 or w < 1:
        raise ValueError(f"page_size: the photograph's size must be two positive integers, got {h!r} x {w!r}")
    kind, *args = parse_page_size(spec)
    if kind == "size":
        hp, wp = args
    elif kind == "long":
        n = args[0]                # integer arithmetic: round(n short / long), a half rounding up
        hp, wp = (n, max(1, (2 * n * w + h) // (2 * h))) if h >= w else (max(1, (2 * n * h + w) // (2 * w)), n)
    else:
        hp, wp = max(1, int(np.floor(h * args[0] + 0.5))), max(1, int(np.floor(w * args[0] + 0.5)))
    if not 1 <= hp <= SIZED_MAX_SIDE or not 1 <= wp <= SIZED_MAX_SIDE:
        raise _size_error(spec, f"it asks for {hp} x {wp}")
    return hp, wp


def _sized_size(size, name):
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(v) for v in size) or \
            not all(1 <= v <= SIZED_MAX_SIDE for v in size):
        raise ValueError(f"{name}: size must be two integers (hp, wp) in 1..{SIZED_MAX_SIDE} (ops.page_size parses a request), got {size!r}")
    return int(size[0]), int(size[1])


def _sized_radius(max_radius, name):
    if not _is_int(max_radius) or not 1 <= max_radius <= SIZED_MAX_RADIUS:
        raise ValueError(f"{name}: max_radius must be an integer 1..{SIZED_MAX_RADIUS}, got {max_radius!r}")
    return int(max_radius)


def _sized_src(src_hwc, name, what="src_hwc"):
    if not torch.is_tensor(src_hwc) or not src_hwc.is_cuda:
        raise ValueError(f"{name}: {what} must be a [H,W,3] uint8 tensor on the device, got "
                         f"{src_hwc.device if torch.is_tensor(src_hwc) else type(src_hwc)}")
    if src_hwc.dtype != torch.uint8 or not src_hwc.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous uint8, got {src_hwc.dtype} contiguous={src_hwc.is_contiguous()}")
    if src_hwc.dim() != 3 or src_hwc.shape[2] != 3:
        raise ValueError(f"{name}: {what} must be [H,W,3], got {tuple(src_hwc.shape)}")
    return _synth_sides(int(src_hwc.shape[0]), int(src_hwc.shape[1]), name, what)


def _sized_counts(stats):
    """[n,3] int64 on the device -> n dicts of exact integers (one copy to the host)."""
    return [dict(zip(SIZED_STATS, (int(v) for v in row))) for row in stats.cpu().tolist()]


def unwarp_u8_sized(flow: torch.Tensor, src_hwc: torch.Tensor, size, scale: float = 0.987, max_radius: int = 16, out: torch.Tensor = None,
                    return_stats: bool = False):
    """The page [hp,wp,3] uint8 of the photograph src_hwc [H,W,3] uint8 under the coarse map flow [2,G,G] (or [1,2,G,G]) at ANY
    page size = (hp, wp), each 1..16384 (ops.page_size parses 'long:1600', 'x0.5', 'HxW').  A page pixel's position on the
    photograph is the native tail's own grid at the page's size (size = (H, W): unwarp_u8's, bit for bit) as a signed Q8
    number; the photograph is filtered there with an integer tent whose radii 1..max_radius follow the first differences of
    those positions, so a minified page does not alias; radius 1 x 1 is Q8 bilinear sampling.  A tap outside the photograph
    contributes zero (padding_mode='zeros'); a pixel whose grid value is not finite is black.  The byte is ROUNDED to nearest
    once - unwarp_u8 truncates - so at the photograph's own size the two differ by up to 2 levels.  return_stats=True: also
    {capped, outside, invalid}, the page pixels whose radius would have exceeded max_radius, whose centre lies outside the
    photograph, and whose grid value is not finite: exact integers.  One launch; equal calls give equal bytes."""
    name = "unwarp_u8_sized"
    hp, wp = _sized_size(size, name)
    max_radius = _sized_radius(max_radius, name)
    cscale = _inv_scale(scale, name)
    flow, g = _inv_flow(flow, name)
    hs, ws = _sized_src(src_hwc, name)
    dev = flow.device
    if src_hwc.device != dev:
        raise ValueError(f"{name}: src_hwc is on {src_hwc.device}, flow on {dev}")
    out = _inv_out(out, (hp, wp, 3), torch.uint8, dev, name)
    if out.data_ptr() < src_hwc.data_ptr() + src_hwc.numel() and src_hwc.data_ptr() < out.data_ptr() + out.numel():
        raise ValueError(f"{name}: out must share no byte with src_hwc")
    stats = torch.empty((1, lib.SIZED_STATS), dtype=torch.int64, device=dev) if return_stats else None
    lib.call("dvd_unwarp_u8_sized", ptr(flow), g, ptr(src_hwc), hs, ws, ptr(out), hp, wp, cscale, max_radius, ptr(stats), stream_ptr())
    return (out, _sized_counts(stats)[0]) if return_stats else out


def unwarp_u8_sized_ragged(flow: torch.Tensor, srcs, sizes, scale: float = 0.987, max_radius: int = 16, return_stats: bool = False):
    """flow [n,2,G,G]; srcs: n [H_d,W_d,3] uint8 tensors of ANY sizes; sizes: n page sizes (hp_d, wp_d) -> n uint8 pages, each the
    bytes of unwarp_u8_sized(flow[d], srcs[d], sizes[d]): the batch's documents in ONE launch (per lib.RAGGED_CAP documents).
    The pages are views of one allocation.  return_stats=True: also the list of the documents' counts."""
    name = "unwarp_u8_sized_ragged"
    max_radius = _sized_radius(max_radius, name)
    cscale = _inv_scale(scale, name)
    srcs, sizes = list(srcs), list(sizes)
    _map_device(flow, "[n,2,G,G]", name, "flow")
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[2] != flow.shape[3] or not NOISE_MIN_GRID <= flow.shape[2] <= NOISE_MAX_GRID:
        raise ValueError(f"{name}: flow must be [n,2,G,G] with G {NOISE_MIN_GRID}..{NOISE_MAX_GRID}, got {tuple(flow.shape)}")
    if flow.shape[0] != len(srcs) or len(sizes) != len(srcs):
        raise ValueError(f"{name}: {flow.shape[0]} maps, {len(srcs)} photographs and {len(sizes)} sizes: one of each per document")
    dims = []
    for d, (s, size) in enumerate(zip(srcs, sizes)):
        hs, ws = _sized_src(s, name, f"srcs[{d}]")
        if s.device != flow.device:
            raise ValueError(f"{name}: srcs[{d}] is on {s.device}, flow on {flow.device}")
        dims.append((hs, ws, *_sized_size(size, f"{name}: sizes[{d}]")))
    if not srcs:
        return ([], []) if return_stats else []
    outs = [o.view(hp, wp, 3) for o, (_, _, hp, wp) in zip(_carve([3 * hp * wp for _, _, hp, wp in dims], flow.device), dims)]
    tab = (lib.SizedImage * len(srcs))()
    for d, (s, o, (hs, ws, hp, wp)) in enumerate(zip(srcs, outs, dims)):
        tab[d].src, tab[d].out, tab[d].hs, tab[d].ws, tab[d].hp, tab[d].wp = s.data_ptr(), o.data_ptr(), hs, ws, hp, wp
    stats = torch.empty((len(srcs), lib.SIZED_STATS), dtype=torch.int64, device=flow.device) if return_stats else None
    lib.call("dvd_unwarp_u8_sized_ragged", ptr(flow), int(flow.shape[2]), tab, len(srcs), cscale, max_radius, ptr(stats), stream_ptr())
    return (outs, _sized_counts(stats)) if return_stats else outs


def sized_footprint(flow: torch.Tensor, src_hw, size, scale: float = 0.987, max_radius: int = 16, out: torch.Tensor = None) -> torch.Tensor:
    """[hp,wp] int16: rx | ry << 8, the radii unwarp_u8_sized uses at every page pixel for a photograph of src_hw = (H, W); 0
    where the grid value is not finite.  A radius equal to max_radius may be the cap (unwarp_u8_sized's `capped` counts where
    it is).  The same position and footprint code, no gather: no photograph is needed."""
    name = "sized_footprint"
    if not isinstance(src_hw, (tuple, list)) or len(src_hw) != 2 or not all(_is_int(v) for v in src_hw):
        raise ValueError(f"{name}: src_hw must be two integers (H, W), got {src_hw!r}")
    hs, ws = _synth_sides(src_hw[0], src_hw[1], name, "the photograph")
    hp, wp = _sized_size(size, name)
    max_radius = _sized_radius(max_radius, name)
    cscale = _inv_scale(scale, name)
    flow, g = _inv_flow(flow, name)
    out = _inv_out(out, (hp, wp), torch.int16, flow.device, name)
    lib.call("dvd_sized_footprint", ptr(flow), g, hs, ws, hp, wp, cscale, max_radius, ptr(out), stream_ptr())
    return out


# ---- scan-like pages: the paper estimate, the flattened page and Sauvola's plane (dvd_amd/csrc/clean.hip; definition:
# DESIGN.md 4.17, tests/clean_model.py)
CLEAN_CELLS = (4, 8, 16, 32, 64)
CLEAN_MAX_SIDE, CLEAN_MAX_CLOSE, CLEAN_MAX_SMOOTH, CLEAN_MAX_RADIUS, CLEAN_MAX_KQ = 16384, 8, 8, 63, 256
CLEAN_STATS = ("saturated", "floored", "ink")
CLEAN_STAGES = ("flatten", "binarize")


def parse_clean(spec):
    """A --clean request 'flatten', 'binarize' or 'flatten,binarize' as (flatten, binarize); anything else is a ValueError that
    names the value.  Host only."""
    parts = [p.strip() for p in spec.split(",")] if isinstance(spec, str) else None
    if not parts or any(p not in CLEAN_STAGES for p in parts) or len(set(parts)) != len(parts):
        raise ValueError(f"clean: {spec!r}: expected 'flatten', 'binarize' or 'flatten,binarize'")
    return "flatten" in parts, "binarize" in parts


def _clean_int(v, lo, hi, name, what):
    if not _is_int(v) or not lo <= v <= hi:
        raise ValueError(f"{name}: {what} must be an integer {lo}..{hi}, got {v!r}")
    return int(v)


def _clean_background_params(cell, close, smooth, name):
    if not _is_int(cell) or cell not in CLEAN_CELLS:
        raise ValueError(f"{name}: cell must be one of {CLEAN_CELLS}, got {cell!r}")
    return int(cell), _clean_int(close, 0, CLEAN_MAX_CLOSE, name, "close"), _clean_int(smooth, 0, CLEAN_MAX_SMOOTH, name, "smooth")


def clean_kq(k, name="page_binarize"):
    """Sauvola's k as kq = round(256 k), a half rounding up: 0..256.  Host only."""
    if isinstance(k, bool) or not isinstance(k, (int, float)) or not np.isfinite(k) or not 0 <= np.floor(256 * float(k) + 0.5) <= CLEAN_MAX_KQ:
        raise ValueError(f"{name}: k must be a number in 0..1, got {k!r}")
    return int(np.floor(256 * float(k) + 0.5))


def _clean_page(img, name, what="img", planes=(3,)):
    """A page [H,W,3] uint8 (planes holds 1: also a gray plane [H,W]) on the device: (h, w, channels)."""
    shapes = "[H,W,3]" + (" or [H,W]" if 1 in planes else "")
    if not torch.is_tensor(img) or not img.is_cuda:
        raise ValueError(f"{name}: {what} must be a {shapes} uint8 tensor on the device, got "
                         f"{img.device if torch.is_tensor(img) else type(img)}")
    if img.dtype != torch.uint8 or not img.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous uint8, got {img.dtype} contiguous={img.is_contiguous()}")
    if not ((img.dim() == 3 and img.shape[2] == 3) or (img.dim() == 2 and 1 in planes)):
        raise ValueError(f"{name}: {what} must be {shapes}, got {tuple(img.shape)}")
    h, w = int(img.shape[0]), int(img.shape[1])
    if not 1 <= h <= CLEAN_MAX_SIDE or not 1 <= w <= CLEAN_MAX_SIDE:
        raise ValueError(f"{name}: the sides of {what} must be 1..{CLEAN_MAX_SIDE}, got {h} x {w}")
    return h, w, 3 if img.dim() == 3 else 1


def _clean_disjoint(out, img, name, what="out"):
    if out.data_ptr() < img.data_ptr() + img.numel() and img.data_ptr() < out.data_ptr() + out.numel():
        raise ValueError(f"{name}: {what} must share no byte with the input")


def _clean_workspace(h, w, cell, dev):
    return torch.empty(_size_query("dvd_page_clean_workspace_bytes", h, w, cell), dtype=torch.uint8, device=dev)


def _clean_counts(stats, names):
    return dict(zip(names, (int(v) for v in stats.cpu().tolist())))


def page_background(img: torch.Tensor, cell: int = 16, close: int = 2, smooth: int = 2, neutral: bool = True) -> torch.Tensor:
    """The paper estimate [3,hc,wc] uint8 of the page img [H,W,3] uint8, hc = ceil(H / cell), wc = ceil(W / cell): per channel
    the maximum of every cell of cell x cell pixels (cell in 4, 8, 16, 32, 64), closed with a (2 close + 1)^2 window (ink
    narrower than that many cells is bridged; close 0..8) and smoothed with a tent of half-width `smooth` cells (0..8), every
    window clipped to the plane, rounded once.  neutral=False: one gray plane (R + 2G + B + 2) >> 2 of that estimate stands for
    all three channels, so a later flatten keeps the colour cast.  Two launches; integer arithmetic, equal calls give equal bytes."""
    name = "page_background"
    cell, close, smooth = _clean_background_params(cell, close, smooth, name)
    h, w, _ = _clean_page(img, name)
    bg = torch.empty((3, -(-h // cell), -(-w // cell)), dtype=torch.uint8, device=img.device)
    ws = _clean_workspace(h, w, cell, img.device)
    lib.call("dvd_page_background", ptr(img), h, w, cell, close, smooth, 1 if neutral else 0, ptr(bg), ptr(ws), stream_ptr())
    return bg


def page_flatten(img: torch.Tensor, cell: int = 16, close: int = 2, smooth: int = 2, neutral: bool = True, white: int = 255,
                 background: torch.Tensor = None, out: torch.Tensor = None, return_stats: bool = False):
    """The page img [H,W,3] uint8 with its illumination divided out: every sample becomes min(255, v white / bg) with bg the
    paper estimate of page_background(img, cell, close, smooth, neutral) sampled bilinearly between the cell centres and raised
    to at least one level - a constant page comes out as exactly `white` (1..255).  background: a [3,hc,wc] uint8 estimate to
    use instead (close, smooth and neutral are not read then).  return_stats=True: also {saturated, floored}, the channel
    samples whose quotient exceeded 255 and whose background was raised: exact integers.  img is not written."""
    name = "page_flatten"
    cell, close, smooth = _clean_background_params(cell, close, smooth, name)
    white = _clean_int(white, 1, 255, name, "white")
    h, w, _ = _clean_page(img, name)
    dev = img.device
    shape = (3, -(-h // cell), -(-w // cell))
    if background is None:
        background = page_background(img, cell, close, smooth, neutral)
    elif not torch.is_tensor(background) or background.device != dev or background.dtype != torch.uint8 or \
            not background.is_contiguous() or tuple(background.shape) != shape:
        raise ValueError(f"{name}: background must be a contiguous uint8 tensor {shape} on {dev} (cell = {cell})")
    out = _inv_out(out, (h, w, 3), torch.uint8, dev, name)
    _clean_disjoint(out, img, name)
    _clean_disjoint(out, background, name)
    stats = torch.empty(2, dtype=torch.int64, device=dev) if return_stats else None
    lib.call("dvd_page_flatten_rgb8", ptr(img), h, w, ptr(background), cell, white, ptr(out), None, ptr(stats), stream_ptr())
    return (out, _clean_counts(stats, CLEAN_STATS[:2])) if return_stats else out


def page_binarize(img_or_gray: torch.Tensor, radius: int = 15, k: float = 0.2, out: torch.Tensor = None, return_stats: bool = False):
    """The black-and-white plane [H,W] uint8 (0 ink, 255 paper) of a page [H,W,3] uint8 - its gray (R + 2G + B + 2) >> 2 - or of
    a gray plane [H,W] uint8, by Sauvola's rule in integers: ink where g <= m (1 + k (sd / 128 - 1)) with the mean m and the
    standard deviation sd of the (2 radius + 1)^2 window clipped to the page (radius 1..63); k is quantised to
    kq = round(256 k), 0..256, and the square root is an exact floor.  return_stats=True: also {ink}, the ink pixels."""
    name = "page_binarize"
    radius = _clean_int(radius, 1, CLEAN_MAX_RADIUS, name, "radius")
    kq = clean_kq(k, name)
    h, w, channels = _clean_page(img_or_gray, name, "img_or_gray", planes=(1, 3))
    dev = img_or_gray.device
    out = _inv_out(out, (h, w), torch.uint8, dev, name)
    _clean_disjoint(out, img_or_gray, name)
    stats = torch.empty(1, dtype=torch.int64, device=dev) if return_stats else None
    lib.call("dvd_page_binarize_u8", ptr(img_or_gray), channels, h, w, radius, kq, ptr(out), ptr(stats), stream_ptr())
    return (out, _clean_counts(stats, CLEAN_STATS[2:])) if return_stats else out


def page_clean(img: torch.Tensor, flatten: bool = True, binarize: bool = False, cell: int = 16, close: int = 2, smooth: int = 2,
               neutral: bool = True, white: int = 255, radius: int = 15, k: float = 0.2, return_stats: bool = False):
    """The chain on one page img [H,W,3] uint8 in one workspace: page_flatten (flatten=True), then page_binarize of its result
    (binarize=True) - or of img where flatten=False.  Returns the plane [H,W] uint8 with binarize, else the flattened page
    [H,W,3] uint8: the bytes of the single calls.  The flattened page's gray plane is written by the flatten kernel, so the
    binarise stage reads no RGB page again.  return_stats=True: also {saturated, floored, ink}; a stage that does not run
    counts 0."""
    name = "page_clean"
    if not flatten and not binarize:
        raise ValueError(f"{name}: flatten and binarize are both off: nothing to do")
    cell, close, smooth = _clean_background_params(cell, close, smooth, name)
    white = _clean_int(white, 1, 255, name, "white")
    radius = _clean_int(radius, 1, CLEAN_MAX_RADIUS, name, "radius")
    kq = clean_kq(k, name)
    h, w, _ = _clean_page(img, name)
    dev = img.device
    page = torch.empty((h, w, 3), dtype=torch.uint8, device=dev) if flatten else None
    plane = torch.empty((h, w), dtype=torch.uint8, device=dev) if binarize else None
    ws = _clean_workspace(h, w, cell, dev)
    stats = torch.empty(lib.CLEAN_STATS, dtype=torch.int64, device=dev) if return_stats else None
    lib.call("dvd_page_clean_rgb8", ptr(img), h, w, cell, close, smooth, 1 if neutral else 0, white, 1 if flatten else 0,
             1 if binarize else 0, radius, kq, ptr(page), ptr(plane), ptr(stats), ptr(ws), stream_ptr())
    result = plane if binarize else page
    return (result, _clean_counts(stats, CLEAN_STATS)) if return_stats else result
