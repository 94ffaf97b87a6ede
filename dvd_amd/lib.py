"""ctypes binding of libdvd_hip.so (include/dvd_hip.h).

The HIP library IS the product: there is no CPU or eager-PyTorch fallback.  Importing this
module loads `dvd_amd/libdvd_hip.so` (built in-tree by `__graft_entry__.build()` /
`make -C dvd_amd/csrc`) and raises if it is missing; every wrapper raises `DvdError` with
the library's message on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os

# torch must be imported BEFORE the library is loaded: the PyTorch-ROCm wheel bundles its own
# libamdhip64.so.7 and libdvd_hip.so must bind to that same HIP runtime (same SONAME => the loader
# reuses it); loading ours first would create a second runtime that sees no device.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree build and nothing else: no environment variable can put another library under it.
# benchmarks/ and the `lab` pytest fixture swap in the lab build explicitly, in their own process (use_library below).
LIB_PATH = os.path.join(_HERE, "libdvd_hip.so")


class DvdError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise DvdError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C dvd_amd/csrc`.  The DvD engine has no non-HIP fallback.")
    return C.CDLL(LIB_PATH)


_lib = _load()

c_f32p = C.POINTER(C.c_float)
c_void = C.c_void_p


class SchedCoef(C.Structure):
    _fields_ = [("kind", C.c_int), ("c_recip", C.c_float), ("c_recipm1", C.c_float),
                ("sqrt_abar_prev", C.c_float), ("dir_coef", C.c_float), ("coef1", C.c_float),
                ("coef2", C.c_float), ("sigma", C.c_float)]


class GemmDesc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("batch", C.c_int),
                ("A", C.c_void_p), ("lda", C.c_int), ("strideA", C.c_long),
                ("B", C.c_void_p), ("ldb", C.c_int), ("strideB", C.c_long),
                ("B_lo", C.c_void_p), ("A_lo", C.c_void_p), ("lo_scale", C.c_float),
                ("C32", C.c_void_p), ("ldc", C.c_int), ("strideC32", C.c_long),
                ("C16", C.c_void_p), ("ldc16", C.c_int), ("strideC16", C.c_long),
                ("bias", C.c_void_p), ("bias_row", C.c_int), ("strideBias", C.c_long),
                ("act", C.c_int),
                ("pos", C.c_void_p), ("ldpos", C.c_int), ("pos_rows", C.c_int),
                ("gate", C.c_void_p), ("ldgate", C.c_int), ("gate_rows", C.c_int), ("strideGate", C.c_long),
                ("res", C.c_void_p), ("ldres", C.c_int), ("strideRes", C.c_long), ("small_tiles", C.c_int)]


class AttnDesc(C.Structure):
    _fields_ = [("head_dim", C.c_int), ("heads", C.c_int), ("batch", C.c_int), ("tq", C.c_int), ("tk", C.c_int),
                ("kv_batch_div", C.c_int),
                ("Q", C.c_void_p), ("ldq", C.c_int), ("strideQ", C.c_long),
                ("K", C.c_void_p), ("ldk", C.c_int), ("strideK", C.c_long),
                ("Vt", C.c_void_p), ("ldvt", C.c_int), ("strideVt", C.c_long),
                ("O", C.c_void_p), ("ldo", C.c_int), ("strideO", C.c_long),
                ("scale", C.c_float)]


class CnOp(C.Structure):
    _fields_ = [("op", C.c_int), ("a", C.c_int), ("b", C.c_int), ("dst", C.c_int), ("ks", C.c_int), ("dil", C.c_int),
                ("cout", C.c_int), ("act", C.c_int), ("w_off", C.c_long), ("h", C.c_int), ("w", C.c_int),
                ("flag", C.c_int)]


class RaggedImage(C.Structure):
    """dvd_ragged_image: one document of a ragged batch (device pointers, its own size)."""
    _fields_ = [("src", C.c_void_p), ("out", C.c_void_p), ("h", C.c_int), ("w", C.c_int)]


SSIM_REPLICATE, SSIM_VALID = 0, 1          # DVD_SSIM_*: border of the 11x11 window
MSSSIM_DOCUNET, MSSSIM_WANG = 0, 1         # DVD_MSSSIM_*: presets of dvd_msssim_scales

PNG_SEGMENT = 32768   # DVD_PNG_SEGMENT: filtered-stream bytes per IDAT chunk of the PNG encoder
PNG_HUFFMAN_FIXED, PNG_HUFFMAN_DYNAMIC = 0, 1   # DVD_PNG_HUFFMAN_*: the block type of a segment

JPEG_420, JPEG_444 = 0, 1                  # DVD_JPEG_*: chroma subsampling of the JPEG encoder


class JpegDecInfo(C.Structure):
    """dvd_jpegdec_info: what dvd_jpegdec_probe reads from a JPEG file's header."""
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int), ("components", C.c_int),
                ("hs", C.c_int), ("vs", C.c_int), ("orientation", C.c_int), ("restart_interval", C.c_int),
                ("scan_offset", C.c_long), ("scan_bytes", C.c_long), ("blocks", C.c_long), ("scratch_bytes", C.c_long)]


# DVD_E_JPEG_*: why the JPEG decoder hands a file back (a refusal on the host, or NOSYNC / DATA after the entropy decoder ran)
JPEG_DECODE_CODES = {-20: "HEADER", -21: "PROGRESSIVE", -22: "EXTENDED", -23: "LOSSLESS", -24: "ARITHMETIC", -25: "PRECISION",
                     -26: "COMPONENTS", -27: "ADOBE", -28: "SAMPLING", -29: "SCANS", -30: "QUANT16", -31: "TABLE", -32: "SIZE",
                     -33: "ORIENTATION", -34: "NOSYNC", -35: "DATA"}
JPEGDEC_SUBSEQ = 128   # DVD_JPEGDEC_SUBSEQ: bytes of the scan per lane of the entropy decoder


class PngDecInfo(C.Structure):
    """dvd_pngdec_info: what dvd_pngdec_probe reads from a PNG file's chunks."""
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("colour_type", C.c_int), ("bpp", C.c_int), ("idat_chunks", C.c_long),
                ("payload_bytes", C.c_long), ("scratch_bytes", C.c_long)]


class PngDecStats(C.Structure):
    """dvd_pngdec_stats: what a decode ran."""
    _fields_ = [("candidates", C.c_int), ("segments", C.c_int), ("rounds", C.c_int), ("bands", C.c_int)]


# DVD_E_PNG_*: why the PNG decoder hands a file back (a refusal on the host, or DATA / NOSPLIT after the inflate ran)
PNG_DECODE_CODES = {-36: "HEADER", -37: "INTERLACE", -38: "DEPTH", -39: "COLOUR", -40: "TRNS", -41: "APNG", -42: "METADATA",
                    -43: "ZLIB", -44: "SIZE", -45: "DATA", -46: "NOSPLIT"}
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"

class SflowParams(C.Structure):
    """dvd_sflow_params: the parameters of the SIFT-flow chain, ten ints in this order."""
    _fields_ = [(name, C.c_int) for name in ("levels", "w_top", "w", "iters_top", "iters", "alpha", "d", "gamma", "T", "eps")]


SFLOW_DEFAULTS = dict(levels=4, w_top=10, w=2, iters_top=60, iters=30, alpha=510, d=10200, gamma=1, T=8160, eps=1 << 17)
SFLOW_MIN_TOP = 12    # DVD_SFLOW_MIN_TOP: least side of the top pyramid level

FLOW_NORM_DIAG, FLOW_NORM_MAX = 0, 1   # DVD_FLOW_NORM_*: rad_max of a flow picture
E_FLOW_SHAPE = -50                     # DVD_E_FLOW_SHAPE
E_MAP_SHAPE, E_MAP_RANKS = -51, -52    # DVD_E_MAP_*: what the map score refuses
E_INV_SHAPE, E_INV_STEP, E_INV_LINES, E_INV_POINTS = -53, -54, -55, -56    # DVD_E_INV_*: what the map inverse refuses

E_SYNTH_SHAPE, E_SYNTH_PARAM = -57, -58    # DVD_E_SYNTH_*: what the synthetic-document render refuses


class SynthParams(C.Structure):
    """dvd_synth_params: the render's shading (all of l0, lgx, lgy, k zero: none) and the mean scan area per covered pixel."""
    _fields_ = [(name, C.c_float) for name in ("l0", "lgx", "lgy", "k", "a_ref")]


E_SIZED_SHAPE, E_SIZED_PARAM = -59, -60    # DVD_E_SIZED_*: what the page at a chosen size refuses
SIZED_STATS = 3                            # DVD_SIZED_STATS: the counts of a sized unwarp (capped, outside, invalid)


class SizedImage(C.Structure):
    """dvd_sized_image: one document of a sized ragged batch (device pointers; the photograph's and the page's size)."""
    _fields_ = [("src", C.c_void_p), ("out", C.c_void_p), ("hs", C.c_int), ("ws", C.c_int), ("hp", C.c_int), ("wp", C.c_int)]


E_CLEAN_SHAPE, E_CLEAN_PARAM = -61, -62    # DVD_E_CLEAN_*: what the scan-like page refuses
CLEAN_STATS = 3                            # DVD_CLEAN_STATS: the counts of a cleaned page (saturated, floored, ink)

RAGGED_CAP = 64  # DVD_RAGGED_CAP: documents per launch of the ragged entry points (larger batches are cut by the library)

NON_STATUS = {"dvd_last_error", "dvd_version", "dvd_engine_workspace_bytes", "dvd_engine_tensor_count",
              "dvd_flash_attn_kernel_name", "dvd_gemm_kernel_name", "dvd_convnet_workspace_bytes", "dvd_convnet_weight_floats",
              "dvd_ingest_scratch_bytes", "dvd_ingest_ragged_scratch_bytes", "dvd_resize_gray_scratch_bytes",
              "dvd_msssim_workspace_bytes", "dvd_png_bound", "dvd_png_scratch_bytes", "dvd_png_scratch_bytes_huff", "dvd_jpeg_bound",
              "dvd_jpeg_scratch_bytes", "dvd_sflow_level_workspace_bytes", "dvd_sflow_workspace_bytes",
              "dvd_adist_workspace_bytes", "dvd_corrupt_supported", "dvd_corrupt_table", "dvd_map_deviation_workspace_bytes",
              "dvd_flow_workspace_bytes", "dvd_mapscore_workspace_bytes", "dvd_map_invert_workspace_bytes",
              "dvd_page_clean_workspace_bytes"}

# name -> argtypes; kept in one table so tests can check every symbol of include/dvd_hip.h
SIGNATURES = {
    "dvd_grid_sample_bilinear_zeros_ac": [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, c_void],
    "dvd_unwarp_f32": [c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, C.c_float, c_void],
    "dvd_unwarp_u8": [c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, C.c_float, c_void],
    "dvd_unwarp_f32_batch": [c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_void],
    "dvd_unwarp_u8_batch": [c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_void],
    "dvd_unwarp_grid": [c_void, C.c_int, c_void, C.c_int, C.c_int, C.c_float, c_void],
    "dvd_unwarp_u8_ragged": [c_void, C.c_int, C.POINTER(RaggedImage), C.c_int, C.c_float, c_void],
    "dvd_grid_sample_bicubic_zeros_ac": [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, c_void],
    "dvd_unwarp_u8_bicubic_batch": [c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_void],
    "dvd_unwarp_u8_bicubic_ragged": [c_void, C.c_int, C.POINTER(RaggedImage), C.c_int, C.c_float, c_void],
    "dvd_sched_step": [C.POINTER(SchedCoef), c_void, c_void, c_void, c_void, c_void, C.c_int, C.c_int, c_void],
    "dvd_sched_step_clip": [C.POINTER(SchedCoef), c_void, c_void, c_void, c_void, c_void, C.c_int, C.c_int, c_void],
    "dvd_hyp_mean_clamp": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_selftest_mfma": [c_void, c_void, c_void, c_void, c_void],
    "dvd_gemm_nt": [C.POINTER(GemmDesc), c_void],
    "dvd_gemm_kernel_name": [C.POINTER(GemmDesc)],
    "dvd_flash_attn": [C.POINTER(AttnDesc), c_void],
    "dvd_embed_obs_ln": [c_void, c_void, c_void, c_void, c_void, c_void, C.c_int, C.c_int, c_void],
    "dvd_layernorm_rows": [c_void, C.c_int, C.c_long, c_void, C.c_int, C.c_long, C.c_int, C.c_long, C.c_int, c_void,
                           c_void, c_void, c_void, C.c_int, C.c_int, C.c_float, c_void],
    "dvd_build_r_rows": [c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_patch_rows": [c_void, C.c_long, C.c_long, C.c_long, C.c_long, c_void, C.c_int, C.c_int, C.c_int, C.c_int,
                       c_void],
    "dvd_dwconv3x3": [c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_colmean": [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_posenc_add": [c_void, c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_small_linear": [c_void, C.c_int, c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                         C.c_int, c_void],
    "dvd_final_tokens": [c_void, c_void, c_void, c_void, c_void, C.c_int, C.c_int, c_void, c_void, c_void, c_void,
                         c_void, C.c_int, C.c_int, c_void],
    "dvd_im2col3x3": [c_void, C.c_long, C.c_long, C.c_long, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_conv3x3_nhwc": [c_void, C.c_int, c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_maxpool2_nhwc": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_resize_bilinear_nhwc": [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_nhwc_to_nchw": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_convnet_create": [C.POINTER(CnOp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(c_void)],
    "dvd_convnet_create_batched": [C.POINTER(CnOp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(c_void)],
    "dvd_convnet_destroy": [c_void],
    "dvd_convnet_slot_shape": [c_void, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "dvd_convnet_op_info": [c_void, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "dvd_convnet_run": [c_void, c_void, c_void, c_void, C.c_long, C.c_int, C.POINTER(C.c_int), C.POINTER(c_void), c_void],
    "dvd_resize_bilinear_nchw": [c_void, c_void, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_threshold_mask_mul": [c_void, c_void, c_void, c_void, C.c_int, C.c_long, C.c_float, c_void],
    "dvd_threshold_mask_mul_batch": [c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_long, C.c_float, c_void],
    "dvd_flash_attn_f32": [C.POINTER(AttnDesc), c_void],
    "dvd_layernorm256_f32": [c_void, c_void, C.c_long, c_void, c_void, C.c_float, c_void],
    "dvd_add_rows_f32": [c_void, c_void, c_void, C.c_long, C.c_int, C.c_int, c_void],
    "dvd_transpose_f32": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_soft_mask_mul_batch": [c_void, c_void, c_void, C.c_int, C.c_int, C.c_long, c_void],
    "dvd_convex_upsample": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, C.c_int, C.c_float, c_void],
    "dvd_ingest_u8": [c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, c_void, c_void, c_void],
    "dvd_ingest_ragged_scratch_bytes": [C.c_int, C.c_int],
    "dvd_ingest_u8_ragged": [C.POINTER(RaggedImage), C.c_int, C.c_int, c_void, C.c_int, c_void, c_void],
    "dvd_resize_gray_scratch_bytes": [C.c_int, C.c_int, C.c_int, C.c_int],
    "dvd_resize_gray_u8": [c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, c_void, c_void],
    "dvd_ssim_scale": [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void],
    "dvd_ssim_finalize": [c_void, C.c_int, C.c_int, C.c_long, c_void, C.c_int, c_void],
    "dvd_reduce2_pair": [c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_msssim_workspace_bytes": [C.c_int, C.c_int, C.c_int],
    "dvd_msssim_scales": [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void],
    "dvd_dsift_u8": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void],
    "dvd_sflow_cost": [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.POINTER(SflowParams), c_void, c_void],
    "dvd_sflow_level_workspace_bytes": [C.c_int, C.c_int, C.c_int],
    "dvd_sflow_level": [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SflowParams), c_void, c_void, c_void,
                        c_void],
    "dvd_sflow_workspace_bytes": [C.c_int, C.c_int, C.POINTER(SflowParams)],
    "dvd_sflow": [c_void, c_void, C.c_int, C.c_int, C.c_int, C.POINTER(SflowParams), c_void, c_void, c_void, c_void],
    "dvd_ad_fit": [c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void, c_void],
    "dvd_ad_align": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void],
    "dvd_ad_weighted": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void],
    "dvd_adist_workspace_bytes": [C.c_int, C.c_int, C.POINTER(SflowParams)],
    "dvd_adist": [c_void, c_void, C.c_int, C.c_int, C.c_int, C.POINTER(SflowParams), c_void, c_void, c_void, c_void, c_void, c_void,
                  c_void, c_void, c_void],
    "dvd_corrupt_supported": [C.c_int],
    "dvd_corrupt_table": [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int],
    "dvd_corrupt_rgb8": [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void],
    "dvd_unit_to_rgb8": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_rgb8_to_unit": [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void],
    "dvd_randn_keyed": [c_void, C.c_int, C.c_int, C.c_int, C.c_uint32, c_void, c_void],
    "dvd_map_deviation_workspace_bytes": [C.c_int, C.c_int],
    "dvd_map_deviation": [c_void, c_void, C.c_int, C.c_int, c_void, c_void, c_void],
    "dvd_flow_workspace_bytes": [C.c_int, C.c_int, C.c_int],
    "dvd_flow_radius_max": [c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void],
    "dvd_flow_to_image_rgb8": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, c_void, c_void, c_void, c_void],
    "dvd_flow_full_uv": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void],
    "dvd_flow_picture_rgb8": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void, c_void],
    "dvd_mapscore_workspace_bytes": [C.c_int, C.c_int],
    "dvd_map_errors": [c_void, C.c_int, c_void, C.c_int, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void, c_void],
    "dvd_map_metrics": [c_void, C.c_int, C.c_int, c_void, c_void],
    "dvd_select_u32": [c_void, C.c_long, C.POINTER(C.c_uint32), C.c_int, c_void, c_void, c_void],
    "dvd_sparsify_bins": [c_void, c_void, C.c_long, c_void, C.c_int, c_void, c_void, c_void],
    "dvd_map_invert_workspace_bytes": [C.c_int, C.c_int, C.c_int],
    "dvd_map_invert": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void, c_void],
    "dvd_map_cycle_error": [c_void, C.c_int, c_void, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void],
    "dvd_mesh_overlay_rgb8": [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, c_void, c_void],
    "dvd_transfer_points": [c_void, C.c_int, C.c_int, c_void, C.c_long, c_void, c_void],
    "dvd_map_points": [c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_void, C.c_long, c_void, c_void],
    "dvd_synth_render_rgb8": [c_void, C.c_int, C.c_int, c_void, C.c_int, C.c_int, c_void, C.c_uint32, C.POINTER(SynthParams), c_void, c_void],
    "dvd_synth_footprint": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void],
    "dvd_unwarp_u8_sized": [c_void, C.c_int, c_void, C.c_int, C.c_int, c_void, C.c_int, C.c_int, C.c_float, C.c_int, c_void, c_void],
    "dvd_unwarp_u8_sized_ragged": [c_void, C.c_int, C.POINTER(SizedImage), C.c_int, C.c_float, C.c_int, c_void, c_void],
    "dvd_sized_footprint": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, c_void, c_void],
    "dvd_page_clean_workspace_bytes": [C.c_int, C.c_int, C.c_int],
    "dvd_page_background": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void],
    "dvd_page_flatten_rgb8": [c_void, C.c_int, C.c_int, c_void, C.c_int, C.c_int, c_void, c_void, c_void, c_void],
    "dvd_page_binarize_u8": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void],
    "dvd_page_clean_rgb8": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                            c_void, c_void, c_void, c_void, c_void],
    "dvd_png_bound": [C.c_int, C.c_int],
    "dvd_png_scratch_bytes": [C.c_int, C.c_int],
    "dvd_png_encode_rgb8": [c_void, C.c_int, C.c_int, c_void, C.c_long, c_void, c_void, c_void],
    "dvd_png_scratch_bytes_huff": [C.c_int, C.c_int, C.c_int],
    "dvd_png_encode_rgb8_huff": [c_void, C.c_int, C.c_int, c_void, C.c_long, c_void, c_void, C.c_int, c_void],
    "dvd_jpeg_bound": [C.c_int, C.c_int, C.c_int],
    "dvd_jpeg_scratch_bytes": [C.c_int, C.c_int, C.c_int],
    "dvd_jpeg_encode_rgb8": [c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, C.c_long, c_void, c_void, c_void],
    "dvd_jpegdec_probe": [c_void, C.c_long, C.POINTER(JpegDecInfo)],
    "dvd_jpeg_decode_rgb8": [c_void, c_void, C.c_long, c_void, C.c_long, C.c_int, C.POINTER(C.c_int), c_void, c_void],
    "dvd_pngdec_probe": [c_void, C.c_long, C.POINTER(PngDecInfo)],
    "dvd_png_decode_rgb8": [c_void, c_void, C.c_long, c_void, C.c_long, C.c_long, C.POINTER(PngDecStats), c_void, c_void],
    "dvd_dither_f16": [c_void, c_void, c_void, C.c_long, C.c_uint, C.c_uint, c_void],
    "dvd_engine_create": [C.c_int, C.c_int, C.c_int, C.POINTER(c_void)],
    "dvd_engine_destroy": [c_void],
    "dvd_engine_bind_workspace": [c_void, c_void, C.c_long],
    "dvd_engine_tensor_count": [c_void],
    "dvd_engine_tensor_info": [c_void, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_long)],
    "dvd_engine_set_tensor": [c_void, C.c_char_p, c_void, C.c_long],
    "dvd_engine_prepare_docs": [c_void, c_void, c_void, c_void, c_void, c_void],
    "dvd_engine_feat_nchw": [c_void, c_void, c_void],
    "dvd_engine_denoise_step": [c_void, c_void, C.c_float, C.c_int, c_void, c_void, c_void, c_void],
    "dvd_engine_debug_buffer": [c_void, C.c_char_p, C.POINTER(c_void), C.POINTER(C.c_long)],
    "dvd_engine_debug_stop": [c_void, C.c_int],
    "dvd_engine_set_option": [c_void, C.c_char_p, C.c_int],
    "dvd_engine_profile": [c_void, C.c_int],
    "dvd_engine_profile_read": [c_void, C.POINTER(C.c_int), C.POINTER(C.c_double)],
}


# entries of SIGNATURES that return something other than a status
RESTYPES = {"dvd_gemm_kernel_name": C.c_char_p, "dvd_ingest_ragged_scratch_bytes": C.c_long,
            "dvd_resize_gray_scratch_bytes": C.c_long, "dvd_msssim_workspace_bytes": C.c_long,
            "dvd_sflow_level_workspace_bytes": C.c_long, "dvd_sflow_workspace_bytes": C.c_long,
            "dvd_adist_workspace_bytes": C.c_long, "dvd_map_deviation_workspace_bytes": C.c_long,
            "dvd_flow_workspace_bytes": C.c_long, "dvd_mapscore_workspace_bytes": C.c_long,
            "dvd_map_invert_workspace_bytes": C.c_long, "dvd_page_clean_workspace_bytes": C.c_long, "dvd_png_bound": C.c_long, "dvd_png_scratch_bytes": C.c_long, "dvd_png_scratch_bytes_huff": C.c_long,
            "dvd_jpeg_bound": C.c_long, "dvd_jpeg_scratch_bytes": C.c_long}

# entry points that exist only in the lab build (benchmarks/lab/dvd_hip_lab.h; loaded through use_library)
LAB_SIGNATURES = {"dvd_gemm_debug_stamps": [c_void], "dvd_attn_debug_stamps": [c_void]}


def bind(cdll):
    """Attach argtypes / restypes to a loaded libdvd_hip.so (the product library, or the lab build in tests/benchmarks)."""
    cdll.dvd_last_error.restype = C.c_char_p
    cdll.dvd_version.restype = C.c_int
    cdll.dvd_engine_workspace_bytes.restype = C.c_long
    cdll.dvd_engine_workspace_bytes.argtypes = [C.c_void_p]
    for fn in (cdll.dvd_convnet_workspace_bytes, cdll.dvd_convnet_weight_floats):
        fn.restype, fn.argtypes = C.c_long, [C.c_void_p]
    cdll.dvd_ingest_scratch_bytes.restype, cdll.dvd_ingest_scratch_bytes.argtypes = C.c_long, [C.c_int]
    cdll.dvd_flash_attn_kernel_name.restype = C.c_char_p
    cdll.dvd_flash_attn_kernel_name.argtypes = [C.c_int, C.c_int, C.c_int]
    for name, args in SIGNATURES.items():
        fn = getattr(cdll, name)
        fn.argtypes, fn.restype = args, RESTYPES.get(name, C.c_int)
    for name, args in LAB_SIGNATURES.items():
        if hasattr(cdll, name):
            fn = getattr(cdll, name)
            fn.argtypes, fn.restype = args, C.c_int
    return cdll


bind(_lib)


def use_library(path: str):
    """Route this process through another build of the SAME library (benchmarks/_lab.py and the `lab` pytest fixture
    load benchmarks/lab/libdvd_hip_lab.so this way).  An explicit call in the caller's code - never the environment."""
    global _lib
    _lib = bind(C.CDLL(os.path.abspath(path)))
    return _lib


def call(name: str, *args):
    """Invoke a status-returning entry point; raise DvdError on failure."""
    rc = getattr(_lib, name)(*args)
    if rc != 0:
        raise DvdError(f"{name} failed ({rc}): {_lib.dvd_last_error().decode()}")


def flash_attn_kernel_name(head_dim: int, tq: int, tk: int) -> str:
    return _lib.dvd_flash_attn_kernel_name(head_dim, tq, tk).decode()


def gemm_kernel_name(desc: GemmDesc) -> str:
    """The kernel instance dvd_gemm_nt launches for `desc` ("" if it refuses it); host-only."""
    return _lib.dvd_gemm_kernel_name(C.byref(desc)).decode()


def version() -> int:
    return int(_lib.dvd_version())


def raw():
    return _lib


def ptr(t):
    """Device (or host) address of a torch tensor / None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
