"""`visualize_dewarping` - the egress of the sampling path (utils_flow/visualization_utils.py:64-78): warp the
full-resolution source by the full-resolution sampling grid, truncate to uint8, write
`vis_hp/<eval_dataset_name>/<settings.name>/dewarped_pred/warped_<file stem>.png`.

Called as the reference calls it (evaluation.py:311-312)

    visualize_dewarping(settings, sample, data, i, source_vis, data_path, ref_flow)

`sample` is the grid `((interp(flow) + base)*2 - 1)*0.987` [1,2,H,W] and the warp is `reg_model_bilin([source_vis, sample])`
on the drop-in HIP kernel (32 B/px).  `dvd_amd.evaluation.run_evaluation_docunet` instead passes `warped_u8=`: the bytes its
fused tail kernel (`dvd_unwarp_u8[_batch]`, 6 B/px: up-sampling, base grid, affine, gather and truncation in one launch) already
produced from the COARSE flow - bit-identical to the long way (tests/test_gpu_ops.py::test_unwarp_golden, golden G5).

`settings.env.png_encoder` chooses who writes the PNG: 'pil' (default, the reference's Image.save on a host copy of the page) or
'hip' (`dvd_amd.ops.png_encode_to_file`: filtered and compressed where the page lies, only the file crosses to the host - the
same pixels in a file of other bytes).  With 'hip', `settings.env.png_huffman` = 'fixed' (default) | 'dynamic' chooses
the encoder's deflate blocks: 'dynamic' writes per segment the smaller of a dynamic-Huffman and the fixed block.

`settings.env.page_format = 'jpeg'` (default 'png': all of the above, unchanged) writes `warped_<stem>.jpg` instead: baseline
JFIF at `env.jpeg_quality` (1..100, default 90) and `env.jpeg_subsampling` ('420' default | '444'), encoded on the device by
`dvd_amd.ops.jpeg_encode_to_file`; `png_encoder` is not consulted."""
from __future__ import annotations

import os

import numpy as np
from PIL import Image

from datasets.utils.warping import register_model2

reg_model_bilin = register_model2((512, 512), "bilinear")
PNG_ENCODERS = ("pil", "hip")
PNG_HUFFMAN = ("fixed", "dynamic")
PAGE_FORMATS = ("png", "jpeg")
JPEG_SUBSAMPLINGS = ("420", "444")


def page_settings(env):
    """(page_format, jpeg_quality, jpeg_subsampling) of `env`, each checked: ValueError names the setting."""
    fmt = getattr(env, "page_format", "png")
    quality = getattr(env, "jpeg_quality", 90)
    subsampling = getattr(env, "jpeg_subsampling", "420")
    if fmt not in PAGE_FORMATS:
        raise ValueError(f"env.page_format must be 'png' or 'jpeg', got {fmt!r}")
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"env.jpeg_quality must be an integer 1..100, got {quality!r}")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"env.jpeg_subsampling must be '420' or '444', got {subsampling!r}")
    return fmt, int(quality), subsampling


def png_huffman_setting(env):
    """env.png_huffman, checked: ValueError names the setting."""
    huffman = getattr(env, "png_huffman", "fixed")
    if not isinstance(huffman, str) or huffman not in PNG_HUFFMAN:
        raise ValueError(f"env.png_huffman must be 'fixed' or 'dynamic', got {huffman!r}")
    return huffman


def _stem(data_path):
    name = data_path[0] if isinstance(data_path, (list, tuple)) else data_path
    return name.split("/")[-1][:-4]              # the reference's rule (:78): basename minus a 4-character extension


def visualize_dewarping(settings, sample, data, i, source_vis, data_path, ref_flow=None, *, warped_u8=None):
    """Returns the uint8 [H,W,3] image it wrote (the reference returns None): a NumPy array with png_encoder 'pil', the
    DEVICE tensor with 'hip' and with page_format 'jpeg' (the page is never copied to the host there)."""
    encoder = getattr(settings.env, "png_encoder", "pil")
    if encoder not in PNG_ENCODERS:
        raise ValueError(f"env.png_encoder must be 'pil' or 'hip', got {encoder!r}")
    huffman = png_huffman_setting(settings.env)
    page_format, quality, subsampling = page_settings(settings.env)
    if page_format == "jpeg":
        encoder = "jpeg"                             # the device route below; png_encoder is not consulted
    out_dir = f"vis_hp/{settings.env.eval_dataset_name}/{settings.name}"
    os.makedirs(f"{out_dir}/pred_flow", exist_ok=True)
    os.makedirs(f"{out_dir}/dewarped_pred", exist_ok=True)
    if encoder in ("hip", "jpeg"):
        import torch
        from dvd_amd import ops
        if warped_u8 is None:                        # the reference's call form: truncated to uint8 on the device
            warped = reg_model_bilin([source_vis.to(sample.device).float(), sample])
            warped_u8 = warped[0].permute(1, 2, 0).detach().to(torch.uint8)
        elif not torch.is_tensor(warped_u8):
            warped_u8 = torch.from_numpy(np.asarray(warped_u8))
        if not warped_u8.is_cuda:
            warped_u8 = warped_u8.to(sample.device if sample is not None else "cuda")
        warped_u8 = warped_u8.detach().contiguous()
        if encoder == "jpeg":
            ops.jpeg_encode_to_file(warped_u8, f"{out_dir}/dewarped_pred/warped_{_stem(data_path)}.jpg", quality, subsampling)
        else:
            ops.png_encode_to_file(warped_u8, f"{out_dir}/dewarped_pred/warped_{_stem(data_path)}.png", huffman)
    elif warped_u8 is None:
        warped = reg_model_bilin([source_vis.to(sample.device).float(), sample])
        warped_u8 = warped[0].permute(1, 2, 0).detach().cpu().numpy().astype(np.uint8)
    else:
        warped_u8 = warped_u8.detach().cpu().numpy() if hasattr(warped_u8, "detach") else np.asarray(warped_u8)
    if encoder == "pil":
        Image.fromarray(warped_u8).save(f"{out_dir}/dewarped_pred/warped_{_stem(data_path)}.png")
    if ref_flow is not None:
        os.makedirs(f"{out_dir}/pred_flow_ref", exist_ok=True)
        os.makedirs(f"{out_dir}/dewarped_pred_ref", exist_ok=True)
        ref = reg_model_bilin([source_vis.to(ref_flow.device).float(), ref_flow])
        ref = ref[0].permute(1, 2, 0).detach().cpu().numpy().astype(np.uint8)
        name = data_path[0] if isinstance(data_path, (list, tuple)) else data_path
        Image.fromarray(ref).save(f"{out_dir}/dewarped_pred_ref/warped_{name.split('/')[-1]}")   # with its extension (:92)
    return warped_u8
