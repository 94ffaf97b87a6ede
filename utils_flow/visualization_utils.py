"""`visualize_dewarping` - the egress of the sampling path (utils_flow/visualization_utils.py:64-78): warp the
full-resolution source by the full-resolution sampling grid, truncate to uint8, write
`vis_hp/<eval_dataset_name>/<settings.name>/dewarped_pred/warped_<file stem>.png`.

Called as the reference calls it (evaluation.py:311-312)

    visualize_dewarping(settings, sample, data, i, source_vis, data_path, ref_flow)

`sample` is the grid `((interp(flow) + base)*2 - 1)*0.987` [1,2,H,W] and the warp is `reg_model_bilin([source_vis, sample])`
on the drop-in HIP kernel (32 B/px).  `dvd_amd.evaluation.run_evaluation_docunet` instead passes `warped_u8=`: the bytes its
fused tail kernel (`dvd_unwarp_u8[_batch]`, 6 B/px: up-sampling, base grid, affine, gather and truncation in one launch) already
produced from the COARSE flow - bit-identical to the long way (tests/test_gpu_ops.py::test_unwarp_golden, golden G5).

Who writes the page - PIL on a host copy (the default, the reference's Image.save), `dvd_amd.ops.png_encode_to_file` or, as
`warped_<stem>.jpg`, `dvd_amd.ops.jpeg_encode_to_file` - is `PageOptions.page_writer`: the switches `png_encoder`, `png_huffman`,
`page_format`, `jpeg_quality` and `jpeg_subsampling` of dvd_amd/run_options.py, checked here on every call."""
from __future__ import annotations

import os

import numpy as np
from PIL import Image

from datasets.utils.warping import register_model2
from dvd_amd import run_options
from dvd_amd.run_options import PageOptions

reg_model_bilin = register_model2((512, 512), "bilinear")


def page_settings(env):
    """(page_format, jpeg_quality, jpeg_subsampling) of `env`, each checked: ValueError names the setting."""
    return tuple(run_options.check(env, name) for name in ("page_format", "jpeg_quality", "jpeg_subsampling"))


def png_huffman_setting(env):
    """env.png_huffman, checked: ValueError names the setting."""
    return run_options.check(env, "png_huffman")


def _stem(data_path):
    name = data_path[0] if isinstance(data_path, (list, tuple)) else data_path
    return name.split("/")[-1][:-4]              # the reference's rule (:78): basename minus a 4-character extension


def visualize_dewarping(settings, sample, data, i, source_vis, data_path, ref_flow=None, *, warped_u8=None):
    """Returns the uint8 [H,W,3] image it wrote (the reference returns None): a NumPy array with png_encoder 'pil', the
    DEVICE tensor with 'hip' and with page_format 'jpeg' (the page is never copied to the host there)."""
    opts = PageOptions.from_env(settings.env)
    encoder = opts.page_writer                   # 'pil' | 'hip' | 'jpeg'
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
            ops.jpeg_encode_to_file(warped_u8, f"{out_dir}/dewarped_pred/warped_{_stem(data_path)}.jpg", opts.jpeg_quality,
                                    opts.jpeg_subsampling)
        else:
            ops.png_encode_to_file(warped_u8, f"{out_dir}/dewarped_pred/warped_{_stem(data_path)}.png", opts.png_huffman)
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
