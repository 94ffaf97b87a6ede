"""Per-installation settings of the sampling run: same attribute surface as the reference's
admin/local.py (every name the sampling path or `args_to_dict` reads), expressed as a table.
Engine-side additions are at the end."""

_DEFAULTS = {
    # directories
    "workspace_dir": "checkpoints",
    # what to evaluate on: 'synthetic' generates documents on the fly; any other name expects
    # per-document conditioning .npz files in `conditioning_dir`
    "eval_dataset_name": "synthetic",
    "eval_dataset": "",
    "dataset_name": "doc3d",
    "time_variant": True,
    # live model / loop configuration (reference admin/local.py:27-35,55-69,81-84)
    "train_mode": "stage_1_dit_cross",
    "iter": True,
    "train_VGG": True,
    "use_gt_mask": False,
    "use_line_mask": True,
    "use_init_flow": False,
    "diffusion_steps": 3,
    "image_size": 64,
    "flow_size": (64, 64),
    "num_channels": 128,
    "num_res_blocks": 3,
    "num_heads": 4,
    "num_heads_upsample": -1,
    "attention_resolutions": "16,8",
    "dropout": 0.0,
    "learn_sigma": False,
    "sigma_small": False,
    "class_cond": False,
    "noise_schedule": "cosine",
    "use_kl": False,
    "predict_xstart": True,
    "rescale_timesteps": True,
    "rescale_learned_sigmas": True,
    "use_checkpoint": False,
    "use_scale_shift_norm": True,
    "clip_denoised": False,
    "timestep_respacing": "",
    "n_batch": 2,            # hypotheses per document
    "visualize": True,
    "use_sr_net": False,
    "val_batch_size": 1,
    "model_path": "checkpoints/model1852000.pt",
    "seg_model_path": "checkpoints/seg.pth",
    "line_seg_model_path": "checkpoints/line_model2.pth",
    "new_seg_model_path": "checkpoints/seg_model.pth",
    # ---- engine-side additions (defaults reproduce the reference's behaviour) ----
    "grid_size": 64,         # coordinate grid G (reference: fixed 64)
    "batch_docs": 1,         # documents sampled together per GPU (reference: 1)
    "sampler": "ddim",       # 'ddim' | 'ddpm'
    "unwarp_mode": "bilinear",   # interpolation of the full-resolution unwarp tail: 'bilinear' (reference) | 'bicubic'
    # directory of ground-truth scans `<stem>.png`: when set, every dewarped page is scored against its scan with MS-SSIM
    # (ops.ms_ssim_u8; "" = no scoring, nothing else changes); metric_preset: 'docunet' | 'wang' 
    "gt_dir": "",
    "metric_preset": "docunet",
    # which metrics gt_dir scores: 'ms_ssim' | 'ms_ssim,ld' | 'ld'.  'ld' adds the local distortion, the mean length of a dense
    # SIFT-flow field from the scan to the page (ops.ld_u8): logged, written to ld.txt, left in settings.ld
    "gt_metrics": "ms_ssim",
    # True: gt_dir also scores every page with the aligned distortion (ops.ad_u8): the SIFT-flow left after a
    # fitted translation and scale are taken out, weighted by the scan's gradient magnitude; logged, written to ad.txt, left in
    # settings.ad.  With 'ld' in gt_metrics both come from one run of the chain.
    "gt_ad": False,
    # who writes dewarped_pred/warped_<stem>.png: 'pil' (the reference: copy the page to the host, Image.save) | 'hip'
    # (ops.png_encode on the device, only the compressed file crosses to the host; the same pixels, other bytes - DESIGN.md 4.4)
    "png_encoder": "pil",
    # the deflate blocks of the 'hip' PNG encoder: 'fixed' (one fixed-Huffman block per segment) | 'dynamic' (per segment the
    # smaller of a dynamic-Huffman and the fixed block: the same pixels in a file about a third smaller - DESIGN.md 4.4)
    "png_huffman": "fixed",
    # the container of dewarped_pred/warped_<stem>: 'png' (the reference; png_encoder chooses who writes it) | 'jpeg'
    # (warped_<stem>.jpg: baseline JFIF encoded on the device by ops.jpeg_encode, only the file crosses to the host; png_encoder
    # is not consulted - DESIGN.md 4.5)
    "page_format": "png",
    "jpeg_quality": 90,         # 1..100, PIL's `quality` scale (the Annex K tables scaled by the usual rule)
    "jpeg_subsampling": "420",  # '420' | '444'
    # who decodes the input photograph of the image-directory path: 'pil' (the loader decodes on the CPU, the pixels cross to
    # the device) | 'hip' (a .jpg/.jpeg FILE crosses and ops.jpeg_decode makes the same bytes there; a file the device decoder
    # does not cover, and every other format, is decoded by PIL with one log line naming the reason - DESIGN.md 4.6)
    "image_decoder": "pil",
    # who decodes PNG files - the .png photographs of the image-directory path and the ground-truth scans of gt_dir: 'pil' (on
    # the CPU, the pixels cross to the device) | 'hip' (the FILE crosses and ops.png_decode inflates and unfilters it there:
    # the same bytes; a file the device decoder hands back is decoded by PIL with one log line naming the reason - DESIGN.md 4.9)
    "png_decoder": "pil",
    "num_synthetic_docs": 4,
    "full_res": (1024, 768), # synthetic full-resolution source size (H, W)
    "conditioning_dir": "",   # directory of per-document conditioning .npz files (skips ingest + pre-stage nets)
    "num_workers": 0,         # DataLoader workers of the image-directory path (they only decode; the reference: 8)
    # run the pre-stage conditioning nets (GeoTr_Seg_Inf.msk, Seg, line UNet; reference evaluation.py:162-216) on the
    # document images, as the reference does; False = synthetic documents carry random conditioning tensors
    "use_prestage_nets": True,
    # None = only when eval_dataset_name == 'synthetic' (a missing checkpoint on a real dataset raises)
    "synthetic_weights_if_missing": None,
    # GeoTr checkpoint (DocTr's geometry transformer, keys 'module.<...>') read when use_init_flow is True: the reference's
    # reload_model(pretrained_dewarp_model.GeoTr, settings.env.dewarping_model_path) (train_TDiff.py:89)
    "dewarping_model_path": "",
}


class EnvironmentSettings:
    def __init__(self):
        for key, value in _DEFAULTS.items():
            setattr(self, key, value)
        self.tensorboard_dir = self.workspace_dir
        self.pretrained_networks = self.workspace_dir
        self.pre_trained_models_dir = self.workspace_dir + "/backup"
