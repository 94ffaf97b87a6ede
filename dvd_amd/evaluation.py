"""Per-document driver of the sampling path - mirror of train_settings/dvd/evaluation.py
(`run_sample_lr_dewarping` :80-138, `run_evaluation_docunet` :142-327, both with the reference's positional signatures) on
the HIP engine.

Documents arrive either as decoded images (dict key "image_u8": [H,W,3] uint8 RGB) - then the ingest kernel
(doc_benchmark.py:75-97) and the pre-stage conditioning nets (evaluation.py:162-216, dvd_amd/prestage.py) run first -
as JPEG files (key "file_bytes", env.image_decoder = 'hip': decoded on the device first, `decode_documents`), or as dicts
of ready conditioning tensors (synthetic or loaded from .npz), i.e. exactly the tensors those nets produce."""
from __future__ import annotations

import os
import re
import time

import numpy as np
import torch as th

from . import ops, run_options, synth
from .run_options import FLOW_OUTPUTS, GT_METRICS, INVERSE_OUTPUTS, parse_gt_metrics  # noqa: F401 - these are imported from here
from .run_options import SCORE, SCORES, RoundOptions, RunOptions

MAP_SCORE_COLUMNS, MAP_SCORE_LOGGED = SCORE["map_score"].columns, SCORE["map_score"].logged           # map_score.txt; the log line
MAP_INVERSE_COLUMNS, MAP_INVERSE_LOGGED = SCORE["map_inverse"].columns, SCORE["map_inverse"].logged
map_score_means = SCORE["map_score"].means      # {key: mean over the documents that have a finite value for it} of settings.map_score


def run_dir(settings):
    """Where a round writes: its pictures, its predicted maps and its score sheets."""
    return f"vis_hp/{settings.env.eval_dataset_name}/{settings.name}"


def page_name(path):
    """The file name a document's page is written under: its path, as a .png when it has no extension."""
    return path if os.path.splitext(path)[1] else path + ".png"


def page_stem(path):
    """The <stem> of warped_<stem>.png and of every other per-document file."""
    from utils_flow.visualization_utils import _stem
    return _stem([page_name(path)])


def run_sample_lr_dewarping(settings, logger, diffusion, model, radius, source, feature_size, raw_corr, init_flow, c20,
                            source_64, pyramid, doc_mask, seg_map_all=None, textline_map=None, init_feat=None, *, noise_keys=None,
                            keep_hypotheses=False):
    """One batch of documents through the sampler, with the reference's positional signature (evaluation.py:80-138; call
    site :247-265): returns the clamped flow [B,2,G,G].  `radius`, `raw_corr`, `source_64` and `pyramid` are dead in the
    reference's body as well (the correlation code is commented out, the conv pyramid belongs to the denoiser); `c20` is
    the reference's `src_feat`, None on the live configuration (train_VGG=True, :219-221).  B = source.shape[0] documents
    are sampled in one engine batch (the reference: B = 1).  noise_keys (keyword only, an extension): one (k0, k1) pair per
    document, handed to the loop in sampling_kwargs - the sampler's noise is then keyed per document.
    keep_hypotheses=True (keyword only, an extension): returns (flow, hypotheses), the second the clamped per-sample maps
    [B*n_batch,2,G,G] the mean was taken over (sampling_kwargs["keep_hypotheses"])."""
    kw = {"init_flow": init_flow, "src_feat": c20, "src_64": None, "y512": source, "tmode": settings.env.train_mode,
          "mask_cat": doc_mask, "init_feat": init_feat, "iter": settings.env.iter}
    if not settings.env.use_gt_mask:
        kw["mask_y512"] = seg_map_all
    if settings.env.use_line_mask:
        kw["line_msk"] = textline_map
    logger.info("\nStarting sampling")
    B = source.shape[0]
    extra = {}
    sampler = run_options.read(settings.env, "sampler")
    if sampler != "ddim":
        extra["sampler_kind"] = sampler                       # engine-side extension (BASELINE configs[3]: 'ddpm')
    sampling_kwargs = {"src_img": source}
    if noise_keys is not None:
        sampling_kwargs["noise_keys"] = list(noise_keys)
    if keep_hypotheses:
        sampling_kwargs["keep_hypotheses"] = True
    sample, final = diffusion.ddim_sample_loop(
        model, (B, 2, feature_size, feature_size), noise=None, clip_denoised=settings.env.clip_denoised,
        model_kwargs=kw, eta=0.0, progress=True, denoised_fn=None, sampling_kwargs=sampling_kwargs, logger=logger,
        n_batch=settings.env.n_batch, time_variant=settings.env.time_variant, pyramid=pyramid, **extra)
    if keep_hypotheses:
        return th.clamp(sample, min=-1, max=1), final["hypotheses"]
    return th.clamp(sample, min=-1, max=1)


def synthetic_documents(settings, indices):
    """Synthetic documents: with env.use_prestage_nets a page-like IMAGE (the whole pipeline runs: ingest -> pre-stage
    nets -> sampler -> unwarp), otherwise random conditioning tensors in the value ranges of SURVEY 8(d)."""
    G = settings.env.grid_size
    for i in indices:
        if run_options.read(settings.env, "use_prestage_nets"):
            h, w = settings.env.full_res
            img = synth.smooth_image(f"doc{i}/image", h, w, seed=1234)
            d = {"image_u8": np.ascontiguousarray((img.transpose(1, 2, 0) * 255.0).astype(np.uint8))}
        else:
            d = synth.synth_document(i, G, seed=1234, full_res=tuple(settings.env.full_res))
        d["path"] = f"synthetic_{i:05d}"
        yield d


def npz_documents(settings, indices, files):
    for i in indices:
        z = np.load(files[i])
        d = {k: z[k] for k in ("y512", "mask_cat", "mask_y512", "line_msk", "src_u8")}
        d["path"] = os.path.splitext(os.path.basename(files[i]))[0]
        yield d


def decode_documents(batch, device, log=None, png=False):
    """Documents that arrive as FILES (`file_bytes`: the 1-D uint8 tensor a Doc_benchmark(decode='hip') or
    Doc_benchmark(decode_png='hip') item carries) get `image_u8` [H,W,3] uint8 on the device - the bytes PIL's decode of the
    file gives, EXIF orientation applied - and `decode_route` ('hip' | 'pil': ops.decode_image).  png (env.png_decoder ==
    'hip'): PNG files go to the device's PNG decoder.  Other documents pass through untouched."""
    for d in batch:
        if "file_bytes" in d and "image_u8" not in d and "y512" not in d:
            d["image_u8"], d["decode_route"] = ops.decode_image(d.pop("file_bytes"), device, log=log, png=png)


def corruption_of(settings):
    """(number, severity) of the run's corruption from `settings.corruption_number` and `settings.severity` (the launcher's
    --corruption rounds), or None when nothing is corrupted: severity 0, whatever the number, or an absent attribute.  A bad
    value is a ValueError that names the attribute; a kind without a kernel is ops.CorruptionUnsupported."""
    severity = ops.corruption_severity(getattr(settings, "severity", 0), "settings.severity")
    if severity == 0:
        return None
    number = ops.corruption_number(getattr(settings, "corruption_number", 0), "settings.corruption_number")
    if not ops.corruption_supported(number):
        raise ops.CorruptionUnsupported(number)
    return number, severity


def corrupt_documents(batch, device, kind, severity, seed):
    """The corruption stage, between ingest and the pre-stage nets: every document's 512 x 512 network input
    y512 = k / 255 is replaced by the corrupted bytes k' / 255, in one launch for the batch, keyed per document by
    (seed, path).  `src_u8`, the photograph the page is unwarped from, stays clean.  A document that arrives with ready
    conditioning tensors cannot be corrupted consistently (its nets saw the clean image): a ValueError that names it."""
    for d in batch:
        if "y512" not in d or any(k in d for k in ("mask_cat", "mask_y512", "line_msk")):
            raise ValueError(f"{d.get('path')}: a document with ready conditioning tensors cannot be corrupted (its pre-stage "
                             "nets ran on the clean image): give the image, or run with settings.severity = 0")
    y = th.stack([_on_device(d["y512"], device).float() for d in batch]).contiguous()
    keys = [ops.corruption_key(seed, d["path"]) for d in batch]
    y = ops.rgb8_to_unit(ops.corrupt_rgb8(ops.unit_to_rgb8(y), kind, severity, keys))
    for j, d in enumerate(batch):
        d["y512"] = y[j]


def prepare_conditioning(batch, device, grid, prestage_models, use_init_flow=False, decode_png=False, *, corrupt=None):
    """Documents given as decoded images: ingest (cv2.resize to 512^2, / 255; doc_benchmark.py:84-88) and the pre-stage
    nets (evaluation.py:162-216) fill in y512 / mask_cat / mask_y512 / line_msk / src_u8 as DEVICE tensors.  Documents
    that already carry their conditioning tensors (synthetic ones with env.use_prestage_nets=False, .npz files of
    env.conditioning_dir) pass through untouched and need no pre-stage nets.  use_init_flow: every document also gets
    `init_flow` [2,G,G] from GeoTr (evaluation.py:172-178), in the same pre-stage pass when that runs.  corrupt: None, or
    (kind, severity, seed): `corrupt_documents` runs between ingest and the nets."""
    from . import prestage
    decode_documents(batch, device, png=decode_png)
    need_ingest = [d for d in batch if "image_u8" in d and "y512" not in d]
    imgs = [(d["image_u8"] if th.is_tensor(d["image_u8"]) else th.from_numpy(d["image_u8"])).to(device).contiguous()
            for d in need_ingest]
    if len({tuple(im.shape) for im in imgs}) > 1:          # images of different sizes: one launch per stage for the batch
        y, rgbs = ops.ingest_u8_ragged(imgs, swap_rb=False, out_size=512, want_rgb=True)
        for j, d in enumerate(need_ingest):
            d["y512"], d["src_u8"] = y[j], rgbs[j]
    else:                                                   # one image, or images of one size: per image, as before
        for d, img in zip(need_ingest, imgs):
            d["y512"], d["src_u8"] = ops.ingest_u8(img, swap_rb=False, out_size=512, want_rgb=True)
    if corrupt is not None:
        corrupt_documents(batch, device, *corrupt)
    todo =[d for d in batch if any(k not in d for k in ("mask_cat", "mask_y512", "line_msk"))]
    if use_init_flow and (prestage_models is None or prestage_models[0] is None):
        raise RuntimeError("env.use_init_flow needs the GeoTr_Seg_Inf model (pretrained_dewarp_model)")
    if use_init_flow:
        pending = {id(d) for d in todo}
        rest = [d for d in batch if id(d) not in pending and "init_flow" not in d]
        if rest:
            src = th.stack([(d["y512"] if th.is_tensor(d["y512"]) else th.from_numpy(d["y512"])).to(device) for d in rest])
            flow = prestage.init_flow(prestage_models[0], src, grid)
            for j, d in enumerate(rest):
                d["init_flow"] = flow[j]
    if not todo:
        return
    if prestage_models is None:
        raise RuntimeError(f"{len(todo)} document(s) lack mask_cat / mask_y512 / line_msk and the pre-stage nets are not "
                           "loaded (env.use_prestage_nets=False): give ready conditioning tensors or load the nets")
    src = th.stack([(d["y512"] if th.is_tensor(d["y512"]) else th.from_numpy(d["y512"])).to(device) for d in todo])
    cond = prestage.conditioning(*prestage_models, src, grid)
    if use_init_flow and "init_flow" not in cond:
        raise RuntimeError("env.use_init_flow needs GeoTr weights: reload_model(model.GeoTr, env.dewarping_model_path)")
    for j, d in enumerate(todo):
        for k in ("mask_cat", "mask_y512", "line_msk") + (("init_flow",) if use_init_flow else ()):
            d[k] = cond[k][j]


def documents_of(item):
    """One loader item -> the documents it holds.  Two item shapes are accepted:
      * the reference's (doc_benchmark.py:91-97 through `DataLoader(batch_size=b)`): `source_image` [b,3,512,512] f32 in 0..1
        (may be absent: computed on the GPU, see datasets/doc_dataset/doc_benchmark.py), `source_image_ori` [b,3,H,W]
        (0..255, float or uint8), `path` list of b file names;
      * this package's document dicts (`image_u8` [H,W,3] or ready conditioning tensors + `src_u8`, `path` = a stem);
      * a Doc_benchmark(decode='hip') item: `file_bytes` [b,n] (or [n]) uint8, the JPEG file itself, and `path`."""
    if "file_bytes" in item and "path" in item and not isinstance(item["path"], str):   # through DataLoader(batch_size=b)
        return [{"path": path, "file_bytes": item["file_bytes"][j]} for j, path in enumerate(item["path"])]
    if "source_image_ori" not in item and "source_image" not in item:
        return [item]
    ori = item.get("source_image_ori", item.get("source_image"))
    paths = item["path"]
    if isinstance(paths, str):
        paths, ori = [paths], ori[None]
    docs = []
    for j, path in enumerate(paths):
        d = {"path": path, "source_vis": ori[j]}
        if "source_image" in item:
            src = item["source_image"]
            d["y512"] = src[j] if src.dim() == 4 else src
        docs.append(d)
    return docs


def _source_u8(d, device):
    """The full-resolution source of one document as [H,W,3] uint8 on the device, or None when it cannot be had exactly
    (a float `source_image_ori` that is not integer-valued in 0..255: the f32 tail kernel is used then)."""
    if "src_u8" in d:
        v = d["src_u8"]
        return (v if th.is_tensor(v) else th.from_numpy(v)).to(device).contiguous()
    vis = d["source_vis"].to(device)
    if vis.dtype == th.uint8:
        return vis.permute(1, 2, 0).contiguous()
    as_u8 = vis.clamp(0, 255).to(th.uint8)
    if not th.equal(as_u8.to(vis.dtype), vis):
        return None
    return as_u8.permute(1, 2, 0).contiguous()


def gt_candidates(path):
    """File names under env.gt_dir that may hold the ground-truth scan of document `path`, in the order they are tried: the
    document's own stem, then the stem's leading integer (DocUNet: '12_1 copy.png' -> '12_1 copy.png', '12.png')."""
    stem = os.path.splitext(os.path.basename(str(path)))[0]
    names = [stem + ".png"]
    lead = re.match(r"\d+", stem)
    if lead and lead.group(0) != stem:
        names.append(lead.group(0) + ".png")
    return names


def find_gt(gt_dir, path):
    """The ground-truth file of document `path` under gt_dir, or None."""
    for name in gt_candidates(path):
        full = os.path.join(gt_dir, name)
        if os.path.isfile(full):
            return full
    return None


def png_decoder_setting(env):
    """env.png_decoder 'pil' | 'hip': who decodes PNG files (input photographs and ground-truth scans).  Anything else is a
    ValueError."""
    return run_options.check(env, "png_decoder")


def _score_against_gt(settings, logger, path, out, device, opts):
    """The metrics of one dewarped page (uint8 [H,W,3] on the device) against its ground-truth scan, if there is one: MS-SSIM,
    LD and / or AD (opts.gt_metrics), on planes prepared once."""
    from PIL import Image
    metrics = opts.gt_metrics
    gt_file = find_gt(opts.gt_dir, path)
    if gt_file is None:
        logger.info(f"{path} {','.join(metrics)} skipped: no ground truth in {opts.gt_dir}")
        return
    gt = None
    if opts.png_decoder == "hip":
        # the scan is inflated and unfiltered on the device; a file the decoder hands back (or one that is no PNG) takes
        # the host route below, untouched, so that the scores are the same bits either way
        with open(gt_file, "rb") as f:
            data = f.read()
        if data[:8] == ops.PNG_SIGNATURE:
            try:
                gt = ops.png_decode(data, device)
            except ops.PngUnsupported as e:
                logger.info(f"{gt_file}: decoded by PIL, not on the device: {e}")
    if gt is None:
        gt = th.from_numpy(np.ascontiguousarray(np.asarray(Image.open(gt_file).convert("RGB")))).to(device)
    values = ops.gt_metrics_u8(out.contiguous(), gt, metrics, preset=opts.metric_preset)
    for name in metrics:
        logger.info(f"{path} {name} {values[name]:.6f}")
        getattr(settings, name).append((path, values[name]))


def _on_device(v, device):
    return v.to(device) if th.is_tensor(v) else th.from_numpy(v).to(device)


def _stack(batch, key, device):
    return th.stack([_on_device(d[key], device) for d in batch]).contiguous()


def batches_of(val_loader, size):
    """The loader's documents (`documents_of`) in lists of `size`; the last one may be shorter."""
    batch = []
    for item in val_loader:
        for d in documents_of(item):
            batch.append(d)
            if len(batch) == size:
                yield batch
                batch = []
    if batch:
        yield batch


def adopt_reference_items(batch, device):
    """Reference-shaped items (`source_vis`): the source as `src_u8` for the tail and, without a `source_image`, as `image_u8`
    for ingest."""
    for d in batch:
        if "source_vis" in d and "src_u8" not in d:
            u8 = _source_u8(d, device)
            if u8 is not None:
                d["src_u8"] = u8
                if "y512" not in d:
                    d["image_u8"] = u8
            elif "y512" not in d:
                raise ValueError(f"{d['path']}: no 'source_image' and a non-integer 'source_image_ori' to make it from")


def sample_batch(settings, logger, diffusion, model, batch, grid, device, *, keyed_noise=None, keep_hypotheses=False):
    """The conditioned documents of one batch through `run_sample_lr_dewarping` (evaluation.py:247-265): the flow [B,2,G,G].
    keyed_noise (None: settings.keyed_noise): the sampler's noise is keyed per document by (settings.seed, path), the
    corruption stage's key; False calls the sampler exactly as ever.  keep_hypotheses=True: (flow, the per-sample maps
    [B*n_batch,2,G,G]) - the map score's spread needs them."""
    nb = len(batch)
    src, msk, seg, line = (_stack(batch, k, device) for k in ("y512", "mask_cat", "mask_y512", "line_msk"))
    init_flow = _stack(batch, "init_flow", device) if settings.env.use_init_flow else th.zeros(nb, 2, grid, grid, device=device)  # :176-181
    extra = {}
    if run_options.check(settings, "keyed_noise") if keyed_noise is None else keyed_noise:
        extra["noise_keys"] = [ops.corruption_key(getattr(settings, "seed", 0), d["path"]) for d in batch]
    if keep_hypotheses:
        extra["keep_hypotheses"] = True
    return run_sample_lr_dewarping(settings, logger, diffusion, model, 4, src, grid, None, init_flow, None, None, None, msk,
                                   seg, line, th.zeros(nb, 256, grid, grid, device=device), **extra)


def score_map_deviation(settings, logger, batch, flow, clean):
    """settings.keyed_noise, after a batch is sampled.  A document that has a reference map in
    `settings.map_ref` is scored against it: ops.map_deviation, one log line, an entry of `settings.map_dev`.  A document
    without one leaves its map there when the round is clean, and gets one log line and no score when it is corrupted."""
    have = [j for j, d in enumerate(batch) if d["path"] in settings.map_ref]
    if have:
        ref = th.stack([settings.map_ref[batch[j]["path"]] for j in have]).to(flow.device).contiguous()
        got = (flow if len(have) == len(batch) else flow[have]).float().contiguous()
        for j, value in zip(have, ops.map_deviation(ref, got)):
            logger.info(f"{batch[j]['path']} map_dev {value:.6f}")
            settings.map_dev.append((batch[j]["path"], value))
    for j, d in enumerate(batch):
        if j in have:
            continue
        if clean:
            settings.map_ref[d["path"]] = flow[j].cpu()
        else:
            logger.info(f"{d['path']} map_dev skipped: no clean round has left a reference map")


def unwarp_tail(batch, flow, mode, device):
    """The full-resolution pages of one batch (:301-306 + viz :75-77) as a list of uint8 [H,W,3] device tensors: one launch
    for the batch when its documents are byte images."""
    nb = len(batch)
    if all("src_u8" in d for d in batch) and len({tuple(d["src_u8"].shape) for d in batch}) == 1:
        return list(ops.unwarp_u8_batch(flow.contiguous(), _stack(batch, "src_u8", device), mode=mode))
    # byte images of different sizes: still one launch (the ragged tail); a float source that is not a byte image takes the
    # fused f32 tail on its own, truncated like numpy's astype(uint8) (bicubic: the grid and the f32 drop-in kernel, clamped
    # to 0..255 first - bicubic overshoots)
    outs = [None] * nb
    u8 = [j for j, d in enumerate(batch) if "src_u8" in d]
    if u8:
        fl = flow.contiguous() if len(u8) == nb else flow[u8].contiguous()
        srcs = [_on_device(batch[j]["src_u8"], device).contiguous() for j in u8]
        for j, out in zip(u8, ops.unwarp_u8_ragged(fl, srcs, mode=mode)):
            outs[j] = out
    for j, d in enumerate(batch):
        if outs[j] is not None:
            continue
        vis = d["source_vis"].to(device).float()[None].contiguous()
        if mode == "bicubic":
            grid = ops.unwarp_grid(flow[j:j + 1].contiguous(), vis.shape[-2], vis.shape[-1])
            f32 = ops.grid_sample(vis, grid, mode="bicubic")[0]
            # NaN (a non-finite grid value) -> 0, as the u8 kernels give; then np.clip(a, 0, 255).astype(uint8)
            outs[j] = th.nan_to_num(f32, nan=0.0).clamp(0, 255).to(th.uint8).permute(1, 2, 0).contiguous()
        else:
            outs[j] = ops.unwarp_f32(flow[j:j + 1].contiguous(), vis).to(th.uint8)
    return outs


def write_flow_outputs(settings, logger, d, flow, h, w, outputs, huffman="fixed"):
    """The predicted map of one document (`flow` [2,G,G], what the unwarp tail consumed) under pred_flow/ (DESIGN.md 4.12):
    'png' flow_<stem>.png, the colour-wheel picture of its displacement at the page's size h x w with norm 'max', and one log
    line with the largest radius; 'flo' flow_<stem>.flo, that displacement; 'npy' flow_<stem>.npy, the coarse map itself -
    what ops.unwarp_u8 needs to redo the page."""
    out_dir = f"{run_dir(settings)}/pred_flow"
    os.makedirs(out_dir, exist_ok=True)
    base = f"{out_dir}/flow_{page_stem(d['path'])}"
    flow = flow.detach().float().contiguous()
    if "png" in outputs:
        _, largest = ops.flow_picture_to_file(flow, h, w, base + ".png", norm="max", huffman=huffman, return_radius=True)
        logger.info(f"{d['path']} flow_rad_max {largest:.6f}")
    if "flo" in outputs:
        ops.flow_write_flo(flow, h, w, base + ".flo")
    if "npy" in outputs:
        np.save(base + ".npy", flow.cpu().numpy())


def gt_map_candidates(path):
    """File names under settings.gt_map_dir that may hold the ground-truth map of document `path`, in the order they are tried:
    per stem of `gt_candidates` <stem>.flo, flow_<stem>.flo, <stem>.npy, flow_<stem>.npy."""
    names = []
    for png in gt_candidates(path):
        stem = os.path.splitext(png)[0]
        names += [stem + ".flo", f"flow_{stem}.flo", stem + ".npy", f"flow_{stem}.npy"]
    return names


def find_gt_map(gt_map_dir, path):
    """The ground-truth map file of document `path` under gt_map_dir, or None."""
    for name in gt_map_candidates(path):
        full = os.path.join(gt_map_dir, name)
        if os.path.isfile(full):
            return full
    return None


def score_against_gt_maps(settings, logger, batch, flow, hyps, outs, gt_map_dir):
    """settings.gt_map_dir, after a batch is sampled and unwarped: every document with a ground-truth map is
    scored by ops.map_score - a .flo file is a displacement field in pixels at its own h x w, a .npy file a coarse map [2,g,g]
    evaluated at the page's size - with one log line and an entry (path, dict) of `settings.map_score`.  hyps [B*H,2,G,G] are
    the sampler's per-sample maps; with H = 1 the sparsification part is skipped with one log line."""
    n_hyp = int(hyps.shape[0]) // len(batch)
    for j, (d, out) in enumerate(zip(batch, outs)):
        path = d["path"]
        gt_file = find_gt_map(gt_map_dir, path)
        if gt_file is None:
            logger.info(f"{path} map_score skipped: no ground-truth map in {gt_map_dir}")
            continue
        if gt_file.endswith(".flo"):
            gt, size = th.from_numpy(ops.flow_read_flo(gt_file)).to(flow.device), None
        else:
            coarse = np.load(gt_file)
            if coarse.ndim != 3 or coarse.shape[0] != 2 or coarse.shape[1] != coarse.shape[2]:
                raise ValueError(f"{gt_file}: a ground-truth .npy must hold a coarse map [2,g,g], got {coarse.shape}")
            gt, size = th.from_numpy(np.ascontiguousarray(coarse, np.float32)).to(flow.device), (int(out.shape[0]), int(out.shape[1]))
        mine = hyps[j * n_hyp:(j + 1) * n_hyp].float().contiguous() if n_hyp >= 2 else None
        if mine is None:
            logger.info(f"{path} map_score: one hypothesis, no spread: sparsification skipped")
        score = ops.map_score(flow[j].detach().float().contiguous(), gt, mine, size=size)
        logger.info(f"{path} map_score " + " ".join(f"{k} {SCORE['map_score'].cell(score, k)}" for k in MAP_SCORE_LOGGED))
        settings.map_score.append((path, score))


def _photograph_u8(d, device):
    """The document's photograph as uint8 [H,W,3] on the device: its byte image, or its float image truncated."""
    if "src_u8" in d:
        return _on_device(d["src_u8"], device).contiguous()
    return d["source_vis"].to(device).float().clamp(0, 255).to(th.uint8).permute(1, 2, 0).contiguous()


def write_inverse_outputs(settings, logger, batch, flow, outs, outputs, device, huffman="fixed"):
    """settings.inverse_outputs, after a batch is unwarped: every document's predicted map is inverted at its
    photograph's size (ops.map_invert, ops.map_cycle_error), with one log line and an entry (path, dict) of
    `settings.map_inverse`; under pred_flow/ 'mesh' writes mesh_<stem>.png, the page mesh on the photograph, 'flo'
    inv_<stem>.flo, the forward displacement (1e10 where the page does not reach), 'mask' mask_<stem>.png, 255 where it does."""
    out_dir = f"{run_dir(settings)}/pred_flow"
    os.makedirs(out_dir, exist_ok=True)
    for j, (d, out) in enumerate(zip(batch, outs)):
        path, stem = d["path"], page_stem(d["path"])
        h, w = int(out.shape[0]), int(out.shape[1])
        mine = flow[j].detach().float().contiguous()
        fwd, stats = ops.map_invert(mine, h, w)
        cycle = ops.map_cycle_error(mine, fwd)
        score = {"covered": stats["covered"], "fold_px": stats["fold_px"], "flipped": stats["flipped_tris"],
                 "degenerate": stats["degenerate_tris"], "skipped": stats["skipped_tris"], "tris": stats["tris"],
                 "cycle_mean": cycle["cycle_mean"], "cycle_max": cycle["cycle_max"],
                 "fold": stats["fold_px"] / stats["covered"] if stats["covered"] else float("nan"), "cycle": cycle["cycle_mean"]}
        logger.info(f"{path} map_inverse " + " ".join(f"{k} {SCORE['map_inverse'].cell(score, k)}" for k in MAP_INVERSE_LOGGED))
        settings.map_inverse.append((path, score))
        if "mesh" in outputs:
            ops.mesh_overlay_to_file(_photograph_u8(d, device), fwd, f"{out_dir}/mesh_{stem}.png", huffman=huffman)
        if "flo" in outputs:
            ops.inverse_write_flo(fwd, f"{out_dir}/inv_{stem}.flo")
        if "mask" in outputs:
            ops.png_encode_to_file(ops.coverage_mask(fwd), f"{out_dir}/mask_{stem}.png", huffman)


def emit(settings, logger, batch, outs, results, opts, device, *, flow=None, flow_outputs=()):
    """The pages of one batch into `results`; the picture if env.visualize, the scores if env.gt_dir; the maps `flow` [B,2,G,G]
    as the files `flow_outputs` names (settings.flow_outputs)."""
    for j, (d, out) in enumerate(zip(batch, outs)):
        results.append((d["path"], out))
        if flow_outputs:
            write_flow_outputs(settings, logger, d, flow[j], int(out.shape[0]), int(out.shape[1]), flow_outputs, opts.png_huffman)
        if settings.env.visualize:
            from utils_flow.visualization_utils import visualize_dewarping
            visualize_dewarping(settings, None, d, len(results) - 1, None, [page_name(d["path"])], warped_u8=out)
        if opts.gt_dir:
            _score_against_gt(settings, logger, d["path"], out, device, opts)


def enabled_scores(opts, round_opts):
    """The rows of SCORES that this round keeps: the metrics env.gt_dir scores, and the kinds whose round switch is on."""
    metrics = opts.gt_metrics if opts.gt_dir else ()
    return [kind for kind in SCORES if (kind.name in metrics if kind.switch is None else getattr(round_opts, kind.switch))]


def write_score_sheet(settings, logger, kind, documents):
    """The end of a round for one score kind: `settings.<kind.name>` as <kind.name>.txt in the run's directory - one line per
    scored document, under a header when the values are dicts - and its means over the scored of `documents` documents."""
    scores = getattr(settings, kind.name)
    with open(f"{run_dir(settings)}/{kind.name}.txt", "w") as f:
        if kind.columns:
            f.write("path " + " ".join(kind.columns) + "\n")
        for path, value in scores:
            f.write(f"{path} " + " ".join(kind.cell(value, k) for k in kind.columns or (kind.name,)) + "\n")
    if not scores and kind.none:
        logger.info(f"mean {kind.name}: no document of {documents} has {kind.none.format(settings=settings)}")
    for k, mean in kind.means(scores, kind.mean_keys).items():
        logger.info(f"{kind.mean_words}{k} {mean:.6f} over {len(kind.values(scores, k))} of {documents} documents")


def summarize(settings, logger, kinds, times, documents, clean):
    """The end of a round: the timing, then the sheet and the means of every score kind the round kept."""
    if times:
        print(len(times))
        print("Elapsed time:{:.2f} avg_second ".format(sum(times) / len(times)))
    for kind in kinds:
        if kind.clean_rounds or not clean or getattr(settings, kind.name):
            write_score_sheet(settings, logger, kind, documents)


def run_evaluation_docunet(settings, logger, val_loader, diffusion, model, pretrained_dewarp_model,
                           pretrained_line_seg_model=None, pretrained_seg_model=None):
    """Document loop with the reference's positional signature (evaluation.py:142-327; call site val_TDiff.py:103-104).
    `val_loader` yields the reference's dicts or this package's documents (`documents_of`); env.batch_docs of them go through
    each pass (the reference: 1): adopt, ingest + pre-stage nets (:162-216, with the corruption stage between them), the sampler
    (:247-265), the map deviation, the unwarp tail, the map score, the map inverse, then per document the map files, the picture
    and the env.gt_dir metrics.  Every switch - env.* (RunOptions), settings.severity / corruption_number, then the round's own
    (RoundOptions) - is read and checked once, before the loader is touched and before anything is written; one that is absent
    or off calls nothing, writes nothing and logs nothing.  The round's scores (run_options.SCORES) start empty and end as
    score sheets beside the pictures.  The pre-stage models may all be None when every document carries ready conditioning
    tensors.  Returns [(path, uint8 [H,W,3] device tensor)] (the reference returns None)."""
    opts = RunOptions.from_env(settings.env)
    corruption = corruption_of(settings)
    round_opts = RoundOptions.from_settings(settings)
    # what is absent or off adds no keyword: the stages are called exactly as they were before the switch existed
    stage, sampling = {}, {}
    if corruption is not None:
        logger.info(f"corruption {corruption[0]} ({ops.CORRUPTIONS[corruption[0]]}) severity {corruption[1]}")
        stage["corrupt"] = (*corruption, getattr(settings, "seed", 0))
    if round_opts.keyed_noise:
        sampling["keyed_noise"] = True
    if round_opts.gt_map_dir:
        sampling["keep_hypotheses"] = True      # the map score's spread needs the per-sample maps
    device = next(model.parameters()).device
    nets = (pretrained_dewarp_model, pretrained_seg_model, pretrained_line_seg_model)
    prestage_models = None if all(m is None for m in nets) else nets
    os.makedirs(run_dir(settings), exist_ok=True)
    kinds = enabled_scores(opts, round_opts)
    for kind in kinds:
        setattr(settings, kind.name, [])        # a round's scores are its own; the reference maps outlive the round
    if round_opts.keyed_noise and not isinstance(getattr(settings, "map_ref", None), dict):
        settings.map_ref = {}
    times, results = [], []
    for batch in batches_of(val_loader, opts.batch_docs):
        adopt_reference_items(batch, device)
        prepare_conditioning(batch, device, opts.grid_size, prestage_models, bool(settings.env.use_init_flow),
                             decode_png=opts.png_decoder == "hip", **stage)
        t0 = time.time()
        flow = sample_batch(settings, logger, diffusion, model, batch, opts.grid_size, device, **sampling)
        if round_opts.gt_map_dir:
            flow, hyps = flow
        th.cuda.synchronize()
        times.append((time.time() - t0) / len(batch))
        if round_opts.keyed_noise:
            score_map_deviation(settings, logger, batch, flow, clean=corruption is None)
        outs = unwarp_tail(batch, flow, opts.unwarp_mode, device)
        if round_opts.gt_map_dir:
            score_against_gt_maps(settings, logger, batch, flow, hyps, outs, round_opts.gt_map_dir)
        if round_opts.inverse_outputs:
            write_inverse_outputs(settings, logger, batch, flow, outs, round_opts.inverse_outputs, device, opts.png_huffman)
        maps = {"flow": flow, "flow_outputs": round_opts.flow_outputs} if round_opts.flow_outputs else {}
        emit(settings, logger, batch, outs, results, opts, device, **maps)
    summarize(settings, logger, kinds, times, len(results), clean=corruption is None)
    return results
