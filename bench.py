#!/usr/bin/env python3
"""Headline benchmark: documents/second of the DvD sampling path on MI355X.

  python bench.py --gpus N --steps K --warmup W
  N > 1 works both ways: under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...`
  (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment), and typed bare - `python bench.py --gpus N` with no
  WORLD_SIZE set starts its own N rank processes (launch_ranks: fresh children, one per GPU, 127.0.0.1 rendezvous;
  the parent never touches the GPU) and relays rank 0's line.

One "step" = one pass of the hot path over one batch of documents (BASELINE.json configs[1]):
  8 documents x 2 hypotheses per GPU, 50-step DDIM on the 288x288 coordinate grid
  = per-document conditioning (conv pyramid, c/m/l embeddings, their K/V)   [dvd_engine_prepare_docs]
  + 50 x denoiser evaluation + fused DDIM step                              [dvd_engine_denoise_step, dvd_sched_step]
  + hypothesis mean/clamp + full-resolution (3508x2480) u8 unwarp           [dvd_hyp_mean_clamp, dvd_unwarp_u8]
with every input already resident in HBM.  Documents shard across ranks with no data-path
collective (weak scaling, 8 docs per GPU); the only collective is the one-shot RCCL broadcast of the
packed weight blob from rank 0.  Synthetic inputs and weights (no checkpoint / dataset offline).

Rank 0 prints ONE JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step = wall milliseconds of one
timed step) that also carries
  roofline     : the dominant kernel (head_dim-256 decoder flash attention), timed per launch with HIP
                 events on the launch stream inside the timed region, against the dense f16 MFMA peak.
A plain run does nothing else: set-up, warm-up, the timed steps, the optional output dump, the line.
--full adds what takes work of its own after the timed steps (its fields are null without it):
  roofline_unwarp : the full-resolution gather, timed in launches of its own;
  cpu_baseline    : the CPU oracle (a port pinned to the reference by golden vectors) timed on this
                    host's cores on a bounded sample and scaled to documents/s, with three full-size parity checks;
  other_configs   : bounded legs for the other BASELINE.json configurations, each with a parity figure.
--dump-outputs DIR writes what the last timed step returned on rank 0 (see dump_outputs); the inputs and weights
are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

_T_PROCESS_START = time.perf_counter()
CFG3_FULL_DEADLINE_S = 480        # other_configs: configs[3] runs its stated 32 documents (5.6 minutes) only if, projected from the
                                  # north_star_batch32 leg's time, the leg would end this young; else 4 documents: a --full run
                                  # with a few steps has to end within 10 minutes
DUMP_ELEMS = 1 << 22              # --dump-outputs: at most this many values per array (16 MiB of f32), a seeded sample above it

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F16_TFLOPS = 2500.0      # dense f16/bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0         # HBM3E, same guide
PROFILE_ROUND = "r6"          # which profiles/<round>_pmc_*.json this bench.py's kernels were measured for
HID, DEC, FFN = 384, 1536, 2048


def step_flops(grid):
    """Algorithmic FLOPs of ONE denoiser evaluation for ONE sample (live block only, invariants hoisted;
    SURVEY Appendix A.7) and the share of the head_dim-256 decoder attention."""
    T = (grid // 2) ** 2
    D, E, F = HID, DEC, FFN
    block = 2 * T * 8 * D + 2 * T * 1032 * D + (2 * T * D * D + 4 * T * D * D + 4 * 4 * T * T * D + 4 * 2 * T * D * D) \
        + (4 * 6 * T * D * D + 4 * 4 * T * T * D + 4 * 2 * T * D * D) + 4 * 16 * T * D * D
    dec = 6 * (6 * T * E * E + 4 * T * T * E + 2 * T * E * E + 4 * T * E * F + 18 * T * F) + 16 * T * E
    return block + dec, 4 * T * T * E          # (total per sample-step, one decoder-attention launch per sample)


def faithful_step_flops(grid):
    """FLOPs of ONE denoiser evaluation for ONE sample the way the reference EXECUTES it (idf/cross_model.py:584-616):
    all 12 DiT blocks (11 of them dead compute), the conv pyramid, the c/m/l embeddings and their K/V projections
    recomputed at every step (708.8 GFLOP at G=64)."""
    T = (grid // 2) ** 2
    D, E, F = HID, DEC, FFN
    embeds = 2 * T * 8 * D + 2 * T * 1032 * D + 2 * T * 4 * (256 + 384 + 64) * D
    blk = (2 * T * D * D + 4 * 4 * T * D * D + 4 * 4 * T * T * D + 4 * 2 * T * D * D) \
        + (4 * 6 * T * D * D + 4 * 4 * T * T * D + 4 * 2 * T * D * D) + 4 * 16 * T * D * D
    dec = 6 * (6 * T * E * E + 4 * T * T * E + 2 * T * E * E + 4 * T * E * F + 18 * T * F) + 16 * T * E
    return 97.84e9 + embeds + 12 * blk + dec


def workload_name(B, H, S, sampler, G, FH, FW, world):
    """Which BASELINE.json configuration (if any) this run is."""
    key = (B, S, sampler, G)
    tag = {(8, 50, "ddim", 288): "BASELINE configs[1]" if world == 1 else "BASELINE configs[2] shape (8 documents/GPU)",
           (32, 250, "ddpm", 288): "BASELINE configs[3]", (16, 50, "ddim", 288): "BASELINE configs[4]"}.get(key)
    if tag == "BASELINE configs[2] shape (8 documents/GPU)" and world == 8:
        tag = "BASELINE configs[2]"
    desc = (f"batch={B} documents/GPU x {H} hypotheses, {S}-step {sampler.upper()}, {G}x{G} coordinate grid, "
            f"+ {FH}x{FW} u8 unwarp")
    return f"{tag}: {desc}" if tag else f"custom (not a BASELINE.json configuration): {desc}"


def init_dist(world, local, backend=None):
    """One process per GPU under torch.distributed.run (env:// rendezvous); backend 'nccl' IS RCCL on ROCm."""
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend is None:
            backend = "nccl"
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)


def broadcast_weights(blob, world, sync=None):
    """The path's only collective: ONE flat broadcast of the packed weight blob from rank 0.  Returns ms (None at 1 rank)."""
    if world == 1:
        return None
    sync = sync or (lambda: None)
    sync()
    dist.barrier()
    t0 = time.perf_counter()
    dist.broadcast(blob, src=0)
    sync()
    return (time.perf_counter() - t0) * 1e3


LAUNCH_DEADLINE_S = 3 * 3600      # launch_ranks: no run of this bench is longer; a hung rank must not block the parent for ever


def launch_ranks(n, argv, deadline_s=None, attempts=3):
    """`python bench.py --gpus N` typed without a launcher: start N fresh rank processes of this same script (one per
    GPU, env:// rendezvous on 127.0.0.1 - the reference's own set-up, idf/dist_util.py:21-41, minus MPI), let them print
    (only rank 0 does), and return the worst exit code (a signal exit -s is reported as 128 + s).  The parent has not
    touched the GPU and never will: nothing is re-exec'd, the ranks are children.
    A rank that dies takes the others down after a grace period (terminate, then kill: a rank stuck in a GPU collective may
    ignore SIGTERM); an overall deadline does the same for a rank that hangs without dying; the free-port probe is racy by
    nature (the socket is closed before rank 0 binds it): when rank 0 ALONE is down within seconds of the start the others
    are taken down after a short grace and the run is retried on a new port; any other failure is reported as it is."""
    import socket
    import subprocess
    deadline_s = LAUNCH_DEADLINE_S if deadline_s is None else deadline_s
    worst = 0
    for attempt in range(attempts):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get(
                           "HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
        t_start, failed_at, term_at, rank0_first = time.monotonic(), None, None, False
        while any(p.poll() is None for p in procs):
            now = time.monotonic()
            if failed_at is None and (any(p.poll() not in (None, 0) for p in procs) or now - t_start > deadline_s):
                failed_at = now                              # a rank died (the others would wait in a collective for ever) or hangs
                # the port race: rank 0 alone dies at once (EADDRINUSE on MASTER_PORT) while the others sit in the store's
                # connect - seen as "rank 0 is down within seconds of the start and some other rank is still up"
                rank0_first = procs[0].poll() not in (None, 0) and now - t_start < 10.0 and any(p.poll() is None for p in procs[1:])
            grace = 2.0 if rank0_first else 20.0
            if failed_at is not None and term_at is None and (now - failed_at > grace or now - t_start > deadline_s):
                term_at = now
                for p in procs:
                    if p.poll() is None:
                        p.terminate()                        # by handle, never by pattern
            if term_at is not None and now - term_at > 10.0:
                for p in procs:
                    if p.poll() is None:
                        p.kill()                             # SIGTERM ignored (stuck in a collective): escalate
            time.sleep(0.2)
        codes = [p.wait() for p in procs]
        codes = [128 - rc if rc < 0 else rc for rc in codes]
        worst = next((rc for rc in codes if rc != 0), 0)
        hung = time.monotonic() - t_start > deadline_s
        # retried: ONLY the rendezvous race (rank 0 gone at once, the others had to be taken down).  Ranks that all exit by
        # themselves with an error (a bad argument, an import error) would fail the same way again: reported, not repeated.
        if worst == 0 or hung or not rank0_first:
            return 124 if hung and worst == 0 else worst
    return worst


def ranks_seen(world, rank, local, backend):
    """All-gathered (rank, local rank, current device, device name) of every rank plus the collective library's version:
    evidence on the line that N distinct GPUs took part and which RCCL carried the broadcast."""
    me = {"rank": rank, "local_rank": local}
    if torch.cuda.is_available():
        me["device"] = int(torch.cuda.current_device())
        me["name"] = torch.cuda.get_device_name(me["device"])
    allr = [None] * world
    if world > 1:
        dist.all_gather_object(allr, me)
    else:
        allr = [me]
    ver = None
    if backend == "nccl":
        try:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:           # noqa: BLE001 - version query only
            ver = None
    return {"ranks": allr, "backend": backend + (" (RCCL)" if backend == "nccl" else ""), "rccl_version": ver}


def max_over_ranks(elapsed, world, dev):
    if world == 1:
        return elapsed
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def per_rank_seconds(elapsed, world, dev):
    """Every rank's own wall time of the timed region (one all_gather AFTER it: report only)."""
    if world == 1:
        return [elapsed]
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    out = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return [float(x.item()) for x in out]


def _dump_sample(t, limit=DUMP_ELEMS):
    """`t` flattened as float32 on the host: whole when it has at most `limit` values, otherwise the values at `limit`
    positions drawn (with repetition, then sorted) by a fixed seed - the same positions for the same shape in every run."""
    flat = t.reshape(-1)
    if flat.numel() > limit:
        idx = np.sort(np.random.default_rng(0).integers(0, flat.numel(), limit))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat.float().cpu().numpy()


def dump_outputs(out_dir, flow, outs):
    """What the timed path returned in its last step, as float32 .npy files:
      flow.npy        [B, 2, G, G] coordinate maps after the hypothesis mean + clamp (flattened when sampled);
      unwarped_u8.npy the batch's full-resolution u8 unwarped images [B, H, W, 3] (a seeded sample of DUMP_ELEMS values
                      at the default 3508x2480)."""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in (("flow", flow), ("unwarped_u8", outs)):
        a = _dump_sample(t)
        np.save(os.path.join(out_dir, f"{name}.npy"), a.reshape(t.shape) if a.size == t.numel() else a)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=0)
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--docs", type=int, default=8, help="documents per GPU per step")
    ap.add_argument("--hyp", type=int, default=2, help="hypotheses per document (reference n_batch)")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--sampler", default="ddim", choices=["ddim", "ddpm"])
    ap.add_argument("--full-res", default="3508x2480")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-split-weights", action="store_true")
    ap.add_argument("--no-ffn-lo", action="store_true", help="opt-in fast mode: drop the lo pass of the decoder FFN convs")
    ap.add_argument("--no-dither", action="store_true", help="round 2's weights: (hi, lo) split in every GEMM, 2x the MFMAs")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the bounded legs for BASELINE configs[3], configs[4] and the reference's native point")
    ap.add_argument("--backend", default="nccl", help="process-group backend (nccl = RCCL; the CPU test of the rank logic uses gloo)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure roofline_unwarp, cpu_baseline (+ parity) and other_configs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0) to DIR/<name>.npy as float32")
    args = ap.parse_args(argv)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # typed bare: be our own launcher (before anything touches the GPU in this process)
        rc = launch_ranks(args.gpus, sys.argv[1:] if argv is None else argv)
        if rc != 0:
            raise SystemExit(rc)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world size and --gpus must agree")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    init_dist(world, local, backend=args.backend)
    seen = ranks_seen(world, rank, local, args.backend)

    from dvd_amd import lib, ops, sampler, schedule, synth
    from dvd_amd.engine import Engine, aligned_empty

    G, B, H, S = args.grid, args.docs, args.hyp, args.ddim_steps
    FH, FW = (int(v) for v in args.full_res.split("x"))
    eng = Engine(G, B, H, device=dev)
    if args.no_split_weights:
        eng.set_option("split_weights", 0)
    if args.no_ffn_lo:
        eng.set_option("ffn_lo", 0)
    if args.no_dither:
        eng.set_option("dither", 0)

    # ---- weights: rank 0 builds + packs, ONE flat RCCL broadcast (the only collective of the path) ----
    _, blob_bytes = eng.blob_layout()
    blob = aligned_empty(blob_bytes, dev)
    if rank == 0:
        sd = synth.synth_state_dict(G, seed=7, blocks=[11])
        blob.copy_(eng.pack_blob(sd))
        del sd
    bcast_ms = broadcast_weights(blob, world, torch.cuda.synchronize)
    eng.bind_blob(blob)

    # ---- synthetic per-rank documents, resident in HBM (value ranges as SURVEY 8(d)) ----
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    y512 = torch.rand(B, 3, 512, 512, device=dev, generator=gen)
    mask_cat = torch.rand(B, 1, 512, 512, device=dev, generator=gen)
    mask_y512 = torch.randn(B, 384, G, G, device=dev, generator=gen).clamp_min_(0)
    line_msk = torch.randn(B, 64, G, G, device=dev, generator=gen).clamp_min_(0)
    x_T = torch.randn(B * H, 2, G, G, device=dev, generator=gen)
    src_u8 = torch.randint(0, 256, (B, FH, FW, 3), device=dev, dtype=torch.uint8, generator=gen)
    tab = schedule.Tables(schedule.named_betas("cosine", S))
    noise_fn = None
    if args.sampler == "ddpm":
        noise_fn = lambda i: torch.randn(B * H, 2, G, G, device=dev, generator=gen)  # noqa: E731

    unwarp_events = []          # (start, end) HIP events around the unwarp launches, on the stream they are launched on

    def one_step(timed=False):
        eng.prepare(y512, mask_cat, mask_y512, line_msk)
        flow = sampler.sample(eng, tab, x_T, sampler=args.sampler, noise_fn=noise_fn)     # [B,2,G,G]
        if timed:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        outs = ops.unwarp_u8_batch(flow, src_u8)                                          # ONE launch for the batch
        if timed:
            ev[1].record()
            unwarp_events.append(ev)
        return flow, outs

    for _ in range(args.warmup):
        one_step()
    eng.profile(True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        flow, outs = one_step(timed=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed_local = time.perf_counter() - t0
    elapsed = max_over_ranks(elapsed_local, world, dev)
    rank_seconds = per_rank_seconds(elapsed_local, world, dev)
    launches, attn_ms = eng.profile_read()
    eng.profile(False)
    assert bool(torch.isfinite(flow).all()), "non-finite coordinates"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, flow, outs)

    if rank == 0:
        docs_total = B * world * args.steps
        value = docs_total / elapsed
        per_sample_step, attn_launch_per_sample = step_flops(G)
        n = B * H
        roof = None
        T = (G // 2) ** 2
        attn_kernel = lib.flash_attn_kernel_name(256, T, T)
        launches_issued = 6 * S * args.steps            # 6 decoder layers x S evaluations x steps
        if launches:
            avg_s = attn_ms / launches * 1e-3
            achieved = attn_launch_per_sample * n / avg_s / 1e12
            roof = {"kernel": f"{attn_kernel} (decoder self-attention, 6 heads x 256)", "bound": "mfma",
                    "achieved": round(achieved, 1), "peak": PEAK_F16_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_F16_TFLOPS, 4), "traffic": None,
                    "algorithmic_bytes_per_launch": 4 * n * T * 1536 * 2,   # Q, K, V^T read + O written, f16
                    "launches_timed": launches, "launches_issued": launches_issued,
                    "avg_launch_ms": round(avg_s * 1e3, 3), "flops_per_launch": attn_launch_per_sample * n,
                    "share_of_step_time": round(attn_ms * 1e-3 / elapsed, 3)}
            # HBM bytes per launch of this kernel come from PMC counters, which need their own rocprofv3 passes
            # (benchmarks/pmc_traffic.sh).  The committed measurement is attached ONLY when it was taken on the very
            # kernel this run launched, at this launch shape - a renamed or re-tiled kernel gets traffic: null.
            here = os.path.dirname(os.path.abspath(__file__))
            for name, field in (("pmc_traffic", "traffic"), ("pmc_mfma", "mfma")):
                path = os.path.join(here, "profiles", f"{PROFILE_ROUND}_{name}.json")
                if not os.path.exists(path):
                    continue
                rec = json.load(open(path)).get(attn_kernel)
                if not rec or rec.get("launch_shape") != {"samples": n, "grid": G}:
                    continue
                if field == "traffic":
                    roof["traffic"] = int(rec["hbm_bytes_per_launch"])
                    roof["traffic_unit"] = "bytes/launch"
                    roof["traffic_source"] = (f"profiles/{PROFILE_ROUND}_{name}.json (rocprofv3 --pmc FETCH_SIZE, "
                                              "WRITE_SIZE in separate passes; 2*FETCH+WRITE, gfx950 correction)")
                else:
                    roof["mfma_busy_pmc"] = rec["mfma_busy"]
                    roof["sustained_clock_ghz_pmc"] = rec["sustained_clock_ghz"]
                    roof["pmc_source"] = f"profiles/{PROFILE_ROUND}_{name}.json"
        # second roofline object: the HBM-bound full-resolution gather.  SURVEY 8(d) prices it on the drop-in
        # grid_sample contract (f32: 12 B/px source + 8 B/px grid + 12 B/px output = 32 B/px), so that kernel is
        # timed here, after the timed region, on this run's own documents (all B in one launch); the fused u8 tail the
        # timed region actually uses (6 B/px algorithmic, VALU-bound) is reported beside it.
        roof_unwarp = None
        if args.full and unwarp_events:
            ms_u8 = sum(a.elapsed_time(b) for a, b in unwarp_events) / len(unwarp_events)
            srcf = src_u8.permute(0, 3, 1, 2).float().contiguous()                        # [B,3,H,W] f32 0..255
            # the gather pattern is set by the flow: the sampler's output under RANDOM synthetic weights is white-noise-
            # like (every pixel samples a random place), which no dewarping flow is; the roofline leg therefore uses a
            # document-like field - bicubic-upsampled 6x6 control points of amplitude 0.05 (up to ~35 degrees of local
            # shear), the field of profiles/archive/r1_warp_summary.txt and benchmarks/op_bench.py
            ctrl = (torch.rand(B, 2, 6, 6, device=dev, generator=gen) - 0.5) * 0.1
            flow_doc = torch.nn.functional.interpolate(ctrl, size=(G, G), mode="bicubic", align_corners=True).contiguous()
            grid_full = torch.cat([ops.unwarp_grid(flow_doc[d:d + 1].contiguous(), FH, FW) for d in range(B)])   # [B,2,H,W]
            ev8 = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ops.unwarp_u8_batch(flow_doc, src_u8)
                b.record()
                ev8.append((a, b))
            for _ in range(2):
                ops.grid_sample(srcf, grid_full)
            evs = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ops.grid_sample(srcf, grid_full)
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            ms = sum(a.elapsed_time(b) for a, b in evs) / len(evs)
            ms_u8_doc = sum(a.elapsed_time(b) for a, b in ev8[1:]) / (len(ev8) - 1)
            bytes_alg = 32 * FH * FW * B
            gs_kernel = "grid_sample_lds_kernel<32, 2048, 0, 0>"
            roof_unwarp = {"kernel": f"{gs_kernel} (drop-in register_model2 contract, f32, LDS-staged 32x32 tiles, {B} "
                                     "documents per launch)", "bound": "hbm", "achieved": round(bytes_alg / (ms * 1e-3) / 1e9, 1),
                           "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(bytes_alg / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                           "traffic": None, "algorithmic_bytes_per_launch": bytes_alg, "launches_timed": len(evs),
                           "avg_launch_ms": round(ms, 4),
                           "flow": "document-like: bicubic-upsampled 6x6 control points, amplitude 0.05 (the sampler's output "
                                   "under random synthetic weights is white-noise-like and not a representative gather)",
                           "fused_u8_tail": {"kernel": "unwarp_u8_rows_kernel (what the timed region runs: upsample + affine "
                                                       f"+ gather + uint8 fused, {B} documents per launch)",
                                             "algorithmic_bytes_per_launch": 6 * FH * FW * B,
                                             "avg_launch_ms_in_timed_region_noise_flow": round(ms_u8, 4),
                                             "launches_timed": len(unwarp_events),
                                             "avg_launch_ms": round(ms_u8_doc, 4),
                                             "achieved_GBps": round(6 * FH * FW * B / (ms_u8_doc * 1e-3) / 1e9, 1),
                                             "note": "bound by its dependent chain per pixel (coarse-flow loads -> taps -> gather -> blend -> "
                                                     "store), not by HBM and not by its instruction count: hoisting a third of the "
                                                     "VALU work out of the rows made it slower (profiles/r6_u8_band_variants.txt)"}}
            # HBM-side bytes of that kernel from the committed PMC passes (FETCH_SIZE / WRITE_SIZE in separate rocprofv3
            # runs, 2*FETCH + WRITE: every streaming access of the kernel is 16 bytes per lane) - attached only when the
            # record was taken on this kernel at this launch shape
            tpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"{PROFILE_ROUND}_pmc_traffic.json")
            if os.path.exists(tpath):
                rec = json.load(open(tpath)).get(gs_kernel)
                if rec and rec.get("launch_shape") == {"documents": B, "h": FH, "w": FW}:
                    roof_unwarp["traffic"] = int(rec["hbm_bytes_per_launch"])
                    roof_unwarp["traffic_unit"] = "bytes/launch"
                    roof_unwarp["traffic_source"] = (f"profiles/{PROFILE_ROUND}_pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE, "
                                                     "WRITE_SIZE in separate passes; 2*FETCH+WRITE, gfx950 correction)")
            del srcf, grid_full
        flops_total = per_sample_step * n * S * world * args.steps
        if not args.no_split_weights:
            pass   # split weights double the GEMM MFMAs; algorithmic FLOPs are unchanged by definition
        cpu = None
        if args.full and not args.no_cpu_baseline and world == 1:
            # engine output for the run's first loop step (all samples; sample 0 is compared with the oracle)
            t_first = tab.model_time(S - 1)
            eng.prepare(y512, mask_cat, mask_y512, line_msk)
            x0_first = eng.denoise(x_T, schedule.embedded_time(t_first), sampler.feat_mode_for(t_first, B * H, True),
                                   torch.zeros_like(x_T), dither_step=0).clone()
            # a second evaluation on the WARPED-feature branch (feat_mode 2: t_model <= 600, init_flow = previous x0,
            # init_feat = grid_sample(feat, (x0 + base) * 2 - 1)) - the branch every step but the first few takes
            i_mid = max(i for i in range(S) if tab.model_time(i) <= 600.0)
            t_mid = tab.model_time(i_mid)
            x0_mid = eng.denoise(x_T, schedule.embedded_time(t_mid), 2, x0_first, dither_step=S - 1 - i_mid).clone()
            check = {"doc": [a[:1].float().cpu() for a in (y512, mask_cat, mask_y512, line_msk)], "x": x_T[:1].cpu(),
                     "t_model": float(t_first), "x0_gpu": x0_first[:1].cpu(),
                     "t_model_warp": float(t_mid), "x0_gpu_warp": x0_mid[:1].cpu()}
            if H > 1:          # third timed sample-step: the first loop step of document 0 / hypothesis 1
                check["x_h1"], check["x0_gpu_h1"] = x_T[1:2].cpu(), x0_first[1:2].cpu()
            cpu = cpu_baseline(G, H, S, check)
            for par in cpu.get("parity") or []:
                if not par["ok"]:
                    raise SystemExit(f"PARITY FAILURE at G={G}: {par}")
        others = None
        if args.full and world == 1 and not args.no_other_configs and (G, S, args.sampler) == (288, 50, "ddim"):
            del y512, mask_cat, mask_y512, line_msk, x_T, src_u8, outs
            eng.workspace = None
            torch.cuda.empty_cache()
            others = other_configs(dev, blob, H, FH, FW, want_cpu=not args.no_cpu_baseline)
        line = {
            "metric": "documents/sec (50-step DDIM, 288x288 grid)" if (G, S, args.sampler) == (288, 50, "ddim")
            else f"documents/sec ({S}-step {args.sampler.upper()}, {G}x{G} grid)",
            "value": round(value, 5), "unit": "documents/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": workload_name(B, H, S, args.sampler, G, FH, FW, world),
                       "docs_per_gpu": B, "hypotheses": H, "sampler_steps": S, "grid": G,
                       "weights": ("synthetic (seed 7), " + (
                           "plain f16 (round-to-nearest once)" if (args.no_split_weights and args.no_dither) else
                           "f16 hi/lo split in every GEMM" if args.no_dither else
                           "f16 re-rounded before every evaluation with a zero-mean step-dependent dither for the "
                           "256-wide GEMMs (one pass), f16 hi/lo split for the 384-wide ones")
                                   + (", decoder-FFN lo pass dropped (opt-in fast mode)" if args.no_ffn_lo else "")),
                       "parallelism": f"dp{world} (documents sharded, one weight broadcast)"},
            "algorithmic_tflops": round(flops_total / elapsed / 1e12, 1),
            "weight_broadcast_ms": None if bcast_ms is None else round(bcast_ms, 2),
            "weight_broadcast_bytes": int(blob_bytes),
            # each rank's own clock over the timed region (the line's value uses the MAX): a scaling run explains itself
            "per_rank": [{"rank": r, "seconds": round(t, 4), "documents_per_s": round(B * args.steps / t, 5)}
                         for r, t in enumerate(rank_seconds)],
            "collectives": {"data_path": 0, "setup": ["all_gather_object (ranks_seen)", "barrier", "broadcast (weights, once)"],
                            "timing": ["barrier", "barrier", "all_reduce MAX (elapsed)", "all_gather (per-rank seconds)", "barrier"]},
            "ranks_seen": seen,
            "roofline": roof, "roofline_unwarp": roof_unwarp, "cpu_baseline": cpu,
            "other_configs": others,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _aten_order_matches_host():
    """oracle/aten_order.py (numpy restatement of the arithmetic order the HIP warps implement) against torch's CPU kernels
    on THIS host, bit for bit, on a small tail (what tests/test_oracle_golden.py::test_aten_order_restatement pins)."""
    from oracle import aten_order as A
    from oracle import dvd_oracle as O
    rng = np.random.RandomState(16)
    flow = (rng.randn(1, 2, 16, 16) * 0.06).astype(np.float32)
    src = (rng.rand(1, 3, 97, 131) * 255).astype(np.float32)
    grid, out, u8 = O.unwarp_tail(torch.from_numpy(flow), torch.from_numpy(src))
    grid2, out2, u82 = A.unwarp_tail(flow, src)
    return bool(np.array_equal(grid.numpy(), grid2) and np.array_equal(out.numpy(), out2) and np.array_equal(u8, u82))


def other_configs(dev, blob288, H, FH, FW, want_cpu=True, legs=("cfg4", "ns32", "cfg3", "native")):
    """Bounded legs for the BASELINE.json configurations the headline is NOT quoted on, each with its own time, value and
    parity figure (the headline fields of the line are untouched):
      configs[4]  16 documents, 50-step DDIM, G = 288, + 3508x2480 unwarp: ONE whole batch;
      ns32        north_star's stated target point: 32 documents, 50-step DDIM, G = 288, + unwarp: ONE whole batch (round 6);
      configs[3]  (parity since round 6: the fused step vs the oracle AND document 0 of the batch after all 250 steps == itself alone)
                  250-step DDPM ancestral sampling at G = 288 at its STATED 32 documents (x H hypotheses = 64 samples, one
                  engine batch, ~5.5 minutes; round 5) - unless the process would be older than CFG3_FULL_DEADLINE_S at its
                  end (projected as 5x the ns32 leg's time; no ns32 leg, no projection), in which case 4 documents are run and
                  the leg says so (the loop is strictly per-document work, so
                  documents/s at 4 per batch is a lower bound of the rate at 32);
      native      the reference's own operating point (admin/local.py:28-35,82: G = 64, 3 DDIM steps, 2 hypotheses, one
                  document at a time) from a decoded IMAGE: ingest + the three pre-stage nets + sampling + unwarp."""
    import statistics
    from dvd_amd import ops, prestage, sampler, schedule, synth
    from dvd_amd.engine import Engine
    out = {}
    ns32_s = None
    G = 288
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)

    def docs(B, grid):
        return (torch.rand(B, 3, 512, 512, device=dev, generator=gen), torch.rand(B, 1, 512, 512, device=dev, generator=gen),
                torch.randn(B, 384, grid, grid, device=dev, generator=gen).clamp_min_(0),
                torch.randn(B, 64, grid, grid, device=dev, generator=gen).clamp_min_(0))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    if "cfg4" in legs:
        # ---- configs[4]: 16 documents + full-resolution unwarp --------------------------------------------------------
        B = 16
        eng = Engine(G, B, H, device=dev)
        eng.bind_blob(blob288)
        cond = docs(B, G)
        x_T = torch.randn(B * H, 2, G, G, device=dev, generator=gen)
        src_u8 = torch.randint(0, 256, (B, FH, FW, 3), device=dev, dtype=torch.uint8, generator=gen)
        tab = schedule.Tables(schedule.named_betas("cosine", 50))

        def cfg4():
            eng.prepare(*cond)
            flow = sampler.sample(eng, tab, x_T)
            return flow, ops.unwarp_u8_batch(flow, src_u8)
        dt, (flow, outs) = timed(cfg4)
        # parity of the leg's own product: document 0's unwarped u8 image against the CPU oracle's tail on the same flow
        par = None
        if want_cpu:
            from oracle import dvd_oracle as O
            srcf = src_u8[0].permute(2, 0, 1)[None].float().cpu()
            _, _, ref8 = O.unwarp_tail(flow[:1].cpu(), srcf)
            got8 = outs[0].cpu().numpy().astype(np.int32)
            d = np.abs(got8 - ref8.astype(np.int32))
            par = {"what": "document 0: fused u8 unwarp (3508x2480) vs the CPU oracle's upsample + grid_sample + uint8 on the "
                           "same flow", "pixels_equal": float((d == 0).mean()), "max_abs_u8": int(d.max()),
                   "ok": bool((d == 0).all()),       # round 5: the tail follows ATen's arithmetic order - the same bytes
                   # byte equality holds while THIS host's torch contracts its CPU kernels into the FMA order the
                   # kernels restate (oracle/aten_order.py); on another torch build / CPU ISA the strict flag could go false
                   # with max_abs_u8 == 1 and nothing changed on the GPU - so the old tolerance and the host check ride along
                   "ok_within_1": bool(d.max() <= 1), "aten_order_matches_host_torch": _aten_order_matches_host()}
        out["configs[4]"] = {"workload": f"BASELINE configs[4]: batch={B} documents x {H} hypotheses, 50-step DDIM, 288x288 grid, "
                                         f"+ {FH}x{FW} u8 unwarp", "batches_timed": 1, "ms_per_batch": round(dt * 1e3, 1),
                             "value": round(B / dt, 5), "unit": "documents/s", "parity": par}
        del eng, cond, x_T, src_u8, outs, flow
        torch.cuda.empty_cache()

    if "ns32" in legs:
        # ---- north_star's stated target point: 50-step DDIM, 288x288 grid, batch = 32 (+ the full-resolution unwarp) ------------
        # (VERDICT r5 missing 7: configs[1] (8) and configs[4] (16) bracket it from below only.)  Parity of the leg's own product:
        # document 0 of the batch must have the bits it has when sampled ALONE (one engine of one document, same x_T) - the
        # kernel choice is a function of the shape, never of the batch, so a 32-document batch changes no document.
        B = 32
        eng = Engine(G, B, H, device=dev)
        eng.bind_blob(blob288)
        cond = docs(B, G)
        x_T = torch.randn(B * H, 2, G, G, device=dev, generator=gen)
        src_u8 = torch.randint(0, 256, (B, FH, FW, 3), device=dev, dtype=torch.uint8, generator=gen)
        tab = schedule.Tables(schedule.named_betas("cosine", 50))

        def ns32():
            eng.prepare(*cond)
            flow = sampler.sample(eng, tab, x_T)
            return flow, ops.unwarp_u8_batch(flow, src_u8)
        dt, (flow, outs) = timed(ns32)
        ns32_s = dt
        del eng
        torch.cuda.empty_cache()
        eng1 = Engine(G, 1, H, device=dev)
        eng1.bind_blob(blob288)
        eng1.prepare(*[c[:1].contiguous() for c in cond])
        flow1 = sampler.sample(eng1, tab, x_T[:H].contiguous())
        same = bool(torch.equal(flow1[0], flow[0]))
        out["north_star_batch32"] = {"workload": f"north_star target point: batch={B} documents x {H} hypotheses, 50-step DDIM, 288x288 "
                                                 f"grid, + {FH}x{FW} u8 unwarp, 1 GPU", "batches_timed": 1,
                                     "ms_per_batch": round(dt * 1e3, 1), "value": round(B / dt, 5), "unit": "documents/s",
                                     "finite": bool(torch.isfinite(flow).all()),
                                     "parity": {"what": "document 0 of the 32-document batch == the same document sampled alone "
                                                        "(coordinate map, bit for bit)", "ok": same}}
        del eng1, cond, x_T, src_u8, outs, flow, flow1
        torch.cuda.empty_cache()

    if "cfg3" in legs:
        # ---- configs[3]: 250-step DDPM at the stated 32 documents (4 if the run is already long) ------------------------
        full_ok = ns32_s is not None and time.perf_counter() - _T_PROCESS_START + 5 * ns32_s < CFG3_FULL_DEADLINE_S
        B = 32 if full_ok else 4
        eng = Engine(G, B, H, device=dev)
        eng.bind_blob(blob288)
        cond = docs(B, G)
        noise_state = gen.get_state()            # the leg's x_T and noise table can be re-drawn (the single-document re-run below)
        x_T = torch.randn(B * H, 2, G, G, device=dev, generator=gen)
        tab = schedule.Tables(schedule.named_betas("cosine", 250))
        last = {}

        def noise_fn(i):
            z = torch.randn(B * H, 2, G, G, device=dev, generator=gen)
            if i == 125:
                last[i] = z
            return z

        def cfg3():
            eng.prepare(*cond)
            return sampler.sample(eng, tab, x_T, sampler="ddpm", noise_fn=noise_fn)
        dt, flow = timed(cfg3)
        # parity of the scheduler path this leg exercises: one ancestral step on the run's own tensors vs the oracle's formula
        par = None
        if want_cpu:
            from oracle import dvd_oracle as O
            i = 125
            x_t, x0 = x_T[:2].contiguous(), flow.repeat_interleave(H, 0)[:2].contiguous()
            nz = last[i][:2].contiguous()
            got = ops.sched_step(tab.ddpm_coef(i), x_t, x0, nz).cpu()
            ref = O.ddpm_step(O.Schedule(250), i, x_t.cpu(), x0.cpu(), nz.cpu())
            err = float((got - ref).abs().max())
            par = {"what": "fused DDPM step (t = 125, FIXED_LARGE) on this run's tensors vs the oracle's p_mean_variance + "
                           "noise line", "max_abs": err, "ok": bool(err < 1e-5)}
        # ... and of the whole 250-step chain: document 0 of the batch must have the bits it has when sampled ALONE with the same
        # x_T and the same noise table (re-drawn from the saved generator state; one engine of one document: ~1/32 of the leg)
        del eng
        torch.cuda.empty_cache()
        gen.set_state(noise_state)
        x_T1 = torch.randn(B * H, 2, G, G, device=dev, generator=gen)[:H].contiguous()
        eng1 = Engine(G, 1, H, device=dev)
        eng1.bind_blob(blob288)
        eng1.prepare(*[c[:1].contiguous() for c in cond])
        flow1 = sampler.sample(eng1, tab, x_T1, sampler="ddpm",
                               noise_fn=lambda i: torch.randn(B * H, 2, G, G, device=dev, generator=gen)[:H].contiguous())
        chain_same = bool(torch.equal(flow1[0], flow[0]))
        if par is None:
            par = {"what": "", "ok": True}
        par["what"] = (par["what"] + "; " if par["what"] else "") + \
            "document 0 of the batch after all 250 ancestral steps == the same document sampled alone (bit for bit)"
        par["chain_batch_equals_single"] = chain_same
        par["ok"] = bool(par["ok"] and chain_same)
        del eng1, flow1, x_T1
        out["configs[3]"] = {"workload": (f"BASELINE configs[3]: batch={B} documents x {H} hypotheses" if B == 32 else
                                          f"BASELINE configs[3] at batch={B} instead of 32 documents (x {H} hypotheses; the run "
                                          f"would have ended past {CFG3_FULL_DEADLINE_S} s with 32)") +
                                         ": 250-step DDPM ancestral sampling, 288x288 grid (no unwarp in this configuration)",
                             "batches_timed": 1, "ms_per_batch": round(dt * 1e3, 1), "value": round(B / dt, 5),
                             "unit": "documents/s", "finite": bool(torch.isfinite(flow).all()), "parity": par}
        del cond, x_T, flow, last
        torch.cuda.empty_cache()

    if "native" not in legs:
        return out
    # ---- the reference's native point, from a decoded image -------------------------------------------------------
    Gn, Sn = 64, 3
    sd = synth.synth_state_dict(Gn, seed=7, blocks=[11])
    eng = Engine(Gn, 1, H, device=dev)
    eng.load_state_dict(sd)
    tt = lambda d: {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}  # noqa: E731
    dewarp, seg, line = prestage.GeoTr_Seg_Inf(), prestage.Seg(), prestage.UNet(n_channels=3, n_classes=1)
    dewarp.msk.load_state_dict(tt(synth.synth_convnet_state_dict("u2netp", 11)), strict=True)
    seg.load_state_dict(tt(synth.synth_convnet_state_dict("u2netp", 22, prefix="msk.")), strict=True)
    line.load_state_dict(tt(synth.synth_convnet_state_dict("unet", 13)), strict=True)
    for m in (dewarp, seg, line):
        m.to(dev)
        m.eval()
    img = synth.smooth_image("bench/native", 1024, 768, seed=1234)
    img_u8 = torch.from_numpy(np.ascontiguousarray((img.transpose(1, 2, 0) * 255.0).astype(np.uint8))).to(dev)
    xT = torch.from_numpy(synth.synth_noise(0, H, Gn, 1234)).to(dev)
    tabn = schedule.Tables(schedule.named_betas("cosine", Sn))

    def native():
        y512, src = ops.ingest_u8(img_u8, swap_rb=False, out_size=512, want_rgb=True)
        c = prestage.conditioning(dewarp, seg, line, y512[None], Gn)
        eng.prepare(y512[None].contiguous(), c["mask_cat"].contiguous(), c["mask_y512"].contiguous(), c["line_msk"].contiguous())
        flow = sampler.sample(eng, tabn, xT)
        return y512, c, flow, ops.unwarp_u8_batch(flow, src[None])
    for _ in range(3):
        native()
    lat = []
    for _ in range(15):
        dt, (y512, c, flow, o8) = timed(native)
        lat.append(dt * 1e3)
    par = None
    if want_cpu:
        from oracle import dvd_oracle as O
        doc = {"y512": y512[None].cpu(), "mask_cat": c["mask_cat"].cpu(), "mask_y512": c["mask_y512"].cpu(),
               "line_msk": c["line_msk"].cpu()}
        with torch.no_grad():
            t0 = time.perf_counter()
            ref = O.Oracle(sd, Gn).sample_loop(O.Schedule(Sn), xT.cpu(), doc)
            cpu_s = time.perf_counter() - t0
        rm = float((flow.cpu() - ref).pow(2).mean().sqrt())
        par = {"what": "coordinate map of the 3-step loop (conditioning = the GPU pre-stage's own output) vs the CPU oracle",
               "coord_rmse": rm, "bar": 1e-3, "ok": bool(rm < 1e-3), "cpu_oracle_seconds_sampling_only": round(cpu_s, 2)}
    out["native_point"] = {"workload": f"reference-native: 1 document at a time, G=64, 3-step DDIM, {H} hypotheses, from a "
                                       "decoded 1024x768 image: ingest (parity with a real cv2.resize UNPINNED: no OpenCV offline) + U2NETP x2 + "
                                       "line UNet + sampling + u8 unwarp",
                           "documents_timed": len(lat), "ms_per_document_median": round(statistics.median(lat), 3),
                           "value": round(1e3 / statistics.median(lat), 2), "unit": "documents/s", "parity": par}
    # ---- the same operating point BATCHED (admin/local.py's per-document settings, `batch_docs` documents per engine
    # batch - what val_TDiff.run does): B distinct decoded images -> ingest each, ONE pass of the three pre-stage nets over
    # the batch, ONE engine batch (B x H samples), one batched unwarp.  Parity: every document of the batch must give the bits
    # it gives alone (no cross-document arithmetic), and document 0 is compared with the CPU oracle like the single leg.
    single_flow, single_img = flow.clone(), img_u8
    del eng
    for Bn in (32,):          # (round 6: the 8-document leg made room for north_star_batch32)
        imgs = [torch.roll(img_u8, shifts=(17 * d, 29 * d), dims=(0, 1)).contiguous() for d in range(Bn)]
        engb = Engine(Gn, Bn, H, device=dev)
        engb.load_state_dict(sd)
        xTb = torch.cat([torch.from_numpy(synth.synth_noise(d, H, Gn, 1234)).to(dev) for d in range(Bn)])

        def native_batch():
            ys, srcs = zip(*[ops.ingest_u8(im, swap_rb=False, out_size=512, want_rgb=True) for im in imgs])
            y = torch.stack(ys)
            c = prestage.conditioning(dewarp, seg, line, y, Gn)
            engb.prepare(y, c["mask_cat"].contiguous(), c["mask_y512"].contiguous(), c["line_msk"].contiguous())
            fl = sampler.sample(engb, tabn, xTb)
            return fl, ops.unwarp_u8_batch(fl, torch.stack(srcs))
        for _ in range(2):
            native_batch()
        lat = []
        for _ in range(7):
            dt, (flb, o8b) = timed(native_batch)
            lat.append(dt * 1e3)
        med = statistics.median(lat)
        same = bool(torch.equal(flb[0], single_flow[0]))          # document 0 is the single leg's document
        out[f"native_point_batch{Bn}"] = {
            "workload": f"reference-native settings (G=64, 3-step DDIM, {H} hypotheses), {Bn} documents per engine batch, from "
                        "decoded 1024x768 images: ingest + ONE batched pass of U2NETP x2 + line UNet + sampling + batched u8 unwarp",
            "batches_timed": len(lat), "ms_per_batch_median": round(med, 3), "ms_per_document": round(med / Bn, 3),
            "value": round(Bn * 1e3 / med, 1), "unit": "documents/s",
            "parity": {"what": "document 0 of the batch == the same document sampled alone (bit for bit; its map is the one "
                               "compared with the CPU oracle in native_point)", "ok": same}}
        del engb, xTb, imgs, flb, o8b
        torch.cuda.empty_cache()
    for k in out:
        p = out[k].get("parity")
        if p is not None and not p["ok"]:
            raise SystemExit(f"PARITY FAILURE in other_configs[{k}]: {p}")
    return out


def cpu_baseline(grid, hyp, steps, check=None):
    """Time the CPU oracle (kind 'port': a restatement pinned to the reference by the golden vectors) on a
    bounded sample: ONE denoiser evaluation for ONE sample (of hyp*steps per document) with the same hoisted
    algebra as the GPU engine, scaled linearly to documents/s.  The evaluation is run at the benchmark grid
    when the host can do it in well under a minute, otherwise at G=64 and scaled by the FLOP ratio."""
    from dvd_amd import synth
    from oracle import dvd_oracle as O
    # torch's intra-op pool stops scaling (and then collapses) long before a 256-thread host is full on these op sizes:
    # the thread count is the MEASURED knee of this host (one G=64 sample-step per candidate, best wins), not a fixed cap.
    # `cores` reports the threads used.
    # the CPUs this process may use (its affinity mask), and no more threads than OMP_NUM_THREADS asks for when it is set:
    # on a shared host the probes above that only oversubscribe the cores the job was given
    ncpu = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS") or 1 << 30))
    cores, knee = ncpu, None

    def time_one(g):
        sd = synth.synth_state_dict(g, seed=7, blocks=[11])
        orc = O.Oracle(sd, g)
        gen = torch.Generator().manual_seed(5)
        T = (g // 2) ** 2
        inv = {"feat": torch.rand(1, 256, g, g, generator=gen),
               "cond": torch.randn(1, T, 384, generator=gen), "msk6": torch.randn(1, T, 384, generator=gen),
               "line": torch.randn(1, T, 384, generator=gen)}
        x = torch.randn(1, 2, g, g, generator=gen)
        flow = torch.zeros(1, 2, g, g)
        t0 = time.perf_counter()
        with torch.no_grad():
            orc.forward(x, 666.7, inv, flow, inv["feat"])
        return time.perf_counter() - t0

    def time_and_check(g):
        """The timed evaluation doubles as a FULL-SIZE parity check: it is the first loop step of document 0 /
        hypothesis 0 of this very run (same synthetic weights, conditioning and x_T), compared with what the engine
        produced for that sample; a second (untimed) evaluation checks the warped-feature branch."""
        sd = synth.synth_state_dict(g, seed=7, blocks=[11])
        orc = O.Oracle(sd, g)
        res = []
        with torch.no_grad():
            inv = orc.prepare(*check["doc"])                      # once-per-document work: not part of the timed step
            dts = []
            t0 = time.perf_counter()
            x0_ref, _ = orc.forward(check["x"], check["t_model"], inv, torch.zeros_like(check["x"]), inv["feat"])
            dts.append(time.perf_counter() - t0)
            rmse = float((x0_ref - check["x0_gpu"]).pow(2).mean().sqrt())
            res.append({"what": f"x0 prediction of the first loop step (t_model = {check['t_model']:.1f}, init_feat = "
                                f"feat) of document 0 / hypothesis 0 at G={g}: HIP engine vs CPU oracle",
                        "coord_rmse": rmse, "bar": 1e-3, "ok": bool(rmse < 1e-3)})
            if "x0_gpu_warp" in check:
                flow = check["x0_gpu"]                            # the engine's own first-step x0 is the init_flow
                init_feat = O.grid_sample_ref(inv["feat"], (flow + O.base_grid(g, g)) * 2 - 1)
                t0 = time.perf_counter()
                x0w, _ = orc.forward(check["x"], check["t_model_warp"], inv, flow, init_feat)
                dts.append(time.perf_counter() - t0)
                rmse = float((x0w - check["x0_gpu_warp"]).pow(2).mean().sqrt())
                res.append({"what": f"x0 prediction on the warped-feature branch (feat_mode 2, t_model = "
                                    f"{check['t_model_warp']:.1f}, init_flow = first-step x0) at G={g}: HIP engine vs "
                                    "CPU oracle", "coord_rmse": rmse, "bar": 1e-3, "ok": bool(rmse < 1e-3)})
            if "x_h1" in check:
                t0 = time.perf_counter()
                x0h, _ = orc.forward(check["x_h1"], check["t_model"], inv, torch.zeros_like(check["x_h1"]), inv["feat"])
                dts.append(time.perf_counter() - t0)
                rmse = float((x0h - check["x0_gpu_h1"]).pow(2).mean().sqrt())
                res.append({"what": f"x0 prediction of the first loop step of document 0 / hypothesis 1 at G={g}: HIP engine "
                                    "vs CPU oracle", "coord_rmse": rmse, "bar": 1e-3, "ok": bool(rmse < 1e-3)})
        return dts, res

    def time_faithful(g=64):
        """What the reference EXECUTES per sample-step (all 12 blocks, pyramid + c/m/l embeddings every step):
        one sample-step at G=64, scaled by the faithful FLOP ratio to the benchmark grid (stated in `sample`)."""
        sd = synth.synth_state_dict(g, seed=7)
        orc = O.Oracle(sd, g, live_blocks_only=False)
        gen = torch.Generator().manual_seed(5)
        doc = [torch.rand(1, 3, 512, 512, generator=gen), torch.rand(1, 1, 512, 512, generator=gen),
               torch.randn(1, 384, g, g, generator=gen).clamp_min_(0), torch.randn(1, 64, g, g, generator=gen).clamp_min_(0)]
        x = torch.randn(1, 2, g, g, generator=gen)
        t0 = time.perf_counter()
        with torch.no_grad():
            inv = orc.prepare(*doc)                               # per-step in the reference: inside the timed region
            orc.forward(x, 666.7, inv, torch.zeros(1, 2, g, g), inv["feat"])
        return time.perf_counter() - t0

    # (candidates stop at 128: on a 256-thread host the 256-thread probe alone took 52 s for a 0.2 s step)
    cands = sorted({c for c in (8, 16, 32, 64, 128, min(ncpu, 128)) if c <= ncpu})
    knee = {}
    for c in cands:
        torch.set_num_threads(c)
        time_one(64) if c == cands[0] else None           # first call warms the allocator / weight generation caches
        knee[c] = round(time_one(64), 3)
    cores = min(knee, key=knee.get)
    torch.set_num_threads(cores)
    t64 = knee[cores]
    f64, _ = step_flops(64)
    fg, _ = step_flops(grid)
    est = t64 * fg / f64
    parity = None
    samples = None
    if grid != 64 and est < 120.0 and check is not None:
        samples, parity = time_and_check(grid)
        t_step = sorted(samples)[len(samples) // 2]
        sample = (f"median of {len(samples)} sample-steps at G={grid} (of {hyp * steps} per document), each 1 sample x 1 "
                  "denoiser evaluation of this very run (first loop step of document 0 for both hypotheses, one step on the "
                  "warped-feature branch), hoisted algebra")
    elif grid != 64 and est < 120.0:
        t_step, sample = time_one(grid), f"1 sample x 1 denoiser evaluation at G={grid} (of {hyp * steps} per document), hoisted algebra"
    else:
        t_step = est
        sample = (f"1 sample x 1 denoiser evaluation at G=64 ({t64:.2f} s), scaled by the FLOP ratio to G={grid} "
                  f"(of {hyp * steps} per document), hoisted algebra")
    docs_per_s = 1.0 / (hyp * steps * t_step)
    out = {"value": round(docs_per_s, 7), "unit": "documents/s", "cores": cores, "kind": "port", "sample": sample,
           "mode": "hoisted (the GPU engine's algebra: live block only, per-document invariants outside the step)",
           "seconds_per_sample_step": round(t_step, 3),
           "seconds_per_sample_step_samples": None if samples is None else [round(v, 2) for v in samples],
           "thread_knee_seconds_per_G64_step": knee}
    tf64 = sorted(time_faithful(64) for _ in range(3))[1]
    tf = tf64 * faithful_step_flops(grid) / faithful_step_flops(64)
    out["faithful"] = {"value": round(1.0 / (hyp * steps * tf), 8), "unit": "documents/s", "cores": cores,
                       "mode": "faithful (what the reference executes: 12 DiT blocks, conv pyramid and c/m/l "
                               "embeddings at every step; idf/cross_model.py:584-616)",
                       "sample": f"median of 3 x (1 sample x 1 denoiser evaluation at G=64) ({tf64:.2f} s, "
                                 f"{faithful_step_flops(64) / 1e9:.1f} GFLOP), scaled by the faithful FLOP ratio "
                                 f"{faithful_step_flops(grid) / faithful_step_flops(64):.1f} to G={grid}",
                       "seconds_per_sample_step": round(tf, 3)}
    if parity is not None:
        out["parity"] = parity
    return out


if __name__ == "__main__":
    main()
