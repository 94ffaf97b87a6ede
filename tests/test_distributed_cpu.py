"""Multi-process (gloo, world_size 2, CPU) test of the sampling path's distributed plumbing: rank-0 packs the
weight blob, ONE flat broadcast, both ranks hold identical bytes; documents shard disjointly with no collective."""
import hashlib
import os
import socket
import sys
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn_ranks(target, world, extra_args=(), timeout=240, attempts=2):
    """Start `world` rank processes of `target(rank, world, port, queue, *extra_args)` and collect one result per rank.
    A rendezvous hiccup (port grabbed between probe and bind, a slow spawn on a loaded machine) gets ONE clean retry on a
    fresh port; the ranks of a failed attempt are terminated by handle."""
    import queue as _queue
    last = None
    for _ in range(attempts):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=target, args=(r, world, port, q, *extra_args)) for r in range(world)]
        for p in procs:
            p.start()
        try:
            res = sorted(q.get(timeout=timeout) for _ in range(world))
            for p in procs:
                p.join(timeout=120)
            if all(p.exitcode == 0 for p in procs):
                return res
            last = AssertionError(f"rank exit codes {[p.exitcode for p in procs]}")
        except _queue.Empty as e:
            last = e
        for p in procs:
            if p.is_alive():
                p.terminate()
            p.join(timeout=30)
    raise AssertionError(f"ranks did not finish after {attempts} attempts: {last!r}")



def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from dvd_amd import dist_util, synth, weights
    dist_util.setup_dist(backend="gloo")
    assert dist_util.rank() == rank and dist_util.world_size() == world
    grid = 16
    # blob layout must be computable on every rank without the weights
    if rank == 0:
        packed = weights.pack(synth.synth_state_dict(grid, 7, blocks=[11]), grid)
        names = sorted(packed)
        blob = torch.cat([packed[n].contiguous().view(-1).view(torch.uint8) for n in names])
        size = torch.tensor([blob.numel()])
    else:
        size = torch.tensor([0])
    dist.broadcast(size, 0)
    if rank != 0:
        blob = torch.empty(int(size), dtype=torch.uint8)
    dist_util.broadcast_blob(blob, src=0)
    digest = hashlib.sha256(blob.numpy().tobytes()).hexdigest()
    docs = dist_util.shard_documents(7)
    dist.barrier()
    q.put((rank, digest, docs))
    dist.destroy_process_group()


def test_two_rank_broadcast_and_sharding():
    res = _spawn_ranks(_worker, 2)
    assert res[0][1] == res[1][1], "ranks disagree on the broadcast weight blob"
    assert res[0][2] == [0, 2, 4, 6] and res[1][2] == [1, 3, 5]


# ------------------------------------------------------------------------------------------------
# The product's own multi-rank path: val_TDiff.run(settings) under 2 gloo ranks, with the engine's
# COMPUTE entry points stubbed at the lib.call boundary (there is no GPU here; the host-only entry
# points - create / tensor_info / bind_workspace / set_tensor - run for real).
# ------------------------------------------------------------------------------------------------
COMPUTE = {"dvd_unwarp_grid", "dvd_grid_sample_bilinear_zeros_ac", "dvd_convnet_run", "dvd_resize_bilinear_nchw", "dvd_threshold_mask_mul", "dvd_threshold_mask_mul_batch", "dvd_ingest_u8",
           "dvd_unwarp_u8_batch", "dvd_engine_prepare_docs", "dvd_engine_denoise_step", "dvd_engine_feat_nchw", "dvd_sched_step",
           "dvd_hyp_mean_clamp", "dvd_unwarp_u8"}


def _stub_compute(calls):
    """Patch the GPU-only pieces; returns nothing, records (name) of every stubbed compute call."""
    import torch as th
    from dvd_amd import cross_model, engine, lib, ops, prestage, val_TDiff
    real_call = lib.call

    def call(name, *args):
        if name in COMPUTE:
            calls.append(name)
            return
        return real_call(name, *args)
    lib.call = call
    for mod in (engine, ops, prestage):
        mod.stream_ptr = lambda: None
    ops._chk = lambda *a, **k: None
    engine._is_dev = lambda t: True
    cross_model._require_gpu = lambda dev: None
    val_TDiff._require_gpu = lambda: None
    th.cuda.synchronize = lambda *a, **k: None


def _run_worker(rank, world, port, q, n_docs, tmp):
    sys.path.insert(0, ROOT)
    os.chdir(tmp)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    calls = []
    _stub_compute(calls)
    import admin.settings as ws
    from dvd_amd import dist_util, val_TDiff
    dist_util.setup_dist(backend="gloo")           # run() finds the group initialised and leaves it to us
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps, s.env.n_batch = 16, 3, 2
    s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res, s.env.visualize = n_docs, 2, (32, 24), False
    s.name, s.seed, s.severity, s.corruption_number = f"gloo{rank}", 0, 0, 0
    seen = {}
    orig = val_TDiff.run_evaluation_docunet

    def spy(settings, logger, val_loader, diffusion, model, dewarp, line=None, seg=None):
        h = hashlib.sha256(model._blob.cpu().numpy().tobytes())
        for m in (dewarp, seg, line):                  # denoiser + pre-stage nets travel in the one flat broadcast
            h.update((m.msk if hasattr(m, "msk") else m)._blob.cpu().numpy().tobytes())
        seen["digest"] = h.hexdigest()
        return orig(settings, logger, val_loader, diffusion, model, dewarp, line, seg)
    val_TDiff.run_evaluation_docunet = spy
    results = val_TDiff.run(s)
    q.put((rank, seen["digest"], [p for p, _ in results], calls.count("dvd_engine_denoise_step"),
           calls.count("dvd_engine_prepare_docs"), calls.count("dvd_unwarp_u8_batch"), calls.count("dvd_convnet_run"),
           calls.count("dvd_ingest_u8")))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_docs", [1, 5])
def test_val_tdiff_run_two_ranks(tmp_path, n_docs):
    """n_docs = 1 < world: rank 1 owns NO document - it must still take part in the one weight broadcast (issued
    eagerly by run(), never lazily by engine()) and reach the final barrier (this used to hang).
    n_docs = 5: disjoint shards [0,2,4] / [1,3], batches of 2, 3 DDIM steps per batch."""
    res = _spawn_ranks(_run_worker, 2, (n_docs, str(tmp_path)))
    (r0, d0, docs0, den0, prep0, unw0, cn0, ing0), (r1, d1, docs1, den1, prep1, unw1, cn1, ing1) = res
    assert d0 == d1, "ranks disagree on the broadcast weight blob"
    want0 = [f"synthetic_{i:05d}" for i in range(0, n_docs, 2)]
    want1 = [f"synthetic_{i:05d}" for i in range(1, n_docs, 2)]
    assert docs0 == want0 and docs1 == want1
    for docs, den, prep, unw, cn, ing in ((want0, den0, prep0, unw0, cn0, ing0), (want1, den1, prep1, unw1, cn1, ing1)):
        batches = (len(docs) + 1) // 2
        assert den == 3 * batches and prep == batches and unw == batches      # one batched unwarp launch per batch
        assert ing == len(docs) and cn == 3 * batches      # ingest once per document; each of the three pre-stage nets
                                                           # runs its op list ONCE per batch of documents (round 3)


def _missing_ckpt_worker(rank, world, port, q, tmp):
    sys.path.insert(0, ROOT)
    os.chdir(tmp)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    calls = []
    _stub_compute(calls)
    import admin.settings as ws
    from dvd_amd import dist_util, val_TDiff
    dist_util.setup_dist(backend="gloo")
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps, s.env.n_batch = 16, 3, 2
    s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res, s.env.visualize = 2, 2, (32, 24), False
    s.env.synthetic_weights_if_missing = False          # no checkpoint file here: rank 0 (the only reader) must fail ...
    s.name, s.seed, s.severity, s.corruption_number = f"gloo_missing{rank}", 0, 0, 0
    try:
        val_TDiff.run(s)
        outcome = "returned"
    except FileNotFoundError:
        outcome = "FileNotFoundError"
    except RuntimeError as e:                           # ... and every OTHER rank must raise too, not wait in the broadcast
        outcome = "RuntimeError" if "another rank" in str(e) else f"unexpected RuntimeError: {e}"
    q.put((rank, outcome, calls.count("dvd_engine_denoise_step")))
    dist.barrier()
    dist.destroy_process_group()


def test_missing_checkpoint_fails_on_every_rank(tmp_path):
    """Only rank 0 reads checkpoint files.  When it cannot, the other ranks used to sit in the weight broadcast until the
    launcher killed them (round-2 ADVICE); now a 4-byte all-reduce in front of the broadcast makes every rank raise."""
    res = _spawn_ranks(_missing_ckpt_worker, 2, (str(tmp_path),))
    assert res[0][1] == "FileNotFoundError" and res[1][1] == "RuntimeError", res
    assert res[0][2] == res[1][2] == 0


# ------------------------------------------------------------------------------------------------
# bench.py's rank logic (the functions its N > 1 branch is made of) under 2 gloo ranks
# ------------------------------------------------------------------------------------------------
def _bench_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from dvd_amd import engine, synth
    bench.init_dist(world, rank, backend="gloo")
    grid = 16
    _, nbytes = engine.blob_layout(grid)
    blob = engine.pack_blob(synth.synth_state_dict(grid, seed=7, blocks=[11]), grid) if rank == 0 \
        else torch.empty(nbytes, dtype=torch.uint8)
    ms = bench.broadcast_weights(blob, world)
    slowest = bench.max_over_ranks(1.0 + rank, world, torch.device("cpu"))
    q.put((rank, hashlib.sha256(blob.numpy().tobytes()).hexdigest(), ms is not None and ms >= 0.0, slowest))
    dist.barrier()
    dist.destroy_process_group()


def test_bench_rank_logic_two_ranks():
    res = _spawn_ranks(_bench_worker, 2)
    assert res[0][1] == res[1][1] and res[0][2] and res[1][2]
    assert res[0][3] == res[1][3] == 2.0          # every rank reports the slowest rank's time


# ------------------------------------------------------------------------------------------------
# bench.py's main() itself, N = 2: the whole N > 1 branch (rank-0 pack, one broadcast, per-rank synthetic documents, timed
# region bracketed by barriers, max over ranks, rank 0 prints the one JSON line) with the device stubbed to the CPU and
# the compute entry points stubbed at the lib.call boundary.
# ------------------------------------------------------------------------------------------------
class _FakeEvent:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass

    def elapsed_time(self, other):
        return 1.0


def _count_collectives(log, marks):
    """Wrap every torch.distributed collective bench.py could issue: log (name, payload bytes).  `marks` are appended to the same
    log by the stubbed compute calls, so the log shows what ran BETWEEN the two barriers of the timed region."""
    def wrap(name, nbytes):
        real = getattr(dist, name)

        def f(*a, **k):
            log.append((name, nbytes(*a, **k)))
            return real(*a, **k)
        setattr(dist, name, f)
    tb = lambda t, *a, **k: t.numel() * t.element_size()  # noqa: E731
    wrap("broadcast", tb)
    wrap("all_reduce", tb)
    wrap("all_gather", lambda out, t, *a, **k: t.numel() * t.element_size())
    wrap("all_gather_object", lambda *a, **k: -1)
    wrap("barrier", lambda *a, **k: 0)
    for name in ("reduce", "gather", "scatter", "reduce_scatter", "all_to_all", "all_to_all_single", "send", "recv", "isend", "irecv",
                 "broadcast_object_list", "all_gather_into_tensor", "reduce_scatter_tensor"):
        if hasattr(dist, name):
            wrap(name, lambda *a, **k: -2)


def _bench_main_worker(rank, world, port, q, tmp):
    sys.path.insert(0, ROOT)
    os.chdir(tmp)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import io
    import contextlib
    import importlib.util
    calls = []
    _stub_compute(calls)
    _count_collectives(calls, None)            # collectives and stubbed compute calls in ONE log, in program order
    import torch as th
    from dvd_amd import engine as eng_mod
    real_device = th.device
    th.cuda.set_device = lambda *a, **k: None
    th.cuda.Event = _FakeEvent
    th.device = lambda *a, **k: real_device("cpu") if (a and a[0] == "cuda") else real_device(*a, **k)
    eng_mod.Engine.profile = lambda self, on: None
    eng_mod.Engine.profile_read = lambda self: (0, 0.0)
    from dvd_amd import ops as ops_mod         # the stubbed kernels write nothing: give bench's finiteness check defined zeros
    ops_mod.hyp_mean_clamp = lambda x0, n_hyp: th.zeros(x0.shape[0] // n_hyp, 2, x0.shape[2], x0.shape[3])
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        try:
            bench.main(["--gpus", str(world), "--steps", "2", "--warmup", "1", "--grid", "16", "--docs", "3", "--ddim-steps", "3",
                        "--full-res", "32x24", "--no-cpu-baseline", "--backend", "gloo"])
        except AssertionError as e:          # the stubbed engine writes nothing: bench's own finiteness check may fire
            if "non-finite" not in str(e):
                raise
    q.put((rank, out.getvalue(), calls.count("dvd_engine_denoise_step"), calls.count("dvd_engine_prepare_docs"),
           [c for c in calls if isinstance(c, tuple)],
           # the log between the two barriers that bracket the timed region (the 2nd and 3rd barrier of the run)
           _between_timing_barriers(calls)))


def _between_timing_barriers(calls):
    idx = [i for i, c in enumerate(calls) if c == ("barrier", 0)]
    return calls[idx[1] + 1:idx[2]] if len(idx) >= 3 else None


def test_bench_main_eight_ranks(tmp_path):
    """Round 6: no 8-GPU node has ever been available, so the first real SCALE run must be boring - the
    WHOLE `bench.py --gpus 8` branch under 8 gloo ranks (BASELINE configs[2]'s world size): exactly ONE broadcast, of the packed
    weight blob's byte count; NO collective of any kind between the two barriers of the timed region (only engine launches); the
    same number of evaluations on every rank; the line carries the broadcast's time and bytes and every rank's own
    documents/s."""
    import json
    res = _spawn_ranks(_bench_main_worker, 8, (str(tmp_path),), timeout=600)
    assert [r[0] for r in res] == list(range(8))
    line = json.loads([ln for ln in res[0][1].splitlines() if ln.startswith("{")][-1])
    for rank, out, den, prep, coll, timed in res:
        assert den == 3 * 3 and prep == 3, (rank, den, prep)
        assert rank == 0 or out.strip() == ""
        names = [c[0] for c in coll]
        assert names == ["all_gather_object", "barrier", "broadcast", "barrier", "barrier", "all_reduce", "all_gather", "barrier"], (rank, names)
        (bcast,) = [c for c in coll if c[0] == "broadcast"]
        assert bcast[1] == line["weight_broadcast_bytes"] > 1_000_000, (rank, bcast)
        assert timed is not None and not [c for c in timed if isinstance(c, tuple)], (rank, timed)      # zero collectives inside
        assert timed.count("dvd_engine_denoise_step") == 2 * 3 and timed.count("dvd_unwarp_u8_batch") == 2
    assert line["n_gpus"] == 8 and line["scaling"] == "weak" and line["config"]["parallelism"].startswith("dp8")
    assert line["weight_broadcast_ms"] is not None and line["collectives"]["data_path"] == 0
    assert [p["rank"] for p in line["per_rank"]] == list(range(8)) and all(p["documents_per_s"] > 0 for p in line["per_rank"])
    assert len(line["ranks_seen"]["ranks"]) == 8
    assert abs(line["value"] - 8 * 3 * 2 / (line["ms_per_step"] * 2 / 1e3)) < 0.05 * line["value"]
    slowest = max(p["seconds"] for p in line["per_rank"])
    assert abs(slowest - line["ms_per_step"] * 2 / 1e3) < 0.05 * slowest + 1e-3      # the value uses the MAX over ranks


def test_bench_main_two_ranks(tmp_path):
    import json
    res = _spawn_ranks(_bench_main_worker, 2, (str(tmp_path),))
    (r0, out0, den0, prep0, _, _), (r1, out1, den1, prep1, _, _) = res
    assert den0 == den1 == 3 * 3 and prep0 == prep1 == 3        # (1 warm-up + 2 timed) x 3 DDIM steps on EVERY rank
    assert out1.strip() == ""                                     # only rank 0 prints
    lines = [ln for ln in out0.splitlines() if ln.startswith("{")]
    if lines:                                                    # (absent only if the stub's uninitialised output was non-finite)
        line = json.loads(lines[-1])
        assert line["n_gpus"] == 2 and line["steps"] == 2 and line["warmup"] == 1 and line["scaling"] == "weak"
        assert line["config"]["docs_per_gpu"] == 3 and line["config"]["parallelism"].startswith("dp2")
        assert line["weight_broadcast_ms"] is not None
        # whole-job value = documents of ALL ranks / max-over-ranks time (both fields are rounded: loose tolerance)
        assert abs(line["value"] - 2 * 3 * 2 / (line["ms_per_step"] * 2 / 1e3)) < 0.05 * line["value"]


# ------------------------------------------------------------------------------------------------
# `python bench.py --gpus 2` typed WITHOUT a launcher (how the driver types it): bench.py must start its own rank
# processes, relay rank 0's one JSON line and exit 0.  The ranks are fresh interpreters, so the CPU stubs of the compute
# entry points are installed through a `sitecustomize` module on PYTHONPATH (bench.py itself knows nothing about it).
# ------------------------------------------------------------------------------------------------
_SITECUSTOMIZE = '''
import os, sys
if os.environ.get("DVD_TEST_STUB_BENCH") == "1" and "RANK" in os.environ:
    sys.path.insert(0, os.environ["DVD_TEST_ROOT"])
    import torch as th
    from tests.test_distributed_cpu import _stub_compute, _FakeEvent
    from dvd_amd import engine as eng_mod
    _stub_compute([])
    _real_device = th.device
    th.cuda.set_device = lambda *a, **k: None
    th.cuda.Event = _FakeEvent
    th.device = lambda *a, **k: _real_device("cpu") if (a and a[0] == "cuda") else _real_device(*a, **k)
    _zeros = th.zeros
    th.empty = lambda *a, **k: _zeros(*a, **k)          # the stubbed engine writes nothing: keep its outputs finite
    eng_mod.Engine.profile = lambda self, on: None
    eng_mod.Engine.profile_read = lambda self: (0, 0.0)
'''


def test_bench_launches_its_own_ranks(tmp_path):
    import json
    import subprocess
    (tmp_path / "sitecustomize.py").write_text(_SITECUSTOMIZE)
    env = dict(os.environ, DVD_TEST_STUB_BENCH="1", DVD_TEST_ROOT=ROOT,
               PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--grid", "16",
           "--docs", "3", "--ddim-steps", "3", "--full-res", "32x24", "--no-cpu-baseline", "--backend", "gloo"]
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]                    # ONE line, from rank 0
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert line["weight_broadcast_ms"] is not None
    assert [r["rank"] for r in line["ranks_seen"]["ranks"]] == [0, 1]
    assert line["config"]["parallelism"].startswith("dp2")


@pytest.mark.parametrize("full", [False, True])
def test_bench_single_rank_plain_full_and_dump(tmp_path, full):
    """`bench.py --gpus 1`: a plain run reports the headline and leaves the extras null; --full measures roofline_unwarp;
    --dump-outputs writes the last timed step's outputs as float32 .npy in their own shapes (small enough to be whole)."""
    import json
    import subprocess
    import numpy as np
    (tmp_path / "sitecustomize.py").write_text(_SITECUSTOMIZE)
    env = dict(os.environ, DVD_TEST_STUB_BENCH="1", DVD_TEST_ROOT=ROOT, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--grid", "16",
           "--docs", "3", "--ddim-steps", "3", "--full-res", "32x24", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd + (["--full"] if full else []), env=env, cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "documents/s" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["cpu_baseline"] is None and line["other_configs"] is None
    assert (line["roofline_unwarp"] is not None) == full
    shapes = {"flow": (3, 2, 16, 16), "unwarped_u8": (3, 32, 24, 3)}
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{n}.npy" for n in shapes)
    for name, shape in shapes.items():
        a = np.load(tmp_path / "out" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape, (name, a.dtype, a.shape)


def test_bench_dump_sample_is_seeded_and_bounded():
    """An output larger than the dump limit is written as the same seeded sample of its values in every run."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    a, b = bench._dump_sample(t, limit=300), bench._dump_sample(t.clone(), limit=300)
    assert a.dtype == "float32" and a.shape == (300,) and (a == b).all()
    assert (a[1:] >= a[:-1]).all() and a.max() < 5000
    assert bench._dump_sample(t, limit=5000).shape == (5000,)


def test_bench_launcher_propagates_a_rank_failure(tmp_path):
    """A rank that dies must end the job with a non-zero exit code instead of leaving the others in a collective."""
    import subprocess
    (tmp_path / "sitecustomize.py").write_text(
        _SITECUSTOMIZE + 'if os.environ.get("RANK") == "1" and os.environ.get("DVD_TEST_STUB_BENCH") == "1":\n    raise SystemExit(7)\n')
    env = dict(os.environ, DVD_TEST_STUB_BENCH="1", DVD_TEST_ROOT=ROOT,
               PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--grid", "16", "--docs", "2",
           "--ddim-steps", "3", "--full-res", "32x24", "--no-cpu-baseline", "--backend", "gloo"]
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode != 0


def test_bench_launcher_ends_a_hung_rank(tmp_path, monkeypatch):
    """a rank that hangs without dying - and ignores SIGTERM, like one stuck in a GPU collective - must not block
    the parent for ever: past the overall deadline the ranks are terminated, then killed, and the launcher returns a positive
    exit code (signal exits are reported as 128 + signal)."""
    import importlib.util
    (tmp_path / "sitecustomize.py").write_text(
        'import os, signal, time\n'
        'if os.environ.get("DVD_TEST_HANG") == "1" and "RANK" in os.environ:\n'
        '    signal.signal(signal.SIGTERM, signal.SIG_IGN)\n'
        '    time.sleep(600)\n')
    monkeypatch.setenv("DVD_TEST_HANG", "1")
    monkeypatch.setenv("PYTHONPATH", os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    spec = importlib.util.spec_from_file_location("bench_launcher", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t0 = time.monotonic()
    rc = bench.launch_ranks(2, ["--gpus", "2", "--steps", "1"], deadline_s=3.0)
    dt = time.monotonic() - t0
    assert rc > 0 and rc in (124, 128 + 9, 128 + 15), rc
    assert dt < 60, dt


def test_bench_launcher_retries_only_the_rendezvous_race(tmp_path, monkeypatch):
    """the retry must fire for the port race it exists for - rank 0 ALONE dies at once (EADDRINUSE), the others sit
    in the store's connect - and must NOT re-run a job whose ranks all fail by themselves (a bad argument would be printed three
    times).  Fake ranks: on the first attempt rank 0 exits 98 at once while rank 1 waits; on the second attempt (a marker file
    exists) both exit 0.  Then: every rank exits 5 at once -> reported after ONE attempt."""
    import importlib.util
    (tmp_path / "sitecustomize.py").write_text(
        'import os, sys, time\n'
        'mode = os.environ.get("DVD_TEST_RACE")\n'
        'if mode and "RANK" in os.environ:\n'
        '    mark = os.path.join(os.environ["DVD_TEST_DIR"], "attempts_" + os.environ["RANK"])\n'
        '    n = len(open(mark).read()) if os.path.exists(mark) else 0\n'
        '    open(mark, "a").write("x")\n'
        '    if mode == "race":\n'
        '        if n == 0 and os.environ["RANK"] == "0": os._exit(98)\n'
        '        if n == 0: time.sleep(300)\n'
        '        os._exit(0)\n'
        '    os._exit(5)\n')
    monkeypatch.setenv("PYTHONPATH", os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    monkeypatch.setenv("DVD_TEST_DIR", str(tmp_path))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    spec = importlib.util.spec_from_file_location("bench_launcher2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setenv("DVD_TEST_RACE", "race")
    t0 = time.monotonic()
    assert bench.launch_ranks(2, ["--gpus", "2"]) == 0
    assert time.monotonic() - t0 < 40                                         # the short grace, not the 20 s one
    assert (tmp_path / "attempts_0").read_text() == "xx" and (tmp_path / "attempts_1").read_text() == "xx"
    for f in ("attempts_0", "attempts_1"):
        (tmp_path / f).unlink()
    monkeypatch.setenv("DVD_TEST_RACE", "all_fail")
    assert bench.launch_ranks(2, ["--gpus", "2"]) == 5
    assert (tmp_path / "attempts_0").read_text() == "x"                        # ONE attempt
