"""GPU tests of the ragged batch: documents of DIFFERENT sizes through one launch per stage (ops.unwarp_u8_ragged,
ops.ingest_u8_ragged, and run_evaluation_docunet on a mixed-size batch).  The yardstick is bit-equality with the
single-document entry points ops.unwarp_u8 / ops.ingest_u8 (pinned to golden G5 and to oracle/ingest_oracle.py by
tests/test_gpu_ops.py): torch.equal on whole buffers, no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from dvd_amd import lib, ops, synth

pytestmark = pytest.mark.gpu

# each shape is the smallest that reaches one branch of the tail: 3hw < 12 (scalar path); exactly 12 bytes (fast path,
# last_base = 0); w = 1 (sx = 0); w % 4 != 0; two 256-column blocks x two 4-row blocks, ragged in both; two plain ones
TAIL_SHAPES = [(1, 3), (1, 4), (5, 1), (7, 6), (6, 260), (37, 64), (64, 64)]
INGEST_SHAPES = [(32, 32), (1, 1), (16, 16), (9, 40), (50, 33)]     # exactly 2x of 16; 1 px; identity; up / down; odd


def _images(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).cuda() for h, w in shapes]


@pytest.fixture(scope="module", params=[8, 16])
def tail_case(request):
    """flow = 0.1 * randn (taps inside and across the border), the sources, and each document's bytes from ops.unwarp_u8
    alone - computed once per G and shared."""
    g = request.param
    gen = torch.Generator().manual_seed(100 + g)
    flow = (0.1 * torch.randn(len(TAIL_SHAPES), 2, g, g, generator=gen)).cuda()
    srcs = _images(TAIL_SHAPES, 200 + g)
    want = [ops.unwarp_u8(flow[d:d + 1].contiguous(), s) for d, s in enumerate(srcs)]
    return flow, srcs, want


def test_ragged_tail_equals_single_document_calls(tail_case):
    flow, srcs, want = tail_case
    got = ops.unwarp_u8_ragged(flow, srcs)
    assert len(got) == len(srcs)
    for d, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == torch.uint8 and a.shape == srcs[d].shape and torch.equal(a, b), TAIL_SHAPES[d]


def test_ragged_tail_reversed_order_and_single(tail_case):
    flow, srcs, want = tail_case
    got = ops.unwarp_u8_ragged(flow.flip(0).contiguous(), srcs[::-1])
    for d, (a, b) in enumerate(zip(got, want[::-1])):
        assert torch.equal(a, b), TAIL_SHAPES[::-1][d]
    for d in range(len(srcs)):                                   # n = 1: every shape alone through the ragged kernel
        (a,) = ops.unwarp_u8_ragged(flow[d:d + 1].contiguous(), [srcs[d]])
        assert torch.equal(a, want[d]), TAIL_SHAPES[d]
    assert ops.unwarp_u8_ragged(flow[:0].contiguous(), []) == []


def test_ragged_tail_chunks_above_the_cap(tail_case):
    """n = cap + 1 documents: the entry point cuts the batch into two launches; the second starts at flow[cap]."""
    flow, srcs, _ = tail_case
    assert lib.RAGGED_CAP < 2 ** 10
    n, g = lib.RAGGED_CAP + 1, flow.shape[-1]
    gen = torch.Generator().manual_seed(7)
    fl = (0.1 * torch.randn(n, 2, g, g, generator=gen)).cuda()
    docs = [srcs[3] if d % 2 == 0 else srcs[1] for d in range(n)]          # (7, 6) and (1, 4) alternating
    got = ops.unwarp_u8_ragged(fl, docs)
    for d in range(n):
        assert torch.equal(got[d], ops.unwarp_u8(fl[d:d + 1].contiguous(), docs[d])), d


def test_ragged_tail_stays_inside_each_document(tail_case):
    """Every src and out carved from ONE buffer filled with 0xA5, 16 bytes between neighbours: after the call the gaps (and
    the sources) are untouched, and the outputs equal the single-document results - which a read of a neighbour's bytes
    through a 12-byte access would change."""
    flow, srcs, want = tail_case
    sizes = [s.numel() for s in srcs]
    total = 16 + sum(sz + 16 for sz in sizes) * 2
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    spans, off = [], 16
    for sz in sizes * 2:                                         # all sources, then all outputs
        spans.append((off, off + sz))
        off += sz + 16
    assert off == total
    n = len(srcs)
    for (a, b), s in zip(spans[:n], srcs):
        buf[a:b] = s.reshape(-1)
    before = buf.clone()
    tab = (lib.RaggedImage * n)()
    for d in range(n):
        tab[d].src, tab[d].out = buf.data_ptr() + spans[d][0], buf.data_ptr() + spans[n + d][0]
        tab[d].h, tab[d].w = TAIL_SHAPES[d]
    lib.call("dvd_unwarp_u8_ragged", lib.ptr(flow), flow.shape[-1], tab, n, C.c_float(0.987), lib.stream_ptr())
    torch.cuda.synchronize()
    keep = torch.ones(total, dtype=torch.bool, device="cuda")
    for d in range(n):
        a, b = spans[n + d]
        keep[a:b] = False
        assert torch.equal(buf[a:b].view(srcs[d].shape), want[d]), TAIL_SHAPES[d]
    assert torch.equal(buf[keep], before[keep])                  # gaps still 0xA5, sources unchanged


@pytest.fixture(scope="module")
def ingest_case():
    imgs = _images(INGEST_SHAPES, 300)
    want = {swap: [ops.ingest_u8(im, swap_rb=swap, out_size=16, want_rgb=True) for im in imgs] for swap in (False, True)}
    return imgs, want


@pytest.mark.parametrize("want_rgb", [False, True])
@pytest.mark.parametrize("swap_rb", [False, True])
def test_ragged_ingest_equals_single_image_calls(ingest_case, swap_rb, want_rgb):
    imgs, want = ingest_case
    keep = [im.clone() for im in imgs]
    got = ops.ingest_u8_ragged(imgs, swap_rb=swap_rb, out_size=16, want_rgb=want_rgb)
    y, rgbs = got if want_rgb else (got, None)
    assert y.shape == (len(imgs), 3, 16, 16) and y.dtype == torch.float32
    for d, (wy, wrgb) in enumerate(want[swap_rb]):
        assert torch.equal(y[d], wy), INGEST_SHAPES[d]
        assert torch.equal(imgs[d], keep[d])
        if want_rgb:
            assert rgbs[d].shape == imgs[d].shape and torch.equal(rgbs[d], wrgb), INGEST_SHAPES[d]
    (y1,) = ops.ingest_u8_ragged(imgs[3:4], swap_rb=swap_rb, out_size=16)          # n = 1
    assert torch.equal(y1, want[swap_rb][3][0])


def test_ragged_ingest_copies_rgb_when_asked_through_the_c_abi(ingest_case):
    """swap_rb = 0 with an `out` of its own is a plain copy; out == src copies nothing; a null out is skipped."""
    imgs, want = ingest_case
    n = len(imgs)
    outs = [torch.zeros_like(im) for im in imgs]
    tab = (lib.RaggedImage * n)()
    for d, im in enumerate(imgs):
        tab[d].src, tab[d].h, tab[d].w = im.data_ptr(), im.shape[0], im.shape[1]
        tab[d].out = (outs[d].data_ptr(), im.data_ptr(), None)[d % 3]
    y = torch.empty(n, 3, 16, 16, device="cuda")
    scratch = torch.empty(lib.raw().dvd_ingest_ragged_scratch_bytes(16, n), dtype=torch.uint8, device="cuda")
    lib.call("dvd_ingest_u8_ragged", tab, n, 0, lib.ptr(y), 16, lib.ptr(scratch), lib.stream_ptr())
    for d, im in enumerate(imgs):
        assert torch.equal(y[d], want[False][d][0])
        assert torch.equal(outs[d], im if d % 3 == 0 else torch.zeros_like(im)), d


def test_ragged_ingest_at_the_product_size():
    imgs = _images([(600, 450), (1024, 1024)], 400)             # general resize; the exactly-2x INTER_AREA switch at 512
    y, rgbs = ops.ingest_u8_ragged(imgs, swap_rb=True, out_size=512, want_rgb=True)
    for d, im in enumerate(imgs):
        wy, wrgb = ops.ingest_u8(im, swap_rb=True, out_size=512, want_rgb=True)
        assert torch.equal(y[d], wy) and torch.equal(rgbs[d], wrgb), d


def test_ragged_ops_refuse_host_and_strided_tensors():
    flow = torch.zeros(1, 2, 8, 8, device="cuda")
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    for bad in (img.cpu(), img.float(), img.transpose(0, 1)):
        with pytest.raises(lib.DvdError):
            ops.unwarp_u8_ragged(flow, [bad])
        with pytest.raises(lib.DvdError):
            ops.ingest_u8_ragged([img, bad], out_size=16)


# ---------------------------------------------------------------------------------------------------------------------
# through the public surface
# ---------------------------------------------------------------------------------------------------------------------
def _build(grid, steps):
    import admin.settings as ws
    from dvd_amd.script_util import args_to_dict, create_model_and_diffusion, model_and_diffusion_defaults
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps = grid, steps
    s.name = "pytest_ragged"
    model, diffusion = create_model_and_diffusion(device="cuda", train_mode=s.env.train_mode, tv=s.env.time_variant,
                                                  grid_size=grid, **args_to_dict(s, model_and_diffusion_defaults().keys()))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(grid, 7).items()}
    model.cpu().load_state_dict(sd, strict=False)
    model.to("cuda")
    model.eval()
    return s, model, diffusion


class _Noise:
    """Answers the sampler's two torch.randn draws per batch (gaussian_diffusion.py: a discarded draw, then x_T for
    B * n_batch samples) so that document j gets rows [j * n_batch, (j + 1) * n_batch) of ONE fixed bank whatever batch it
    is sampled in: the batched and the one-by-one runs then start from the same noise."""

    def __init__(self, docs, n_batch, grid):
        gen = torch.Generator().manual_seed(11)
        self.bank = torch.randn(docs * n_batch, 2, grid, grid, generator=gen).cuda()
        self.n_batch, self.first_doc, self.draws, self.real = n_batch, 0, 0, torch.randn

    def __call__(self, *shape, **kw):
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        self.draws += 1
        if self.draws % 2 == 1:
            return self.real(*shape, **kw)
        lo = self.first_doc * self.n_batch
        assert shape[1:] == tuple(self.bank.shape[1:]) and lo + shape[0] <= self.bank.shape[0]
        return self.bank[lo:lo + shape[0]].clone()


def _evaluate(monkeypatch, tmp_path, make_docs):
    """run_evaluation_docunet on make_docs() with batch_docs = 3 and then one document at a time; returns both result
    lists and the number of per-document ops.unwarp_u8 / ops.ingest_u8 calls the batched run made."""
    import dvd_amd.gaussian_diffusion as gd
    from dvd_amd import logger
    from train_settings.dvd.evaluation import run_evaluation_docunet
    monkeypatch.chdir(tmp_path)
    grid = 16
    s, model, diffusion = _build(grid, 3)
    s.env.visualize, s.env.eval_dataset_name = False, "docunet"
    calls = {"unwarp_u8": 0, "ingest_u8": 0}
    for name in calls:
        def counted(*a, _real=getattr(ops, name), _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    noise = _Noise(3, s.env.n_batch, grid)
    monkeypatch.setattr(gd.th, "randn", noise)
    s.env.batch_docs = 3
    batched = run_evaluation_docunet(s, logger, make_docs(), diffusion, model, None, None, None)
    in_batch = dict(calls)
    s.env.batch_docs = 1
    single = []
    for j, d in enumerate(make_docs()):
        noise.first_doc = j
        single += run_evaluation_docunet(s, logger, [d], diffusion, model, None, None, None)
    return batched, single, in_batch


def _conditioning(i, grid=16):
    doc = synth.synth_document(i, grid, 1234)
    return {k: doc[k] for k in ("mask_cat", "mask_y512", "line_msk")}


def test_run_evaluation_docunet_on_a_mixed_size_batch(tmp_path, monkeypatch):
    """Three image_u8 documents of three sizes, batch_docs = 3: one ragged ingest and one ragged tail (no per-document
    ops.ingest_u8 / ops.unwarp_u8 call), and the same bytes, order and paths as three batch_docs = 1 runs."""
    shapes = [(96, 64), (64, 96), (70, 50)]
    arrays = [np.ascontiguousarray((synth.smooth_image(f"ragged{i}/image", h, w, seed=1234).transpose(1, 2, 0) * 255.0)
                                   .astype(np.uint8)) for i, (h, w) in enumerate(shapes)]

    def make_docs():
        return [dict(_conditioning(i), image_u8=a, path=f"doc_{i}") for i, a in enumerate(arrays)]
    batched, single, in_batch = _evaluate(monkeypatch, tmp_path, make_docs)
    assert in_batch == {"unwarp_u8": 0, "ingest_u8": 0}
    assert [p for p, _ in batched] == [p for p, _ in single] == ["doc_0", "doc_1", "doc_2"]
    for (_, a), (_, b), shp in zip(batched, single, shapes):
        assert a.dtype == torch.uint8 and tuple(a.shape) == shp + (3,) and torch.equal(a, b), shp
    assert not torch.equal(batched[0][1], torch.from_numpy(arrays[0]).cuda())      # the flow did move pixels


def test_run_evaluation_docunet_mixed_batch_with_a_float_source(tmp_path, monkeypatch):
    """A document on the f32 fallback (a float source that is not a byte image) stays on its own; the u8 rest of the batch
    still goes through the ragged tail with its own rows of the flow."""
    shapes = [(40, 24), (33, 20), (24, 40)]
    gen = torch.Generator().manual_seed(5)
    docs = []
    for i, (h, w) in enumerate(shapes):
        d = dict(synth.synth_document(i, 16, 1234), path=f"doc_{i}")
        u8 = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8)
        if i == 1:
            d["source_vis"] = u8.permute(2, 0, 1).float() + 0.25
        else:
            d["src_u8"] = u8.numpy()
        docs.append(d)
    batched, single, in_batch = _evaluate(monkeypatch, tmp_path, lambda: [dict(d) for d in docs])
    assert in_batch == {"unwarp_u8": 0, "ingest_u8": 0}
    for (pa, a), (pb, b), shp in zip(batched, single, shapes):
        assert pa == pb and tuple(a.shape) == shp + (3,) and torch.equal(a, b), shp
