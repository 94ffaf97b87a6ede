"""The kernels of dvd_amd/csrc/flowviz.hip against the NumPy definition tests/flowviz_model.py, byte for byte; the
drop-in datasets/utils/flow_viz.py against the reference's goldens; settings.flow_outputs through the launcher.  Expected values
come from the model at test time.  Shapes: 1 x 1, 1 x 67 and 33 x 31 have no side (and no pixel count) that is a multiple of the
four-pixel store group, so the last lane stores bytes, and with n = 3 a group spans two images; one image of 130 x 257 takes
33 workgroups of the picture kernel and nine of the radius reduction, whose last one is partly empty."""
import numpy as np
import pytest
import torch

import flowviz_model as M
from flowviz_fixtures import CASES, SHARE_BAR, UPSAMPLE_SHAPES, coarse_maps, golden, odd_field

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, F).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("norm", M.NORMS)
def test_flow_to_image_equals_the_model_on_the_goldens(norm):
    from dvd_amd import ops
    for name in CASES:
        field, _, clip, bgr = golden(name)
        want = M.flow_to_image(field, clip, bgr, norm)
        assert np.array_equal(ops.flow_to_image(_dev(field), clip, bgr, norm).cpu().numpy(), want), name        # n = 1, as [H,W,2]
        three = np.stack([field, field[::-1], 0.5 * field[:, ::-1]]).astype(F)
        got = ops.flow_to_image(_dev(three), clip, bgr, norm).cpu().numpy()
        assert got.shape == three.shape[:3] + (3,)
        for k in range(3):
            assert np.array_equal(got[k], M.flow_to_image(three[k], clip, bgr, norm)), (name, k)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 67), (33, 31), (130, 257)])
def test_flow_to_image_equals_the_model_on_odd_sizes(h, w):
    from dvd_amd import ops
    fields = np.stack([odd_field(h, w, seed) for seed in range(3)])
    dev = _dev(fields)
    for norm in M.NORMS:
        for clip, bgr in ((None, False), (0.4 * max(h, w), True), (None, True)):
            got = ops.flow_to_image(dev, clip, bgr, norm).cpu().numpy()
            for k in range(3):
                assert np.array_equal(got[k], M.flow_to_image(fields[k], clip, bgr, norm)), (norm, clip, bgr, k)
    assert np.array_equal(ops.flow_to_image(dev[1]).cpu().numpy(), M.flow_to_image(fields[1]))


def test_flow_radius_max_equals_the_model_and_repeats():
    from dvd_amd import ops
    for h, w in ((1, 1), (33, 31), (130, 257)):
        fields = np.stack([odd_field(h, w, seed) for seed in range(3)])
        dev = _dev(fields)
        for clip in (None, 0.4 * max(h, w)):
            first, second = ops.flow_radius_max(dev, clip), ops.flow_radius_max(dev, clip)
            want = np.asarray([M.radius_max(f, clip) for f in fields], F)
            assert np.array_equal(_bits(first), _bits(want)) and np.array_equal(_bits(first), _bits(second)), (h, w, clip)
        assert ops.flow_radius_max(dev[2]).dim() == 0 and float(ops.flow_radius_max(dev[2])) == float(M.radius_max(fields[2]))
    assert float(ops.flow_radius_max(_dev(np.full((3, 3, 2), np.nan, F)))) == 0.0


@pytest.mark.parametrize("g,h,w", UPSAMPLE_SHAPES)
def test_full_uv_and_the_fused_picture(g, h, w):
    from dvd_amd import ops
    flow = coarse_maps(g)
    dev = _dev(flow)
    uv = ops.flow_full_uv(dev, h, w)
    assert np.array_equal(_bits(uv), _bits(np.stack([M.full_uv(m, h, w) for m in flow])))
    assert np.array_equal(_bits(ops.flow_full_uv(dev[1], h, w)), _bits(M.full_uv(flow[1], h, w)))
    for norm in M.NORMS:
        pic, largest = ops.flow_picture(dev, h, w, norm=norm, return_radius=True)
        assert torch.equal(pic, ops.flow_to_image(uv, norm=norm)), norm
        assert np.array_equal(pic.cpu().numpy(), np.stack([M.flow_picture(m, h, w, norm) for m in flow])), norm
        assert torch.equal(ops.flow_picture(dev, h, w, norm=norm, convert_to_bgr=True), pic.flip(-1))
        if norm == "max":
            assert torch.equal(largest, ops.flow_radius_max(uv))
        else:
            assert largest is None


def test_drop_in_flow_viz_on_numpy_and_on_tensors():
    from datasets.utils import flow_viz
    differ = total = 0
    for name in CASES:
        field, image, clip, bgr = golden(name)
        got = flow_viz.flow_to_image(field, clip_flow=clip, convert_to_bgr=bgr)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == image.shape
        d = np.abs(got.astype(np.int32) - image.astype(np.int32))
        assert d.max() <= 1, name
        differ, total = differ + int((d > 0).sum()), total + d.size
        on_dev = flow_viz.flow_to_image(_dev(field), clip, bgr)
        assert torch.is_tensor(on_dev) and on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), got)
    assert differ / total <= SHARE_BAR, (differ, total)
    assert np.array_equal(flow_viz.flow_to_image(golden("anchors")[0]), golden("anchors")[1])
    field = golden("smooth")[0]
    assert np.array_equal(flow_viz.flow_to_image(field.astype(np.float64), norm="max"), M.flow_to_image(field, norm="max"))
    # normalised components: radius 1/2 along +x is the wheel's colour for a = atan2(-0, -1/2) / pi = -1 (red), half way to white
    u, v = np.full((4, 6), 0.5, F), np.zeros((4, 6), F)
    assert flow_viz.flow_uv_to_colors(u, v)[0, 0].tolist() == [255, 127, 127]
    assert flow_viz.flow_uv_to_colors(u, v, convert_to_bgr=True)[0, 0].tolist() == [127, 127, 255]
    with pytest.raises(ValueError, match="three dimensions"):
        flow_viz.flow_to_image(np.zeros((4, 4), F))
    with pytest.raises(ValueError, match=r"\[H,W,2\]"):
        flow_viz.flow_to_image(np.zeros((4, 4, 3), F))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
PATHS = ["synthetic_00000", "synthetic_00001"]
SIZE = (96, 80)


def _launcher(monkeypatch, tmp_path):
    import types
    import admin.settings as ws
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    made = []

    class Small(ws.Settings):
        def __init__(self):
            super().__init__()
            self.env.grid_size, self.env.diffusion_steps = 16, 2
            self.env.num_synthetic_docs, self.env.batch_docs, self.env.full_res = 2, 2, SIZE
            self.env.visualize, self.env.use_prestage_nets = True, True
            self.env.eval_dataset_name = "synthetic"
            made.append(self)
    monkeypatch.setattr(R, "ws_settings", types.SimpleNamespace(Settings=Small))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))
    return R, made


def test_run_writes_the_maps_and_a_run_without_the_attribute_does_not(tmp_path, monkeypatch):
    """G = 16, 2 steps, synthetic weights, two synthetic image documents, keyed noise (so that two runs sample the same maps)."""
    from PIL import Image
    from dvd_amd import evaluation, ops
    R, made = _launcher(monkeypatch, tmp_path)
    R.run_sampling("dvd", "val_TDiff", 77, "with", keyed_noise=True, flow_outputs="png,flo,npy")
    R.run_sampling("dvd", "val_TDiff", 77, "without", keyed_noise=True)
    with_, without = made
    assert with_.flow_outputs == "png,flo,npy" and not hasattr(without, "flow_outputs")
    root = tmp_path / "vis_hp" / "synthetic"
    assert sorted(f.name for f in (root / "with" / "pred_flow").iterdir()) == sorted(f"flow_{p}.{e}" for p in PATHS for e in ("png", "flo", "npy"))
    assert (root / "without" / "pred_flow").is_dir() and list((root / "without" / "pred_flow").iterdir()) == []
    h, w = SIZE
    for i, p in enumerate(PATHS):
        coarse = np.load(root / "with" / "pred_flow" / f"flow_{p}.npy")
        assert coarse.shape == (2, 16, 16) and coarse.dtype == np.float32 and np.abs(coarse).max() <= 1
        assert np.array_equal(coarse, with_.map_ref[p].numpy())                                   # the map the sampler returned
        dev = _dev(coarse)
        picture = np.asarray(Image.open(root / "with" / "pred_flow" / f"flow_{p}.png"))
        assert picture.shape == (h, w, 3) and np.array_equal(picture, ops.flow_picture(dev, h, w, norm="max").cpu().numpy())
        assert np.array_equal(_bits(ops.flow_read_flo(str(root / "with" / "pred_flow" / f"flow_{p}.flo"))), _bits(ops.flow_full_uv(dev, h, w)))
        page = np.asarray(Image.open(root / "with" / "dewarped_pred" / f"warped_{p}.png"))
        src = next(evaluation.synthetic_documents(with_, [i]))["image_u8"]
        assert np.array_equal(ops.unwarp_u8(dev[None].contiguous(), _dev(src)).cpu().numpy(), page)
        assert (root / "without" / "dewarped_pred" / f"warped_{p}.png").read_bytes() == \
            (root / "with" / "dewarped_pred" / f"warped_{p}.png").read_bytes()


def test_apply_map_reproduces_a_page(tmp_path):
    from PIL import Image
    from dvd_amd import apply_map, ops, synth
    coarse = coarse_maps(16, 1)[0] * F(0.2)
    src = np.ascontiguousarray((synth.smooth_image("flowviz/apply", 61, 47, seed=3).transpose(1, 2, 0) * 255).astype(np.uint8))
    np.save(tmp_path / "m.npy", coarse)
    Image.fromarray(src).save(tmp_path / "in.png")
    for mode in ("bilinear", "bicubic"):
        apply_map.main([str(tmp_path / "m.npy"), str(tmp_path / "in.png"), str(tmp_path / "out.png"), "--mode", mode])
        want = ops.unwarp_u8(_dev(coarse[None]), _dev(src), mode=mode).cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out.png")), want), mode
