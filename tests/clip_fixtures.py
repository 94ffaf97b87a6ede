"""Shared by tests/test_clip_host.py and tests/test_gpu_clip.py: the clip_denoised / denoised_fn / iter=False fixtures of
tests/tools/gen_clip_golden.py and the bar of the GPU loop tests (the CPU test needs it too: the fixtures must move the
result by at least 10 x that bar, or a build that ignores a flag could pass)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The project's rule: RMSE measured on the MI355X x 3, never above north_star's 1e-3.  See tests/test_gpu_clip.py and
# DESIGN.md section 5 for where this figure comes from.
LOOP_BAR = 2.7e-4
SINGLE_STEP_BAR = 2.7e-4        # tests/test_gpu_dropin.py::test_single_step_signatures_vs_reference_golden's bar for 'sample'

LOOPS = {"clip": "loop_g64_s10_clip.npz", "noiter": "loop_g64_s10_noiter.npz", "fn": "loop_g32_s10_fn.npz",
         "noiterfeat": "loop_g32_s10_noiter_feat.npz"}


def noiterfeat_init_feat():
    """The non-zero init_feat of loop_g32_s10_noiter_feat.npz ([1,256,32,32]; regenerated, not stored)."""
    from dvd_amd import synth
    return synth.uniform("clip/init_feat", (1, 256, 32, 32), 0.0, 1.5, 1234)


def load(tag):
    return np.load(os.path.join(GOLD, LOOPS.get(tag, tag)))


def fn_of(g):
    """The fixture's denoised_fn (None if it has none): x -> fn_scale * x in float32, as the generator's lambda."""
    scale = float(g["fn_scale"])
    if scale == 1.0:
        return None
    return lambda x: scale * x


def processed(g):
    """pred_xstart per step as the reference returned it ([S,1,2,G,G], hypothesis 0)."""
    return g["pred_steps"] if "pred_steps" in g.files else g["raw_steps"]


def rmse(a, b):
    return float(np.sqrt(((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2).mean()))
