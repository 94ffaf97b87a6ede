"""Which GEMM kernel every engine call site runs, and that the choice does not follow the batch (CPU only: dvd_gemm_kernel_name
is host-only, so the descriptors carry fabricated addresses of the engine's alignment).

A document must get the same bits alone and in a batch.  Where the kernel of a call site changes with the sample count, the
two kernels must be in one declared SAME-BITS class below, and each class names the GPU test that proves it."""
import os
import re

import pytest

from dvd_amd import lib

import gemm_callsites as CS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GRIDS = (16, 32, 64, 72, 96, 160, 288)
SAMPLES = (1, 2, 4, 6, 8, 16, 32, 64)

# class name -> (member kernels, the GPU test that shows they give the same bits)
SAME_BITS = {
    # small_tiles 1 vs 2 (the engine switches at 16 384 token rows) and the 128 x 128 family's tile-count choice
    "128x128 family": ({"gemm_nt_kernel<false, 2, false>", "gemm_nt_ring128_kernel", "gemm_nt_ring256_kernel",
                        "gemm_nt_big_kernel<0>/small_tiles 2"},
                       "tests/test_gpu_gemm.py::test_gemm_small_family_engine_shapes_same_bits, ::test_gemm_ring128_kernel"),
    # FULL (M % 384 == 0: no row masks, the XT ring that never drains) vs ragged, per epilogue flavour
    **{f"t384 FL{fl}": ({f"gemm_nt_t384_kernel<0, {fl}, true, true>", f"gemm_nt_t384_kernel<0, {fl}, false, true>"},
                        "tests/test_gpu_gemm_callsites.py::test_t384_full_and_ragged_same_bits")
       for fl in range(5)},
}


def bits_class(call, name):
    key = name + ("/small_tiles 2" if call.small_tiles == 2 and name.startswith("gemm_nt_big_kernel") else "")
    for cls, (members, _) in SAME_BITS.items():
        if key in members:
            return cls
    return key


def fake_address(buffers):
    """Every buffer at its own 256-byte aligned address (the workspace and w16dith are 256-byte aligned, weights at least 16)."""
    def addr(p):
        buf, off = p
        if buf not in buffers:
            buffers[buf] = (1 << 40) + len(buffers) * (1 << 36)
        return buffers[buf] + off
    return addr


def names(G, samples):
    bufs = {}
    addr = fake_address(bufs)
    out = []
    for c in CS.calls(G, samples, 1):
        out.append((c, lib.gemm_kernel_name(CS.descriptor(c, addr))))
    return out


def test_table_covers_every_engine_gemm_call():
    src = open(os.path.join(ROOT, "dvd_amd", "csrc", "engine.hip")).read()
    n = len(re.findall(r"TRY\(gemm\(", src))
    assert n == len(CS.SITES) == 19, (n, len(CS.SITES))
    # ... and in the engine's order: prepare_docs' four first, then enqueue_step's fifteen
    prep = src[src.index("extern \"C\" int dvd_engine_prepare_docs"):src.index("extern \"C\" int dvd_engine_feat_nchw")]
    assert len(re.findall(r"TRY\(gemm\(", prep)) == sum(1 for _, f in CS.SITES if f == "prepare") == 4
    got = []
    for c in CS.calls(72, 2, 1):
        if not got or got[-1] != c.site:
            got.append(c.site)
    order = [s for s, _ in CS.SITES]
    assert [s for s in dict.fromkeys(got)] == order


def test_every_call_site_is_accepted_and_aligned():
    """dvd_gemm_nt takes every descriptor of the table, and every pointer the engine passes is 16-byte aligned (what the
    engine's gemm() helper requires)."""
    for G in GRIDS:
        for s in (1, 2, 32):
            bufs = {}
            addr = fake_address(bufs)
            for c in CS.calls(G, s, 1):
                d = CS.descriptor(c, addr)
                assert lib.gemm_kernel_name(d) != "", (G, s, c.site, lib.raw().dvd_last_error())
                for f in CS.PTR_FIELDS:
                    v = getattr(c, f)
                    assert v is None or addr(v) % 16 == 0, (G, s, c.site, f)


def test_g288_kernels_are_the_profiled_ones():
    """G = 288, 8 documents x 2 hypotheses (the bench point): every call site runs the kernel profiles/r6_final_summary.txt
    shows for it."""
    want = {
        "pyr_conv0": "gemm_f32_narrow_kernel<2>",
        "patch_embed": "gemm_nt_kernel<true, 2, false>", "ca_k32": "gemm_nt_kernel<true, 2, false>",
        "ca_vt32": "gemm_nt_kernel<true, 2, false>",
        "r_embed": "gemm_nt_split128_kernel<true>", "ca_q": "gemm_nt_split128_kernel<true>",
        "ca_k": "gemm_nt_split128_kernel<true>", "ca_out": "gemm_nt_split128_kernel<true>",
        "sa_proj": "gemm_nt_split128_kernel<true>", "fc2": "gemm_nt_split128_kernel<true>",
        "ca_vt": "gemm_nt_ring256_kernel", "sa_vt": "gemm_nt_ring256_kernel",
        "sa_qk": "gemm_nt_t384_kernel<0, 0, true, true>", "fc1": "gemm_nt_t384_kernel<0, 0, true, true>",
        "dec_qk": "gemm_nt_t384_kernel<0, 0, true, true>", "dec_vt": "gemm_nt_t384_kernel<0, 0, true, true>",
        "dec_conv1": "gemm_nt_t384_kernel<0, 0, true, true>",
        "dec_fc": "gemm_nt_t384_kernel<0, 2, true, true>", "dec_conv2": "gemm_nt_t384_kernel<0, 2, true, true>",
    }
    assert set(want) == {s for s, _ in CS.SITES}
    bufs = {}
    addr = fake_address(bufs)
    count = {}
    for c in CS.calls(288, 8, 2):
        name = lib.gemm_kernel_name(CS.descriptor(c, addr))
        assert name == want[c.site], (c.site, name)
        count[name] = count.get(name, 0) + 1
    # the launch counts of one evaluation + one prepare against the 50-step profile (kernel, calls / 50 or per prepare)
    prof = open(os.path.join(ROOT, "profiles", "r6_final_summary.txt")).read()
    for name, n in count.items():
        m = re.search(r"dvd::" + re.escape(name) + r"\(dvd::GemmArgs\)\s+(\d+)", prof)
        assert m, name
        calls = int(m.group(1))
        if name.startswith("gemm_nt_kernel<true") or name.startswith("gemm_f32_narrow"):
            assert calls == n, (name, calls, n)        # once per prepare
        else:
            assert calls == 50 * n, (name, calls, n)   # once per evaluation, 50 evaluations


@pytest.mark.parametrize("G", GRIDS)
def test_kernel_choice_does_not_follow_the_batch(G):
    """Per call site and grid, the kernel is the same for every sample count - or in one declared same-bits class."""
    per_site = {}
    for s in SAMPLES:
        if 4 * (G // 2) ** 2 * s >= 1 << 31:
            continue
        for c, name in names(G, s):
            assert name, (G, s, c.site)
            per_site.setdefault(c.site, {}).setdefault(bits_class(c, name), set()).add((s, name))
    for site, classes in per_site.items():
        assert len(classes) == 1, f"G={G} {site}: the kernel follows the batch across classes {classes}"


def test_the_t384_full_and_ragged_class_is_exercised():
    """The FULL / ragged t384 class is not hypothetical: at G = 72 one document (2 592 rows) runs the ragged instance and a
    batch of four (10 368 = 27 x 384 rows) the FULL one, on the same call sites."""
    one = {c.site: n for c, n in names(72, 2)}
    four = {c.site: n for c, n in names(72, 8)}
    for site in ("dec_qk", "dec_conv1"):
        assert one[site] == "gemm_nt_t384_kernel<0, 0, false, true>" and four[site] == "gemm_nt_t384_kernel<0, 0, true, true>"
    for site in ("dec_fc", "dec_conv2"):
        assert one[site] == "gemm_nt_t384_kernel<0, 2, false, true>" and four[site] == "gemm_nt_t384_kernel<0, 2, true, true>"


def test_unaligned_output_leaves_t384_so_the_engine_requires_alignment():
    """A 4-byte-aligned C or residual pointer moves a t384 call site to gemm_nt_big_kernel, whose bits differ since round 6.
    This is not a same-bits class: the engine instead guarantees the alignment - its workspace must be 256-byte aligned and
    every weight 16-byte aligned (refused otherwise, below), the buffer offsets keep it (test_every_call_site_is_accepted_and_aligned),
    and its gemm() helper refuses an unaligned pointer."""
    bufs = {}
    addr = fake_address(bufs)
    seen = 0
    for c in CS.calls(288, 2, 1):
        d = CS.descriptor(c, addr)
        if not lib.gemm_kernel_name(d).startswith("gemm_nt_t384_kernel"):
            continue
        seen += 1
        for f in ("C32", "C16", "res"):
            if getattr(d, f):
                setattr(d, f, getattr(d, f) + 4)
        assert lib.gemm_kernel_name(d) == "gemm_nt_big_kernel<0>", c.site
    assert seen == 2 + 5 * 6           # sa_qk, fc1 and five decoder GEMMs per layer
    # the engine refuses the misalignment where it would enter
    import ctypes as C
    h = C.c_void_p()
    lib.call("dvd_engine_create", 16, 1, 2, C.byref(h))
    try:
        need = lib.raw().dvd_engine_workspace_bytes(h)
        assert lib.raw().dvd_engine_bind_workspace(h, C.c_void_p((1 << 40) + 4), need) != 0
        assert b"256-byte aligned" in lib.raw().dvd_last_error()
        name, dt, ne = C.c_char_p(), C.c_int(), C.c_long()
        lib.call("dvd_engine_tensor_info", h, 0, C.byref(name), C.byref(dt), C.byref(ne))
        assert lib.raw().dvd_engine_set_tensor(h, name.value, C.c_void_p((1 << 40) + 4), ne.value) != 0
        assert b"16-byte aligned" in lib.raw().dvd_last_error()
    finally:
        lib.raw().dvd_engine_destroy(h)


# ---- the lab build's DVD_GEMM_* switches: each still chooses what it chose before the instance table ----
# tests/golden/gemm_lab_names.json is the recording: lab_names() below, run in record mode (`python tests/test_gemm_dispatch.py
# --record LIB`) on the lab library of the commit before the instance table.
LAB_RECORDING = os.path.join(ROOT, "tests", "golden", "gemm_lab_names.json")
RINGS_OFF = {"RING128": "0", "RING256": "0"}
LAB_SWITCHES = [{}, {"V1": "1"}, {"TWOPASS": "1"}, {"SCALAR_EPILOGUE": "1"}, {"SPREAD": "1"}, {"NO_T384": "1"},
                {"NO_T384": "1", "SPREAD": "1"}, {"DEBUG": "1"}, {"DEBUG": "3"}, {"DEBUG": "7"}, {"RING": "1"}, {"M16": "1"},
                {"BIG2": "1"}, {"RING128": "0"}, {"RING256": "0"}, {"RING256": "2"}, {"W8": "1", **RINGS_OFF},
                {"PD4": "1", **RINGS_OFF}, {"T384_M32": "1"}, {"T384_X16": "1"}, {"T384_DBG": "5"},
                *({"T384_M32": "1", "T384_DBG": str(n)} for n in range(1, 7))]
CODE = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"     # one character per distinct name


def switch_id(switches):
    return "+".join(f"{k}={v}" for k, v in switches.items()) or "none"


def hand_made(dtype=0, N=256, **fields):
    """A descriptor the engine never builds: 4096 x N x 256, f32 output, every pointer 256-byte aligned unless `fields` says so."""
    d = lib.GemmDesc()
    d.dtype, d.M, d.N, d.K, d.batch = dtype, 4096, N, 256, 1
    d.A, d.B, d.C32, d.lda, d.ldb, d.ldc, d.lo_scale = 1 << 40, 1 << 41, 1 << 42, 256, 256, N, 1.0
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def lab_descriptors():
    """(label, descriptor): the engine's call sites at three grids, alone and in a large batch, then what the engine never reaches."""
    for G in (16, 72, 288):
        for s in (2, 32):
            addr = fake_address({})
            for i, c in enumerate(CS.calls(G, s, 1)):
                yield f"G={G} s={s} #{i} {c.site}", CS.descriptor(c, addr)
    lo = 1 << 43
    yield "B_lo", hand_made(B_lo=lo)                                   # gemm_nt_split_kernel<true>
    yield "B_lo, lo_scale 0.5", hand_made(B_lo=lo, lo_scale=0.5)
    yield "A_lo", hand_made(A_lo=lo)
    yield "N=384", hand_made(N=384)                                    # gemm_nt_split128_kernel<false>
    for st in (1, 2):
        yield f"small_tiles {st}", hand_made(small_tiles=st)
        yield f"small_tiles {st}, B_lo", hand_made(small_tiles=st, B_lo=lo)
    yield "C + 4 bytes", hand_made(C32=(1 << 42) + 4)
    yield "N=100", hand_made(N=100)
    yield "f32 N=32", hand_made(dtype=1, N=32)                         # gemm_f32_narrow_kernel<1>
    yield "f32 N=64", hand_made(dtype=1, N=64)                         # gemm_f32_narrow_kernel<2>
    yield "f32 N=128", hand_made(dtype=1, N=128)


def lab_names():
    return [(label, lib.gemm_kernel_name(d)) for label, d in lab_descriptors()]


@pytest.mark.parametrize("switches", LAB_SWITCHES, ids=switch_id)
def test_lab_switches_choose_what_they_chose_before(lab, monkeypatch, switches):
    """For every descriptor, under every switch set, the lab library names the kernel that the recording holds."""
    import json
    for k in [k for k in os.environ if k.startswith("DVD_GEMM_")]:
        monkeypatch.delenv(k)
    for k, v in switches.items():
        monkeypatch.setenv("DVD_GEMM_" + k, v)
    rec = json.load(open(LAB_RECORDING))
    want = [rec["names"][CODE.index(ch)] for ch in rec["cases"][switch_id(switches)]]
    got = lab_names()
    assert len(got) == len(want)
    for (label, name), w in zip(got, want):
        assert name == w, (switch_id(switches), label, name, w)


def test_lab_recording_covers_every_instance():
    """The recording is worth something: it reaches every product instance dvd_gemm_nt has, both t384 K loops with their
    ablations, and every experiment kernel of the lab."""
    import json
    names = set(json.load(open(LAB_RECORDING))["names"])
    assert "" not in names
    for must in ("gemm_nt_split128_kernel<true>", "gemm_nt_split128_kernel<false>", "gemm_nt_split_kernel<true>", "gemm_nt_big_kernel<0>",
                 "gemm_f32_narrow_kernel<1>", "gemm_f32_narrow_kernel<2>", "gemm_nt_ring256_kernel", "gemm_nt_ring128_kernel",
                 "gemm_nt_kernel<false, 2, false>", "gemm_nt_kernel<true, 2, false>", "gemm_nt_split_kernel<false>",
                 "gemm_nt_big16_kernel", "gemm_nt_big2_kernel", "gemm_nt_w8_kernel", "gemm_nt_kernel<false, 4, false>",
                 "gemm_nt_kernel<true, 4, false>", "gemm_nt_big_kernel<1>", "gemm_nt_big_kernel<3>", "gemm_nt_big_kernel<4>",
                 "gemm_nt_big_kernel<7>", "gemm_nt_t384_kernel<5, 0, true, true>", "gemm_nt_t384_kernel<0, 0, true, false>",
                 *(f"gemm_nt_t384_kernel<{n}, 0, true, false>" for n in range(1, 7))):
        assert must in names, must


def test_kernel_name_refuses_what_dispatch_refuses():
    d = lib.GemmDesc()
    assert lib.gemm_kernel_name(d) == ""                          # null pointers
    d.dtype, d.M, d.N, d.K, d.batch = 0, 512, 256, 100, 1          # K not a multiple of 64
    d.A, d.B, d.C32, d.lda, d.ldb, d.ldc, d.lo_scale = 1 << 20, 1 << 21, 1 << 22, 128, 128, 256, 1.0
    assert lib.gemm_kernel_name(d) == ""
    d.K = 128
    assert lib.gemm_kernel_name(d) != ""


if __name__ == "__main__":       # record mode: python tests/test_gemm_dispatch.py --record path/to/libdvd_hip_lab.so
    import json
    import sys
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gemm_dispatch.py --record LAB_LIBRARY"
    lib.use_library(sys.argv[2])
    names, cases = [], {}
    for switches in LAB_SWITCHES:
        for k in [k for k in os.environ if k.startswith("DVD_GEMM_")]:
            del os.environ[k]
        os.environ.update({"DVD_GEMM_" + k: v for k, v in switches.items()})
        row = []
        for _, name in lab_names():
            if name not in names:
                names.append(name)
            row.append(CODE[names.index(name)])
        cases[switch_id(switches)] = "".join(row)
    header = ("dvd_gemm_kernel_name of the LAB library built from the commit before the GEMM instance table, per switch set "
              "(DVD_GEMM_ + key) and descriptor of tests/test_gemm_dispatch.py::lab_descriptors, recorded by that file's record "
              "mode; cases[switch set][i] is the position in CODE of descriptor i's name in `names`")
    json.dump({"header": header, "names": names, "cases": cases}, open(LAB_RECORDING, "w"), indent=1)
    print(len(cases), "switch sets x", len(row), "descriptors,", len(names), "distinct names")
