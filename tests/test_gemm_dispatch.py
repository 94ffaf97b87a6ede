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


def test_kernel_name_refuses_what_dispatch_refuses():
    d = lib.GemmDesc()
    assert lib.gemm_kernel_name(d) == ""                          # null pointers
    d.dtype, d.M, d.N, d.K, d.batch = 0, 512, 256, 100, 1          # K not a multiple of 64
    d.A, d.B, d.C32, d.lda, d.ldb, d.ldc, d.lo_scale = 1 << 20, 1 << 21, 1 << 22, 128, 128, 256, 1.0
    assert lib.gemm_kernel_name(d) == ""
    d.K = 128
    assert lib.gemm_kernel_name(d) != ""
