"""CPU-side checks of the C-ABI library: it loads, and exports every symbol include/dvd_hip.h
declares (no compute calls - there is no GPU here)."""
import os

import pytest
import re

from dvd_amd import lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "dvd_amd", "csrc")
# the generators of the committed loop bodies (dvd_amd/csrc/*_body.inc) and the experiment switches each of them accepts, with
# a non-default value that it can emit (gen_common.py: SWITCHES)
GENERATORS = {
    "gen_attn_r64m.py": [],
    "gen_attn_r64x.py": [["--sum-by-dot2"], ["--pk-args"], ["--wait-every-step"]],
    "gen_attn_h64m.py": [],
    "gen_attn_h64x.py": [["--l-spread"], ["--sum-by-dot2"], ["--wait-every-step"]],
    "gen_gemm_t384.py": [["--pieces", "0,2,4,6,8"], ["--x-pieces", "2.1,2.3,2.5,2.7,3.1"], ["--x-bar", "1"]],
}


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "dvd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dvd_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    syms = declared_symbols()
    assert len(syms) >= 8
    raw = lib.raw()
    missing = [s for s in syms if not hasattr(raw, s)]
    assert not missing, missing


def test_python_binding_table_matches_header():
    syms = set(declared_symbols()) - {"dvd_last_error", "dvd_version", "dvd_engine_workspace_bytes",
                                      "dvd_flash_attn_kernel_name", "dvd_convnet_workspace_bytes",
                                      "dvd_convnet_weight_floats", "dvd_ingest_scratch_bytes"}
    assert syms == set(lib.SIGNATURES), (syms ^ set(lib.SIGNATURES))


def test_product_library_reads_no_environment_and_ships_no_experiments():
    """The product .so has no getenv import and none of the lab's experiment kernels / switch names; the lab build
    (benchmarks/lab/libdvd_hip_lab.so, -DDVD_LAB) is where those live."""
    import subprocess
    so = os.path.join(ROOT, "dvd_amd", "libdvd_hip.so")
    dyn = subprocess.run(["nm", "-D", so], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in dyn
    blob = open(so, "rb").read()
    for needle in (b"DVD_ATTN_", b"DVD_GEMM_", b"DVD_WARP_", b"DVD_DWCONV_", b"flash_attn_pipe_kernel", b"flash_attn_dsplit_kernel",
                   b"flash_attn_glds64x2_kernel", b"gemm_nt_big16_kernel", b"DVD_HIP_LIB"):
        assert needle not in blob, needle
    assert "dvd_attn_debug_stamps" not in dyn and "dvd_gemm_debug_stamps" not in dyn


def test_attention_kernel_choice_depends_on_shape_only():
    assert lib.flash_attn_kernel_name(256, 20736, 20736) == "flash_attn_r64x_kernel<0>"
    assert lib.flash_attn_kernel_name(256, 1024, 1024) == "flash_attn_glds_kernel<256, 0>"
    assert lib.flash_attn_kernel_name(256, 1296, 1296) == "flash_attn_kernel<256>"
    assert lib.flash_attn_kernel_name(64, 20736, 20736) == "flash_attn_h64x_kernel<0, true>"
    assert lib.flash_attn_kernel_name(64, 1024, 1024) == "flash_attn_glds_kernel<64, 0>"
    assert lib.flash_attn_kernel_name(64, 1296, 1296) == "flash_attn_kernel<64>"


def test_version_and_error_string():
    assert lib.version() >= 1000
    assert isinstance(lib.raw().dvd_last_error(), bytes)


def test_argument_validation_without_gpu():
    # null pointers are rejected before any HIP call
    import ctypes as C
    rc = lib.raw().dvd_unwarp_f32(None, 16, None, None, 10, 10, C.c_float(0.987), None)
    assert rc == -1 and b"null" in lib.raw().dvd_last_error()


def test_header_is_plain_c():
    """The boundary is a C ABI: include/dvd_hip.h (and the lab header) compile as C99 and as C++ with no torch / HIP types."""
    import subprocess
    for hdr in ("include/dvd_hip.h", "benchmarks/lab/dvd_hip_lab.h"):
        path = os.path.join(ROOT, hdr)
        subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", path], check=True)
        subprocess.run(["g++", "-fsyntax-only", "-x", "c++", path], check=True)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvd_hip.h")).read(), flags=re.S)   # code only
    assert "torch" not in text.lower() and "hipStream_t" not in text and "#include <hip" not in text


def test_generated_attention_body_is_current():
    """The hand-allocated loops are GENERATED and committed: dvd_amd/csrc/attn_r64x_body.inc (the decoder attention kernel,
    flash_attn_r64x_kernel) and attn_h64x_body.inc / attn_h64l_body.inc (head_dim 64, flash_attn_h64x_kernel), attn_r64m_body.inc
    and attn_h64m_body.inc (their 32x32x16-MFMA siblings, lab dispatch only) and gemm_t384_body.inc (gemm_nt_t384_kernel's K
    loop).  The committed files must be what the committed generators write."""
    for name in GENERATORS:
        assert _gen(name, "--check").returncode == 0, f"run python3 dvd_amd/csrc/{name}"


def _gen(name, *args, env=None):
    import subprocess
    import sys
    return subprocess.run([sys.executable, os.path.join(CSRC, name), *args], env=env, capture_output=True, text=True)


def _committed_bodies():
    """name -> (content, mtime) of every generated file beside the generators"""
    return {f: (open(os.path.join(CSRC, f), "rb").read(), os.stat(os.path.join(CSRC, f)).st_mtime_ns)
            for f in sorted(os.listdir(CSRC)) if f.endswith(".inc")}


def test_generators_ignore_the_environment():
    """The experiment switches were environment variables once; a value left over from an A/B session must not reach a body."""
    env = dict(os.environ, T384_PIECES="0,2,4,6,8", T384X_PIECES="2.1,2.5,3.1,3.5", T384X_BAR="3", H64X_L_SPREAD="1",
               R64X_SUM_BY_DOT2="1", R64X_PK_ARGS="1", R64X_WAIT_EVERY_STEP="1")
    for name in GENERATORS:
        r = _gen(name, "--check", env=env)
        assert r.returncode == 0, (name, r.stderr[-300:])
    for name in list(GENERATORS) + ["gen_common.py"]:
        assert not re.search(r"\benviron\b|getenv", open(os.path.join(CSRC, name)).read()), name


@pytest.mark.parametrize("name,flag", [(n, f) for n, flags in GENERATORS.items() for f in flags], ids=lambda v: v if isinstance(v, str) else v[0])
def test_generator_experiment_switch_cannot_touch_committed_bodies(name, flag, tmp_path):
    """An experiment switch is refused with --check and without --out-dir (exit 2 = a usage error, not 1 = `stale`); with
    --out-dir it writes there, something other than the committed bodies, and leaves those alone."""
    before = _committed_bodies()
    assert len(before) == 6
    for extra in (["--check"], [], ["--lab"], ["--out-dir", CSRC]):
        r = _gen(name, *flag, *extra)
        assert r.returncode == 2 and "experiment switch" in r.stderr, (extra, r.returncode, r.stderr[-300:])
    r = _gen(name, *flag, "--out-dir", str(tmp_path))
    assert r.returncode == 0, r.stderr[-300:]
    wrote = {f: (tmp_path / f).read_bytes() for f in os.listdir(tmp_path)}
    assert wrote and set(wrote) <= set(before), sorted(wrote)
    assert any(text != before[f][0] for f, text in wrote.items()), "the switch changed nothing"
    assert _committed_bodies() == before


def test_generator_rejects_flags_it_does_not_know():
    """An unknown flag, an abbreviated one or a switch of another generator is an error - never ignored."""
    theirs = [f for flags in GENERATORS.values() for f in flags]
    before = _committed_bodies()
    for name, mine in GENERATORS.items():
        for flag in [["--bogus"], ["--l"], ["bogus"]] + [f for f in theirs if f[0] not in [m[0] for m in mine]]:
            for extra in ([], ["--check"]):
                r = _gen(name, *flag, *extra)
                assert r.returncode == 2, (name, flag, extra, r.returncode, r.stderr[-300:])
    assert _committed_bodies() == before


def test_t384_gemm_kernel_resources(tmp_path):
    """gemm_nt_t384_kernel's K loop owns v[88:127] (declared clobbers) and its twelve accumulators are OUTPUT operands of the
    statement (round 6: pinned to a[0:127] + v[24:87] so that the 16x16x32 loop can name their quads): every product instance must still fit two waves per SIMD, and the three fast
    epilogue flavours on full tiles - what the bench runs - must not reload a spill inside their store streams (a scratch
    load behind a global store waits for that store's acknowledgement).  Checked on hipcc's own report and ISA."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "dvd_amd", "csrc", "gemm_t384.hip")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "--cuda-device-only"]
    r = subprocess.run(base + ["-c", src, "-o", str(tmp_path / "t.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    occ = re.findall(r"Function Name: (\S*gemm_nt_t384_kernel\S*).*?Occupancy \[waves/SIMD\]: (\d+)", r.stderr, re.S)
    assert len(occ) == 10 and all(int(o) == 2 for _, o in occ), occ
    subprocess.run(base + ["-S", src, "-o", str(tmp_path / "t.s")], check=True, stderr=subprocess.DEVNULL)
    text = (tmp_path / "t.s").read_text()
    for fl in (0, 1):                                   # f16 and f32 flavours, full tiles
        name = f"_ZN3dvd19gemm_nt_t384_kernelILi0ELi{fl}ELb1ELb1EEEvNS_8GemmArgsE"      # <DBG 0, FL, FULL, X16>
        body = text[text.index(name + ":"):]
        body = body[:body.index(".end_amdhsa_kernel")].split("\n")
        last_mfma = max(i for i, ln in enumerate(body) if "v_mfma" in ln)
        stores_seen, bad = 0, []
        for ln in body[last_mfma:]:
            if "global_store" in ln:
                stores_seen += 1
            if "scratch_load" in ln and stores_seen > 8:
                bad.append(ln.strip())
        assert stores_seen >= 80 and len(bad) <= 3, (fl, stores_seen, bad[:5])     # (hipcc rotates the tile loop: a few stores sit above the K loop)


def test_attention_kernel_register_contract(tmp_path):
    """flash_attn_r64x_kernel (production) hands v[28:255] and every AGPR to its generated asm statements
    (amdgpu_num_vgpr(28)), flash_attn_h64x_kernel v[32:175] and a[0:79] (round 6: a[64:79] = the row-sum tiles); the lab siblings flash_attn_r64m_kernel / h64m likewise.  Checked on the ISA hipcc produces from the
    committed source: outside the asm statements the kernels name no VGPR of the statements' and no AGPR, and they use no
    scratch (dvd_amd/csrc/check_r64m_isa.py) - with 28 VGPRs hipcc did park per-lane values in a0..a2 until the epilogue
    stopped keeping them live."""
    import shutil
    import subprocess
    import sys
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = CSRC
    for gen in GENERATORS:                              # the lab build's ablation bodies
        if gen.startswith("gen_attn"):
            subprocess.run([sys.executable, os.path.join(csrc, gen), "--lab"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, csrc)
    import check_r64m_isa
    out = tmp_path / "attention.s"
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only", "-o", str(out)]
    subprocess.run(base + [os.path.join(csrc, "attention.hip")], check=True, stderr=subprocess.DEVNULL)
    for name, nv in (("flash_attn_r64x_kernel", 28), ("flash_attn_h64x_kernel", 32)):   # the product library: the production kernels only
        kernels, bad = check_r64m_isa.check(out.read_text(), nv, name)
        assert kernels == 1 and not bad, (name, bad[:10])
    subprocess.run(base + ["-DDVD_LAB", os.path.join(csrc, "attention.hip")], check=True, stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels, bad = check_r64m_isa.check(text, 28, "flash_attn_r64x_kernel")
    assert kernels >= 2 and not bad, bad[:10]
    kernels, bad = check_r64m_isa.check(text)
    assert kernels >= 2 and not bad, bad[:10]
    kernels, bad = check_r64m_isa.check(text, 32, "flash_attn_h64m_kernel")
    assert kernels >= 2 and not bad, bad[:10]
    kernels, bad = check_r64m_isa.check(text, 32, "flash_attn_h64x_kernel")
    assert kernels >= 2 and not bad, bad[:10]
