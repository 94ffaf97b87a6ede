"""The PNG encoder's dynamic-Huffman route without a GPU (format: DESIGN.md 4.4; kernels: tests/test_gpu_png_dyn.py): the shared
code builder of png_core.h through `png_host_check --code-lengths`, whole files of the CPU restatement `png_host_check ...
dynamic` taken apart by png_dyn_model.parse_blocks, the digests both routes are held to, and the argument / env checks.  The host
program is built with -fsanitize=address,undefined and works in exact-size buffers, as in tests/test_png_cpu.py."""
import ctypes as C
import hashlib
import io
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import png_dyn_model as D
import png_model as P
from host_check import build_host_check
from dvd_amd import lib, ops

ROOT = P.ROOT
S = D.S


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_host_check("png", tmp_path_factory.mktemp("png_dyn_host"))


def _lengths(exe, freq, limit):
    r = subprocess.run([str(exe), "--code-lengths", str(limit)] + [str(f) for f in freq], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [int(v) for v in r.stdout.split()]
    assert len(out) == len(freq)
    return out


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _histograms(limit):
    """Fibonacci histograms of 8..30 symbols (the limit binds), flat ones, one and two symbols, 200 seeded random ones."""
    out = [_fib(n) for n in range(8, 31)] + [list(reversed(_fib(n))) for n in (9, 17, 30)]
    out += [[7] * n for n in (2, 3, 4, 5, 16, 19, 30, min(286, 1 << limit))] + [[1] * 19]
    out += [[5], [0, 0, 9, 0], [3, 0, 0, 4], [1, 1], [0, 1000, 1]]
    rng = np.random.RandomState(limit)
    for k in range(200):
        n = int(rng.randint(2, (19 if limit == 7 else 286) + 1))
        kind = k % 4
        if kind == 0:
            f = rng.randint(0, 50, n)
        elif kind == 1:
            f = (rng.exponential(1.0, n) ** 3 * 40).astype(np.int64)
        elif kind == 2:
            f = rng.randint(0, 3, n) * rng.randint(1, 30000, n)
        else:
            f = np.floor(1.7 ** rng.permutation(n).clip(0, 27)).astype(np.int64) * (rng.rand(n) < 0.8)
        out.append([int(v) for v in f])
    assert all(len(f) <= (1 << limit) for f in out)
    return out


@pytest.mark.parametrize("limit", [15, 7])
def test_code_builder_is_optimal_within_the_limit_and_complete(host_check, limit):
    """Within the limit and complete (one used symbol: length 1, the incompleteness zlib tolerates for distances and the
    header rule repairs for the code-length code; none: all 0); equal in cost to the heap optimum whenever that fits the
    limit; the same on a second run."""
    binds = 0
    for freq in _histograms(limit):
        got = _lengths(host_check, freq, limit)
        used = [k for k, f in enumerate(freq) if f]
        assert [k for k, n in enumerate(got) if n] == used, (freq, got)
        assert max(got + [0]) <= limit, (freq, got)
        if len(used) == 1:
            assert got[used[0]] == 1
        elif used:
            assert sum(1 << (limit - n) for n in got if n) == 1 << limit, (freq, got)
        cost, depth = D.huffman_optimum(freq)
        mine = sum(f * n for f, n in zip(freq, got))
        if depth <= limit:
            assert mine == cost, (freq, got, cost)
        else:
            binds += 1
            assert mine >= cost
        assert _lengths(host_check, freq, limit) == got
    assert binds >= 10, binds


def test_code_lengths_mode_refuses_what_the_builder_cannot_take(host_check):
    for args in (["16", "1", "2"], ["0", "1", "2"], ["2", "1", "1", "1", "1", "1"], ["15", "-1", "2"], ["15", str(1 << 23), "1"]):
        r = subprocess.run([str(host_check), "--code-lengths"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout == "", args


# ---- whole files --------------------------------------------------------------------------------------------------------------
def _host_encode(exe, img, tmp_path, *mode):
    h, w, _ = img.shape
    img.tofile(tmp_path / "in.rgb")
    r = subprocess.run([str(exe), str(h), str(w), str(tmp_path / "in.rgb"), str(tmp_path / "out.png"), *mode], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return (tmp_path / "out.png").read_bytes()


@pytest.fixture(scope="module")
def files(host_check, tmp_path_factory):
    """name -> (fixed-mode file in the five-argument form, dynamic-mode file), each encoded once."""
    tmp = tmp_path_factory.mktemp("png_dyn_files")
    return {name: (_host_encode(host_check, D.case(name), tmp), _host_encode(host_check, D.case(name), tmp, "dynamic"))
            for name in D.DIGEST_CASES}


def _digest(data):
    return {"length": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def _golden(which):
    table = json.load(open(os.path.join(D.GOLDEN, f"png_{which}_digests.json")))
    return {name: {k: v[k] for k in ("length", "sha256")} for name, v in table.items()}


def test_both_routes_reproduce_their_digests(files):
    """png_fixed_digests.json was written by the host program as it was BEFORE the token sink and the dynamic route, in its
    five-argument form: the fixed route's bytes have not moved.  png_dynamic_digests.json holds this program's dynamic files;
    tests/test_gpu_png_dyn.py holds the kernels to the same table."""
    assert set(_golden("fixed")) == set(_golden("dynamic")) == set(D.DIGEST_CASES)
    assert {n: _digest(f[0]) for n, f in files.items()} == _golden("fixed")
    assert {n: _digest(f[1]) for n, f in files.items()} == _golden("dynamic")


@pytest.mark.parametrize("name", list(D.CASES))
def test_dynamic_file_decodes_and_every_block_is_the_smaller_type(name, files, host_check):
    img = D.case(name)
    h, w, _ = img.shape
    fixed, data = files[name]
    filters = P.check_png(data, img, S, limit=lib.raw().dvd_png_bound(h, w))
    P.check_png(fixed, img, S, limit=lib.raw().dvd_png_bound(h, w))
    assert len(data) <= len(fixed)
    blocks = D.parse_blocks(D.idat_of(data))
    nseg = -(-(h * (3 * w + 1)) // S)
    # per segment its block and the empty stored block, then the final empty fixed block
    assert [b["type"] for b in blocks[1::2]] == ["stored"] * nseg and len(blocks) == 2 * nseg + 1
    assert blocks[-1]["type"] == "fixed" and blocks[-1]["final"] == 1 and blocks[-1]["tokens"] == []
    assert all(b["final"] == 0 for b in blocks[:-1])
    fixed_blocks = D.parse_blocks(D.idat_of(fixed))
    assert [b["type"] for b in fixed_blocks[:-1:2]] == ["fixed"] * nseg
    code_lengths = lambda freq, limit: _lengths(host_check, freq, limit)  # noqa: E731
    for blk, was in zip(blocks[:-1:2], fixed_blocks[:-1:2]):
        assert blk["tokens"] == was["tokens"]                 # one tokeniser serves both routes
        as_fixed = D.fixed_price(blk["tokens"])
        assert was["bits"] == as_fixed
        if blk["type"] == "dynamic":
            assert blk["bits"] < as_fixed
            assert blk["bits"] == D.dynamic_price(blk["tokens"], code_lengths)
            ll, dd, _ = D.histograms(blk["tokens"])
            assert [k for k, n in enumerate(blk["ll_len"]) if n] == [k for k, f in enumerate(ll) if f]
            assert [k for k, n in enumerate(blk["d_len"]) if n] == [k for k, f in enumerate(dd) if f]
            assert D.kraft(blk["ll_len"]) == 1 << 15 and D.kraft(blk["cl_len"]) == 1 << 15
            assert sum(1 for f in dd if f) < 2 or D.kraft(blk["d_len"]) == 1 << 15
            assert blk["hlit"] == 257 or blk["ll_len"][-1] != 0
            assert blk["hdist"] == 1 or blk["d_len"][-1] != 0
            assert blk["hclen"] == 4 or blk["cl_len"][D.CL_ORDER[blk["hclen"] - 1]] != 0
            assert max(blk["cl_len"]) <= 7
        else:
            assert blk["type"] == "fixed" and blk["bits"] == as_fixed
            assert as_fixed <= D.dynamic_price(blk["tokens"], code_lengths)
    kinds = [b["type"] for b in blocks[:-1:2]]
    if name == "1x1":
        assert data == fixed and kinds == ["fixed"]
    if name == "zeros_256":
        assert len(data) < len(fixed) and "dynamic" in kinds
    if name == "7_segments_200x333":
        assert nseg == 7 or S != 32768
    if name == "deep":
        # the premises of the deep case, from the parsed file: Sub won, a block's histogram needs more than 15 levels
        # unconstrained, and that block's code is within 15 and complete (asserted for every dynamic block above)
        assert filters.tolist() == [1]
        deep = [b for b in blocks if b["type"] == "dynamic" and D.huffman_optimum(D.histograms(b["tokens"])[0])[1] > 15]
        assert deep and all(max(b["ll_len"]) <= 15 and D.kraft(b["ll_len"]) == 1 << 15 for b in deep)


def test_page_is_no_longer_than_pil_level_1(files):
    """The 700 x 500 page of benchmarks/png_time.py: the dynamic file against PIL's compress_level=1 (the measured ratios,
    level 6 included, are in DESIGN.md 4.4)."""
    from PIL import Image
    page = D.case("page_700x500")
    sizes = {}
    for level in (1, 6):
        buf = io.BytesIO()
        Image.fromarray(page).save(buf, format="PNG", compress_level=level)
        sizes[level] = len(buf.getvalue())
    fixed, data = files["page_700x500"]
    print(f"page 700 x 500: fixed {len(fixed)}, dynamic {len(data)}, PIL level 1 {sizes[1]} ({len(data) / sizes[1]:.3f}), "
          f"level 6 {sizes[6]} ({len(data) / sizes[6]:.3f})")
    assert len(data) <= sizes[1]


def test_png_kernels_use_no_scratch_and_the_dynamic_one_keeps_40_kb_of_lds(tmp_path):
    """hipcc's own metadata for gfx950: every kernel of png.hip has .private_segment_fixed_size 0, and png_compress_dyn_kernel
    declares the fixed route's 40 960 bytes of LDS (its tokens are in global scratch), four workgroups per CU."""
    import re
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "png.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "dvd_amd", "csrc", "png.hip")], check=True, stderr=subprocess.DEVNULL)
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1)))
    assert len(kernels) == 5 and all(scratch == 0 for scratch, _ in kernels.values()), kernels
    lds = {name: v[1] for name, v in kernels.items() if "png_compress" in name}
    assert len(lds) == 2 and set(lds.values()) == {40960}, lds


# ---- argument and env checks --------------------------------------------------------------------------------------------------
def test_bad_huffman_is_refused_without_a_gpu():
    raw = lib.raw()
    err = lambda: raw.dvd_last_error().decode()  # noqa: E731
    assert (lib.PNG_HUFFMAN_FIXED, lib.PNG_HUFFMAN_DYNAMIC) == (0, 1)
    fixed, dyn = raw.dvd_png_scratch_bytes_huff(97, 131, 0), raw.dvd_png_scratch_bytes_huff(97, 131, 1)
    assert fixed == raw.dvd_png_scratch_bytes(97, 131)
    assert dyn == fixed + 2 * S * (-(-(97 * (3 * 131 + 1)) // S))            # the tokens: 2 bytes per byte of a full segment
    for bad in (2, -1, 100):
        assert raw.dvd_png_scratch_bytes_huff(97, 131, bad) == -1 and "huffman" in err()
    assert raw.dvd_png_scratch_bytes_huff(0, 5, 1) == -1 and raw.dvd_png_scratch_bytes_huff(2 ** 31 - 1, 2 ** 31 - 1, 1) == -1
    fake = C.c_void_p(1 << 20)                     # never dereferenced: every check below fails before a launch
    bound = raw.dvd_png_bound(4, 4)
    for bad in (2, -1, 100):
        assert raw.dvd_png_encode_rgb8_huff(fake, 4, 4, fake, bound, fake, fake, bad, None) == -1 and "huffman" in err()
    for huff in (0, 1):
        assert raw.dvd_png_encode_rgb8_huff(fake, 4, 4, fake, bound - 1, fake, fake, huff, None) == -1 and "cap" in err()
        assert raw.dvd_png_encode_rgb8_huff(None, 4, 4, fake, bound, fake, fake, huff, None) == -1 and "null" in err()
        assert raw.dvd_png_encode_rgb8_huff(fake, 0, 4, fake, bound, fake, fake, huff, None) == -1 and "h >= 1" in err()
    good = torch.zeros(4, 5, 3, dtype=torch.uint8)
    for bad in ("best", "", None, 1, "Dynamic"):
        with pytest.raises(ValueError, match="'fixed' or 'dynamic'"):
            ops.png_encode(good, huffman=bad)
        with pytest.raises(ValueError, match="'fixed' or 'dynamic'"):
            ops.png_encode_to_file(good, "never_written.png", huffman=bad)
    assert not os.path.exists("never_written.png")
