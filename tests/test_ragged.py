"""CPU-side checks of the ragged (one size per document) batch entry points dvd_unwarp_u8_ragged / dvd_ingest_u8_ragged:
the header declares them, dvd_amd.lib binds them, and they check every argument BEFORE any HIP call - so, like
tests/test_abi.py::test_argument_validation_without_gpu, these run with no device (pointers are never followed)."""
import ctypes as C
import os
import re

import pytest

from dvd_amd import lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCALE = C.c_float(0.987)
PTR = 0x1000          # a non-null "device pointer": rejected calls and n == 0 never follow it


def table(*shapes, src=PTR, out=PTR):
    tab = (lib.RaggedImage * max(len(shapes), 1))()
    for d, (h, w) in enumerate(shapes):
        tab[d].src, tab[d].out, tab[d].h, tab[d].w = src, out, h, w
    return tab


def last_error():
    return lib.raw().dvd_last_error().decode()


def test_header_declares_and_lib_binds_the_ragged_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvd_hip.h")).read(), flags=re.S)
    for name in ("dvd_unwarp_u8_ragged", "dvd_ingest_u8_ragged", "dvd_ingest_ragged_scratch_bytes"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in lib.SIGNATURES
        assert getattr(lib.raw(), name).argtypes == lib.SIGNATURES[name]
    assert "dvd_ragged_image" in text
    cap = int(re.search(r"#define\s+DVD_RAGGED_CAP\s+(\d+)", text).group(1))
    assert cap == lib.RAGGED_CAP and cap >= 1
    assert C.sizeof(lib.RaggedImage) == 24                                   # two pointers + two ints, as the header's struct
    assert lib.raw().dvd_ingest_ragged_scratch_bytes.restype is C.c_long
    assert lib.raw().dvd_ingest_ragged_scratch_bytes(512, 32) == 32 * lib.raw().dvd_ingest_scratch_bytes(512)
    assert lib.raw().dvd_ingest_ragged_scratch_bytes(512, 0) == 0


@pytest.mark.parametrize("what, args", [
    ("null flow", lambda: (None, 16, table((4, 4)), 1)),
    ("null table", lambda: (PTR, 16, None, 1)),
    ("null src", lambda: (PTR, 16, table((4, 4), src=None), 1)),
    ("null out", lambda: (PTR, 16, table((4, 4), out=None), 1)),
    ("h = 0", lambda: (PTR, 16, table((4, 4), (0, 4)), 2)),
    ("w = 0", lambda: (PTR, 16, table((4, 0)), 1)),
    ("h = 65536", lambda: (PTR, 16, table((4, 4), (65536, 4)), 2)),
    ("n < 0", lambda: (PTR, 16, table((4, 4)), -1)),
    ("g < 2", lambda: (PTR, 1, table((4, 4)), 1)),
])
def test_unwarp_u8_ragged_rejects_bad_arguments_before_any_launch(what, args):
    flow, g, tab, n = args()
    rc = lib.raw().dvd_unwarp_u8_ragged(flow, g, tab, n, SCALE, None)
    assert rc == -1, what
    assert "unwarp_u8_ragged" in last_error(), what


def test_unwarp_u8_ragged_accepts_an_empty_batch():
    assert lib.raw().dvd_unwarp_u8_ragged(PTR, 16, table(), 0, SCALE, None) == 0


@pytest.mark.parametrize("what, args", [
    ("null table", lambda: (None, 1, 0, PTR, 16, PTR)),
    ("null y", lambda: (table((4, 4)), 1, 0, None, 16, PTR)),
    ("null scratch", lambda: (table((4, 4)), 1, 0, PTR, 16, None)),
    ("null src", lambda: (table((4, 4), src=None), 1, 0, PTR, 16, PTR)),
    ("h = 0", lambda: (table((4, 4), (0, 4)), 2, 0, PTR, 16, PTR)),
    ("w = 0", lambda: (table((4, 0)), 1, 0, PTR, 16, PTR)),
    ("h = 65536", lambda: (table((65536, 4)), 1, 0, PTR, 16, PTR)),
    ("n < 0", lambda: (table((4, 4)), -1, 0, PTR, 16, PTR)),
    ("out_size = 0", lambda: (table((4, 4)), 1, 0, PTR, 0, PTR)),
    ("swap in place", lambda: (table((4, 4)), 1, 1, PTR, 16, PTR)),
])
def test_ingest_u8_ragged_rejects_bad_arguments_before_any_launch(what, args):
    tab, n, swap, y, out_size, scratch = args()
    rc = lib.raw().dvd_ingest_u8_ragged(tab, n, swap, y, out_size, scratch, None)
    assert rc == -1, what
    assert "ingest_u8_ragged" in last_error(), what


def test_ingest_u8_ragged_accepts_an_empty_batch():
    assert lib.raw().dvd_ingest_u8_ragged(table(), 0, 0, PTR, 16, PTR, None) == 0
    # the RGB copy is optional: a null `out` is not an argument error (checked with n = 0 entries after it only)
    assert lib.raw().dvd_ingest_u8_ragged(table((4, 4), out=None), 0, 0, PTR, 16, PTR, None) == 0
