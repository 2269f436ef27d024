"""CPU-side checks of the gradient-accumulation kernel's boundary, as tests/test_clip_abi.py does them: the header declares the entry
point and its three modes, the library exports it (detected by symbol: the version stays what it was, tests/test_scst_abi.py pins it),
gradaccum.hip is one of the sources, and every argument the header names as refused is refused before anything is launched (so no GPU is
needed to see it; the pointers are never followed on the host)."""
import ctypes
import os
import re

import pytest

from tests import accum_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, G, W, TI, TO, P = 4096, 8192, 16384 + 4, 32768 + 8, 65536 + 12, 131072 + 8     # well-formed "device pointers": buffers at 16 bytes, floats at 4, doubles at 8


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"int\s+mtn_grad_accum\s*\(\s*int\s+\w+\s*,\s*long\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*const\s+float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)
    for name, value in (("FIRST", R.FIRST), ("ADD", R.ADD), ("LAST", R.LAST)):
        assert re.search(r"#define\s+MTN_ACCUM_%s\s+%d\b" % (name, value), hdr)


def test_library_exports_the_entry_point():
    lib = _lib_or_build()
    Pt, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    assert lib.SYMBOLS["mtn_grad_accum"] == (I, [I, L, Pt, Pt, Pt, Pt, Pt, Pt, Pt])
    h = lib.load()
    assert h.mtn_grad_accum is not None
    assert h.mtn_version() >= 125
    assert "gradaccum.hip" in __import__("mtn_amd.build", fromlist=["SOURCES"]).SOURCES


BAD = [
    (3, 8, A, G, W, TI, TO, None), (-1, 8, A, G, W, TI, TO, None),                                    # an unknown mode
    (R.ADD, -1, A, G, W, TI, TO, None),                                                                 # n < 0
    (R.ADD, 8, None, G, W, TI, TO, None), (R.ADD, 8, A, None, W, TI, TO, None),                         # null acc / g
    (R.ADD, 8, A + 4, G, W, TI, TO, None), (R.ADD, 8, A, G + 8, W, TI, TO, None),                       # misaligned acc / g
    (R.FIRST, 8, A, G, None, None, TO, None), (R.ADD, 8, A, G, W + 2, TI, TO, None),                    # null / misaligned w
    (R.ADD, 8, A, G, W, TI + 1, TO, None), (R.ADD, 8, A, G, W, TI, TO + 2, None),                       # misaligned totals
    (R.FIRST, 8, A, G, W, None, None, None), (R.LAST, 8, A, G, W, TI, None, None),                      # null total_out
    (R.LAST, 8, A, G, W, TI, TO, P + 4),                                                                # misaligned partial
    (R.ADD, 8, A, A, W, TI, TO, None), (R.FIRST, 8, G, G, W, None, TO, None),                           # acc == g
    (R.ADD, 8, A, G, W, TI, TI, None), (R.LAST, 8, A, G, W, TO, TO, P), (R.FIRST, 8, A, G, W, TO, TO, None),   # total_in == total_out
    (R.ADD, 8, A, G, W, None, TO, None), (R.LAST, 8, A, G, W, None, TO, None),                          # total_in null outside FIRST
    (R.FIRST, 8, A, G, W, None, TO, P), (R.ADD, 8, A, G, W, TI, TO, P),                                 # partial outside LAST
    (R.ADD, 0, A, A, W, TI, TO, None), (R.LAST, 0, A, G, W, TI, TI, None),                              # refused at n == 0 too
]


@pytest.mark.parametrize("args", BAD, ids=str)
def test_refusals(args):
    h = _lib_or_build().load()
    assert h.mtn_grad_accum(*args, None) == 1             # MTN_ERR_ARG
    assert b"mtn_grad_accum" in h.mtn_last_error()


@pytest.mark.parametrize("mode", [R.FIRST, R.ADD, R.LAST])
def test_an_empty_buffer_is_ok_and_launches_nothing(mode):
    """n == 0 with well-formed arguments returns MTN_OK before any launch: no device is needed to see it."""
    h = _lib_or_build().load()
    assert h.mtn_grad_accum(mode, 0, A, G, W, None if mode == R.FIRST else TI, TO, P if mode == R.LAST else None, None) == 0
