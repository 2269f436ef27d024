"""CPU-side checks of the gradient-clipping kernels' boundary, as tests/test_average_abi.py does them: the header declares the three
entry points, the library exports them (detected by symbol: the version stays what it was, tests/test_scst_abi.py pins it),
gradnorm.hip is one of the sources, and every argument the header names as refused is refused before anything is launched (so no GPU is
needed to see it; the pointers are never followed on the host)."""
import ctypes
import os
import re

import pytest

from tests import clip_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, P, B, S, N, ST = 4096, 8192, 16384 + 4, 32768 + 8, 65536 + 8, 131072      # well-formed "device pointers": g at 16 bytes, doubles at 8, floats at 4
NAN, INF = float("nan"), float("inf")


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"int\s+mtn_grad_sumsq_partials\s*\(\s*long\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_grad_sumsq\s*\(\s*long\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_clip_scale\s*\(\s*int\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*float\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)


def test_library_exports_the_entry_points():
    lib = _lib_or_build()
    Pt, F, L, I = ctypes.c_void_p, ctypes.c_float, ctypes.c_long, ctypes.c_int
    assert lib.SYMBOLS["mtn_grad_sumsq_partials"] == (I, [L])
    assert lib.SYMBOLS["mtn_grad_sumsq"] == (I, [L, Pt, Pt, Pt])
    assert lib.SYMBOLS["mtn_clip_scale"] == (I, [I, Pt, F, Pt, Pt, Pt, Pt, Pt])
    h = lib.load()
    assert h.mtn_grad_sumsq_partials is not None and h.mtn_grad_sumsq is not None and h.mtn_clip_scale is not None
    assert h.mtn_version() >= 125
    assert "gradnorm.hip" in __import__("mtn_amd.build", fromlist=["SOURCES"]).SOURCES


SUMSQ_BAD = [(0, G, P), (-1, G, P), (8, None, P), (8, G, None), (8, G + 4, P), (8, G + 8, P), (8, G, P + 4), (8, G, P + 1)]
SCALE_BAD = [(0, P, 1.0, B, S, N, ST), (-3, P, 1.0, B, S, N, ST), (R.GRID_CAP + 1, P, 1.0, B, S, N, ST),
             (4, None, 1.0, B, S, N, ST), (4, P + 4, 1.0, B, S, N, ST),
             (4, P, 0.0, B, S, N, ST), (4, P, -1.0, B, S, N, ST), (4, P, NAN, B, S, N, ST), (4, P, -INF, B, S, N, ST),
             (4, P, 1.0, B + 2, S, N, ST), (4, P, 1.0, B, None, N, ST), (4, P, 1.0, B, S + 1, N, ST), (4, P, 1.0, B, S + 2, N, ST),
             (4, P, 1.0, B, S, N + 4, ST), (4, P, 1.0, B, S, N, ST + 4), (4, P, 1.0, None, None, None, None)]


@pytest.mark.parametrize("args", SUMSQ_BAD, ids=str)
def test_grad_sumsq_refusals(args):
    h = _lib_or_build().load()
    assert h.mtn_grad_sumsq(*args, None) == 1             # MTN_ERR_ARG
    assert b"mtn_grad_sumsq" in h.mtn_last_error()


@pytest.mark.parametrize("args", SCALE_BAD, ids=str)
def test_clip_scale_refusals(args):
    h = _lib_or_build().load()
    assert h.mtn_clip_scale(*args, None) == 1
    assert b"mtn_clip_scale" in h.mtn_last_error()


def test_partials_is_monotone_capped_and_the_reference():
    h = _lib_or_build().load()
    ns = [-5, 0, 1, 3, 4, 1023, 1024, 1025, 2048, 2049, 10 ** 5, R.CAP_ELEMS - 1024, R.CAP_ELEMS - 1, R.CAP_ELEMS, R.CAP_ELEMS + 5,
          3 * 2 ** 20 + 7, 10 ** 9, 2 ** 40]
    got = [h.mtn_grad_sumsq_partials(n) for n in ns]
    assert got == [R.partials(n) for n in ns]
    assert got == sorted(got) and got[0] == got[1] == 0 and got[2] == 1 and max(got) == got[-1] == R.GRID_CAP == 2048
