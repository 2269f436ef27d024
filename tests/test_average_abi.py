"""CPU-side checks of the weight-averaging kernels' boundary, as tests/test_distill_abi.py does them: the header declares the three entry
points, the library exports them at version >= 124, and every argument the header names as refused is refused before anything is
launched (so no GPU is needed to see it; the pointers are never followed on the host)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, S, CO = 4096, 8192, 16384, 32768 + 4          # well-formed "device pointers": 16-byte aligned buffers, a state block, a float
NAN, INF = float("nan"), float("inf")


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"int\s+mtn_lerp_f32\s*\(\s*long\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_ema_step\s*\(\s*long\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*float\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_swap_f32\s*\(\s*long\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)


def test_library_exports_the_entry_points():
    lib = _lib_or_build()
    P, F, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_long
    assert lib.SYMBOLS["mtn_lerp_f32"] == (ctypes.c_int, [L, P, P, F, P])
    assert lib.SYMBOLS["mtn_ema_step"] == (ctypes.c_int, [L, P, P, P, F, P, P])
    assert lib.SYMBOLS["mtn_swap_f32"] == (ctypes.c_int, [L, P, P, P])
    h = lib.load()
    assert h.mtn_lerp_f32 is not None and h.mtn_ema_step is not None and h.mtn_swap_f32 is not None
    assert h.mtn_version() >= 124
    assert "average.hip" in __import__("mtn_amd.build", fromlist=["SOURCES"]).SOURCES


LERP_BAD = [(-1, A, B, 0.5), (8, None, B, 0.5), (8, A, None, 0.5), (8, A + 4, B, 0.5), (8, A, B + 8, 0.5), (8, A, A, 0.5),
            (8, A, B, -0.01), (8, A, B, 1.01), (8, A, B, NAN), (8, A, B, INF), (8, A, B, -INF)]
EMA_BAD = [(-1, A, B, S, 0.9, CO), (8, None, B, S, 0.9, CO), (8, A, None, S, 0.9, CO), (8, A, B, None, 0.9, CO), (8, A + 4, B, S, 0.9, CO),
           (8, A, B + 12, S, 0.9, CO), (8, A, B, S + 2, 0.9, CO), (8, A, B, S, 0.9, CO + 1), (8, A, A, S, 0.9, None),
           (8, A, B, S, 1.0, None), (8, A, B, S, -0.1, None), (8, A, B, S, 1.5, None), (8, A, B, S, NAN, None), (8, A, B, S, INF, None)]
SWAP_BAD = [(-1, A, B), (8, None, B), (8, A, None), (8, A + 8, B), (8, A, B + 4), (8, A, A)]


@pytest.mark.parametrize("args", LERP_BAD, ids=str)
def test_lerp_refusals(args):
    h = _lib_or_build().load()
    assert h.mtn_lerp_f32(*args, None) == 1               # MTN_ERR_ARG
    assert b"mtn_lerp_f32" in h.mtn_last_error()


@pytest.mark.parametrize("args", EMA_BAD, ids=str)
def test_ema_step_refusals(args):
    h = _lib_or_build().load()
    assert h.mtn_ema_step(*args, None) == 1
    assert b"mtn_ema_step" in h.mtn_last_error()


@pytest.mark.parametrize("args", SWAP_BAD, ids=str)
def test_swap_refusals(args):
    h = _lib_or_build().load()
    assert h.mtn_swap_f32(*args, None) == 1
    assert b"mtn_swap_f32" in h.mtn_last_error()


def test_an_empty_range_is_ok_and_launches_nothing():
    """n == 0 with well-formed arguments returns MTN_OK on a machine without a GPU: a launch there would fail (MTN_ERR_LAUNCH)."""
    h = _lib_or_build().load()
    assert h.mtn_lerp_f32(0, A, B, 0.5, None) == 0
    assert h.mtn_lerp_f32(0, A, B, 0.0, None) == 0 and h.mtn_lerp_f32(0, A, B, 1.0, None) == 0      # the interval's ends are inside
    assert h.mtn_ema_step(0, A, B, S, 0.9, None, None) == 0 and h.mtn_ema_step(0, A, B, S, 0.0, CO, None) == 0
    assert h.mtn_swap_f32(0, A, B, None) == 0
