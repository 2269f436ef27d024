"""CPU-side checks of the corpus-metrics boundary, as tests/test_mbr_abi.py does them: the ctypes mirror of mtn_eval_args has the C struct's
size and field offsets, the library exports the entry points at version >= 122, the workspace size follows the stated rule, and every
argument the header names as refused is refused before anything is launched (so no GPU is needed to see it)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["Q", "R", "L", "ldl", "hyp", "hyp_len", "ref", "ref_len", "n_ref", "workspace", "workspace_bytes", "stats", "rouge", "cider",
          "corpus", "df_of_ref"]


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_eval_args_layout_matches_c(tmp_path):
    lib = _lib_or_build()
    src = tmp_path / "sz.c"
    offs = ", ".join("offsetof(mtn_eval_args, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){size_t v[] = {sizeof(mtn_eval_args), MTN_EVAL_MAX_REF, %s};\n'
                   'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);\nreturn 0;}\n' % offs)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    from mtn_amd import ops
    assert sizes == [ctypes.sizeof(lib.EvalArgs), ops.EVAL_MAX_REF] + [getattr(lib.EvalArgs, f).offset for f in FIELDS]
    assert [f for f, _ in lib.EvalArgs._fields_] == FIELDS


def test_library_exports_the_entry_points():
    lib = _lib_or_build()
    assert "mtn_eval_metrics" in lib.SYMBOLS and "mtn_eval_workspace_bytes" in lib.SYMBOLS
    h = lib.load()
    assert h.mtn_eval_metrics is not None and h.mtn_eval_workspace_bytes is not None and h.mtn_version() >= 122


@pytest.mark.parametrize("Q,R,L", [(1, 1, 1), (2, 4, 10), (300, 1, 30), (64, 1, 128), (1710, 8, 128), (5, 3, 77)])
def test_workspace_holds_a_power_of_two_table_of_twice_four_slots_per_token(Q, R, L):
    h = _lib_or_build().load()
    b = h.mtn_eval_workspace_bytes(Q, R, L)
    slots = b // 8                                                             # a 32-bit key and a 32-bit count per slot
    assert b % 16 == 0 and slots & (slots - 1) == 0 and slots >= 2 * 4 * Q * R * L
    assert slots == 1024 or slots < 2 * (2 * 4 * Q * R * L)                    # ... and the smallest such (above a floor of 1024 slots)


def test_workspace_of_refused_sizes_is_zero():
    h = _lib_or_build().load()
    for Q, R, L in [(0, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, 129), (2 ** 22, 8, 128)]:
        assert h.mtn_eval_workspace_bytes(Q, R, L) == 0


def _args(lib, **kw):
    """A well-formed block (the pointers are never followed on the host), then ``kw`` over it."""
    a = lib.EvalArgs()
    a.Q, a.R, a.L, a.ldl = 2, 4, 10, 10
    a.hyp, a.hyp_len, a.ref, a.ref_len, a.n_ref = 64, 128, 192, 256, 320
    a.workspace, a.workspace_bytes = 4096, lib.load().mtn_eval_workspace_bytes(2, 4, 10)
    a.stats, a.rouge, a.cider, a.corpus = 384, 448, 512, 576
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw", [
    dict(hyp=None), dict(hyp_len=None), dict(ref=None), dict(ref_len=None), dict(n_ref=None),       # a null required buffer
    dict(stats=None), dict(rouge=None), dict(cider=None), dict(corpus=None), dict(workspace=None),
    dict(Q=0), dict(Q=-3),
    dict(R=0), dict(R=9), dict(R=-1),
    dict(L=0), dict(L=129), dict(ldl=129, L=129), dict(L=-1),
    dict(ldl=9),                                                                 # ldl < L
    dict(workspace_bytes=0), dict(workspace_bytes=8191),                         # one byte short of the 1024-slot floor
    dict(Q=200, workspace_bytes=8192),                                           # enough for the block above, not for 200 items
    dict(workspace=4100),                                                        # not 16-byte aligned
], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_bad_arguments_are_refused_before_any_launch(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert _args(lib).workspace_bytes == 8192
    assert h.mtn_eval_metrics(ctypes.byref(_args(lib, **kw)), None) == 1         # MTN_ERR_ARG
    assert b"mtn_eval_metrics" in h.mtn_last_error()


def test_null_argument_block_is_refused():
    lib = _lib_or_build()
    assert lib.load().mtn_eval_metrics(None, None) == 1
