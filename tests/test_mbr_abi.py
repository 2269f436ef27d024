"""CPU-side checks of the minimum-Bayes-risk selection's boundary, as tests/test_diverse_abi.py does them: the ctypes mirror of
mtn_mbr_args has the C struct's size and field offsets, the library exports the entry point at version >= 121, and every argument the
header names as refused is refused before anything is launched (so no GPU is needed to see it)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["sets", "K", "L", "N", "ldl", "tok", "len", "n_hyp", "w", "log_tok", "eos", "expected", "best", "order", "util"]


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_mbr_args_layout_matches_c(tmp_path):
    lib = _lib_or_build()
    src = tmp_path / "sz.c"
    offs = ", ".join("offsetof(mtn_mbr_args, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){size_t v[] = {sizeof(mtn_mbr_args), MTN_MBR_MAX_HYP, %s};\n'
                   'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);\nreturn 0;}\n' % offs)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    from mtn_amd import ops
    assert sizes == [ctypes.sizeof(lib.MbrArgs), ops.MBR_MAX_HYP] + [getattr(lib.MbrArgs, f).offset for f in FIELDS]
    assert [f for f, _ in lib.MbrArgs._fields_] == FIELDS


def test_library_exports_the_entry_point():
    lib = _lib_or_build()
    assert "mtn_mbr_select" in lib.SYMBOLS
    h = lib.load()
    assert h.mtn_mbr_select is not None and h.mtn_version() >= 121


def _args(lib, **kw):
    """A well-formed explicit-source block (the pointers are never followed on the host), then ``kw`` over it."""
    a = lib.MbrArgs()
    a.sets, a.K, a.L, a.N, a.ldl = 2, 4, 10, 2, 10
    a.tok, a.len, a.n_hyp, a.expected, a.best, a.order = 64, 128, 192, 256, 320, 384
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw", [
    dict(expected=None), dict(best=None), dict(order=None),                     # a null required buffer
    dict(len=None), dict(n_hyp=None),                                            # ... of the explicit source
    dict(tok=None),                                                              # no source at all: tok and log_tok both null
    dict(K=0), dict(K=17), dict(K=-1),
    dict(L=0), dict(L=129), dict(ldl=129, L=129),
    dict(N=0), dict(N=5),
    dict(ldl=9),                                                                 # ldl < L
    dict(sets=0), dict(sets=-3),
], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_bad_arguments_are_refused_before_any_launch(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_mbr_select(ctypes.byref(_args(lib, **kw)), None) == 1           # MTN_ERR_ARG
    assert b"mtn_mbr_select" in h.mtn_last_error()


def test_null_argument_block_is_refused():
    lib = _lib_or_build()
    assert lib.load().mtn_mbr_select(None, None) == 1
