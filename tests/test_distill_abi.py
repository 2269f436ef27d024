"""CPU-side checks of the distillation loss head's boundary, as tests/test_mbr_abi.py does them: the header declares both entry points,
the ctypes mirror of mtn_distill_args has the C struct's size and field offsets (and mtn_losshead_args as its prefix), the library
exports the entries at version >= 123, and every argument the header names as refused is refused before anything is launched (so no
GPU is needed to see it)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_FIELDS = ["n_seg", "rows", "target", "norm", "coef", "V", "ldz", "pad", "smoothing", "logits", "lse", "rowloss", "gloss", "dlogits", "ldd"]
FIELDS = HEAD_FIELDS + ["teacher", "ldq", "alpha", "temperature", "rowkd"]


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_header_declares_both_entries():
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"int\s+mtn_distill_fwd\s*\(\s*const\s+mtn_distill_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_distill_bwd\s*\(\s*int\s+\w+\s*,\s*const\s+mtn_distill_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)


def test_distill_args_layout_matches_c(tmp_path):
    lib = _lib_or_build()
    src = tmp_path / "sz.c"
    offs = ", ".join("offsetof(mtn_distill_args, %s)" % f for f in FIELDS)
    head = ", ".join("offsetof(mtn_losshead_args, %s)" % f for f in HEAD_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){size_t v[] = {sizeof(mtn_distill_args), sizeof(mtn_losshead_args), '
                   'MTN_LOSSHEAD_MAX_SEG, %s, %s};\nfor (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);\nreturn 0;}\n' % (offs, head))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D, H = lib.DistillHeadArgs, lib.LossHeadArgs
    assert sizes == ([ctypes.sizeof(D), ctypes.sizeof(H), 4] + [getattr(D, f).offset for f in FIELDS] + [getattr(H, f).offset for f in HEAD_FIELDS])
    assert [f for f, _ in D._fields_] == FIELDS
    assert [getattr(D, f).offset for f in HEAD_FIELDS] == [getattr(H, f).offset for f in HEAD_FIELDS]      # the loss head's block is the prefix


def test_library_exports_the_entry_points():
    lib = _lib_or_build()
    assert "mtn_distill_fwd" in lib.SYMBOLS and "mtn_distill_bwd" in lib.SYMBOLS
    assert lib.SYMBOLS["mtn_distill_fwd"][1][0] == ctypes.POINTER(lib.DistillHeadArgs)
    assert lib.SYMBOLS["mtn_distill_bwd"][1][:2] == [ctypes.c_int, ctypes.POINTER(lib.DistillHeadArgs)]
    h = lib.load()
    assert h.mtn_distill_fwd is not None and h.mtn_distill_bwd is not None and h.mtn_version() >= 123


def _args(lib, **kw):
    """A well-formed block (the pointers are never followed on the host), then ``kw`` over it."""
    a = lib.DistillHeadArgs()
    a.n_seg = 2
    for s in range(2):
        a.rows[s], a.target[s], a.norm[s], a.coef[s] = 3, 64 * (s + 1), 1024 + 64 * s, 1.0
    a.V, a.ldz, a.pad, a.smoothing, a.ldd = 104, 104, 1, 0.1, 104
    a.logits, a.lse, a.rowloss, a.gloss, a.dlogits, a.rowkd = 2048, 4096, 8192, 16384, 32768, 65536
    a.teacher[0], a.ldq[0] = 131072, 104
    a.alpha, a.temperature = 0.5, 2.0
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


BAD = [
    dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=float("inf")),
    dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
    dict(ldq=(0, 100)), dict(ldq=(0, 106)), dict(teacher=(0, 131072 + 4)),
    dict(V=102), dict(V=0), dict(n_seg=5), dict(n_seg=0), dict(rows=(1, 0)), dict(ldz=100), dict(pad=104), dict(pad=-1),
    dict(logits=None), dict(lse=None), dict(target=(1, None)), dict(norm=(0, None)),
]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_bad_arguments_are_refused_before_any_launch(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_distill_fwd(ctypes.byref(_args(lib, **kw)), None) == 1           # MTN_ERR_ARG
    assert b"mtn_distill_fwd" in h.mtn_last_error()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_distill_bwd(code, ctypes.byref(_args(lib, **kw)), None) == 1
        assert b"mtn_distill_bwd" in h.mtn_last_error()


@pytest.mark.parametrize("kw", [dict(ldd=100), dict(ldd=106), dict(gloss=None), dict(dlogits=None)], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_bad_backward_arguments_are_refused(kw):
    lib = _lib_or_build()
    h = lib.load()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_distill_bwd(code, ctypes.byref(_args(lib, **kw)), None) == 1
    assert h.mtn_distill_bwd(7, ctypes.byref(_args(lib)), None) == 1              # a dtype code that does not exist
    assert h.mtn_distill_fwd(ctypes.byref(_args(lib, rowloss=None)), None) == 1


def test_a_segment_without_teacher_ignores_its_ldq():
    """ldq is checked only where a teacher is given: segment 1 has none and ldq[1] = 0 in the well-formed block, and a bad ldq[1]
    changes nothing — the refusal below comes from alpha alone."""
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_distill_fwd(ctypes.byref(_args(lib, ldq=(1, 3), alpha=2.0)), None) == 1
    assert b"alpha" in h.mtn_last_error()


def test_null_argument_block_is_refused():
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_distill_fwd(None, None) == 1 and h.mtn_distill_bwd(0, None, None) == 1
