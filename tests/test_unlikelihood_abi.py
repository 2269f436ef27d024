"""CPU-side checks of the unlikelihood loss head's boundary, as tests/test_scst_abi.py does them: the header declares the two entries, the
ctypes mirror has the C struct's size and field offsets (mtn_losshead_args is the prefix of mtn_ulosshead_args), the library exports them
(detected by symbol: the version stays what it was), and every argument the header names as refused is refused before anything is launched
(so no GPU is needed to see it)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_FIELDS = ["n_seg", "rows", "target", "norm", "coef", "V", "ldz", "pad", "smoothing", "logits", "lse", "rowloss", "gloss", "dlogits", "ldd"]
UL_FIELDS = HEAD_FIELDS + ["seq_len", "ul_alpha", "rowul"]
ENTRIES = ["mtn_ulosshead_fwd", "mtn_ulosshead_bwd"]


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _ids(kw):
    return ",".join("%s=%s" % i for i in kw.items())


def _header():
    return open(os.path.join(ROOT, "include", "mtn_hip.h")).read()


def test_header_declares_the_entries():
    hdr = _header()
    assert re.search(r"int\s+mtn_ulosshead_fwd\s*\(\s*const\s+mtn_ulosshead_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_ulosshead_bwd\s*\(\s*int\s+\w+\s*,\s*const\s+mtn_ulosshead_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)
    assert re.search(r"#define\s+MTN_UL_CLAMP\s+1e-5f", hdr)
    m = re.search(r"#define\s+MTN_ULOSSHEAD_MAX_V\s+(\d+)", hdr)
    assert m and int(m.group(1)) >= 32768                              # the bound on V is stated, and no smaller than this


def test_struct_layout_matches_c(tmp_path):
    lib = _lib_or_build()
    exprs = ["sizeof(mtn_ulosshead_args)"] + ["offsetof(mtn_ulosshead_args, %s)" % f for f in UL_FIELDS]
    exprs += ["sizeof(mtn_losshead_args)"] + ["offsetof(mtn_losshead_args, %s)" % f for f in HEAD_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){size_t v[] = {%s};\n'
                   'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);\nreturn 0;}\n' % ", ".join(exprs))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    U, H = lib.ULossHeadArgs, lib.LossHeadArgs
    assert [f for f, _ in U._fields_] == UL_FIELDS
    mine = [ctypes.sizeof(U)] + [getattr(U, f).offset for f in UL_FIELDS] + [ctypes.sizeof(H)] + [getattr(H, f).offset for f in HEAD_FIELDS]
    assert sizes == mine
    assert [getattr(H, f).offset for f in HEAD_FIELDS] == [getattr(U, f).offset for f in HEAD_FIELDS]      # the loss head's block is the prefix


def test_library_exports_the_entry_points():
    lib = _lib_or_build()
    h = lib.load()
    for name in ENTRIES:
        assert name in lib.SYMBOLS and getattr(h, name) is not None
    assert lib.SYMBOLS["mtn_ulosshead_fwd"][1][0] == ctypes.POINTER(lib.ULossHeadArgs)
    assert lib.SYMBOLS["mtn_ulosshead_bwd"][1][:2] == [ctypes.c_int, ctypes.POINTER(lib.ULossHeadArgs)]


def _head(lib, **kw):
    """A well-formed block (the pointers are never followed on the host), then ``kw`` over it."""
    a = lib.ULossHeadArgs()
    a.n_seg = 2
    for s in range(2):
        a.rows[s], a.target[s], a.norm[s], a.coef[s], a.seq_len[s] = 6, 64 * (s + 1), 1024 + 64 * s, 1.0, (3, 0)[s]
    a.V, a.ldz, a.pad, a.smoothing, a.ldd = 104, 104, 1, 0.1, 104
    a.logits, a.lse, a.rowloss, a.gloss, a.dlogits = 2048, 4096, 8192, 16384, 32768
    a.ul_alpha, a.rowul = 0.5, 65536
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def _max_v():
    return int(re.search(r"#define\s+MTN_ULOSSHEAD_MAX_V\s+(\d+)", _header()).group(1))


HEAD_BAD = [
    dict(ul_alpha=-0.5), dict(ul_alpha=float("nan")), dict(ul_alpha=float("inf")), dict(seq_len=(0, -1)), dict(seq_len=(1, -3)),
    dict(seq_len=(0, 4)), dict(seq_len=(1, 5)), dict(seq_len=(0, 7)),
    dict(V=102), dict(V=0), dict(n_seg=5), dict(n_seg=0), dict(rows=(1, 0)), dict(ldz=100), dict(pad=104), dict(pad=-1),
    dict(logits=None), dict(lse=None), dict(target=(1, None)), dict(norm=(0, None)),
]


@pytest.mark.parametrize("kw", HEAD_BAD, ids=_ids)
def test_unlikelihood_head_refuses_bad_arguments_before_any_launch(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_ulosshead_fwd(ctypes.byref(_head(lib, **kw)), None) == 1           # MTN_ERR_ARG
    assert b"mtn_ulosshead_fwd" in h.mtn_last_error()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_ulosshead_bwd(code, ctypes.byref(_head(lib, **kw)), None) == 1
        assert b"mtn_ulosshead_bwd" in h.mtn_last_error()


def test_a_vocabulary_above_the_stated_bound_is_refused():
    lib = _lib_or_build()
    h = lib.load()
    V = _max_v() + 4
    kw = dict(V=V, ldz=V, ldd=V)
    assert h.mtn_ulosshead_fwd(ctypes.byref(_head(lib, **kw)), None) == 1
    assert b"mtn_ulosshead_fwd" in h.mtn_last_error() and b"MTN_ULOSSHEAD_MAX_V" in h.mtn_last_error()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_ulosshead_bwd(code, ctypes.byref(_head(lib, **kw)), None) == 1
        assert b"mtn_ulosshead_bwd" in h.mtn_last_error()


@pytest.mark.parametrize("kw", [dict(ldd=100), dict(ldd=106), dict(gloss=None), dict(dlogits=None)], ids=_ids)
def test_unlikelihood_head_refuses_bad_backward_arguments(kw):
    lib = _lib_or_build()
    h = lib.load()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_ulosshead_bwd(code, ctypes.byref(_head(lib, **kw)), None) == 1
        assert b"mtn_ulosshead_bwd" in h.mtn_last_error()
    assert h.mtn_ulosshead_bwd(7, ctypes.byref(_head(lib)), None) == 1              # a dtype code that does not exist
    assert h.mtn_ulosshead_fwd(ctypes.byref(_head(lib, rowloss=None)), None) == 1
    assert h.mtn_ulosshead_fwd(None, None) == 1 and h.mtn_ulosshead_bwd(0, None, None) == 1


def test_sequence_lengths_past_n_seg_are_not_looked_at():
    """Segments 2 and 3 do not exist in the well-formed block: a bad seq_len there changes nothing — the refusal is that of the last
    segment's rows, which the walk over the segments reaches last."""
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_ulosshead_fwd(ctypes.byref(_head(lib, seq_len=(3, -5), rows=(1, 0))), None) == 1
    assert b"bad segment" in h.mtn_last_error()
    assert h.mtn_ulosshead_bwd(lib.MTN_BF16, ctypes.byref(_head(lib, seq_len=(2, 7), rows=(1, 0))), None) == 1
    assert b"bad segment" in h.mtn_last_error()
