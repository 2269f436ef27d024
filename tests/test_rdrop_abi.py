"""CPU-side checks of the paired (R-Drop) loss head's boundary, as tests/test_unlikelihood_abi.py does them: the header declares the two
entries, the ctypes mirror has the C struct's size and field offsets (mtn_losshead_args is the prefix of mtn_rlosshead_args), the library
exports them (detected by symbol: the version stays what it was), and every argument the header names as refused is refused before
anything is launched (so no GPU is needed to see it)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_FIELDS = ["n_seg", "rows", "target", "norm", "coef", "V", "ldz", "pad", "smoothing", "logits", "lse", "rowloss", "gloss", "dlogits", "ldd"]
RD_FIELDS = HEAD_FIELDS + ["pair", "rd_alpha", "rowrd", "rowkl"]
ENTRIES = ["mtn_rlosshead_fwd", "mtn_rlosshead_bwd"]


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
    assert re.search(r"int\s+mtn_rlosshead_fwd\s*\(\s*const\s+mtn_rlosshead_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_rlosshead_bwd\s*\(\s*int\s+\w+\s*,\s*const\s+mtn_rlosshead_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)
    m = re.search(r"typedef struct \{([^}]*)\}\s*mtn_rlosshead_args\s*;", hdr)
    assert m
    body = m.group(1)
    assert re.search(r"int\s+pair\s*\[\s*MTN_LOSSHEAD_MAX_SEG\s*\]\s*;", body) and re.search(r"float\s+rd_alpha\s*;", body)
    assert re.search(r"float\s*\*\s*rowrd\s*;", body) and re.search(r"float\s*\*\s*rowkl\s*;", body)


def test_the_version_stays_what_it_was():
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_version() == 125 and all(getattr(h, name, None) is not None for name in ENTRIES)


def test_struct_layout_matches_c(tmp_path):
    lib = _lib_or_build()
    exprs = ["sizeof(mtn_rlosshead_args)"] + ["offsetof(mtn_rlosshead_args, %s)" % f for f in RD_FIELDS]
    exprs += ["sizeof(mtn_losshead_args)"] + ["offsetof(mtn_losshead_args, %s)" % f for f in HEAD_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){size_t v[] = {%s};\n'
                   'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);\nreturn 0;}\n' % ", ".join(exprs))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R, H = lib.RLossHeadArgs, lib.LossHeadArgs
    assert [f for f, _ in R._fields_] == RD_FIELDS
    mine = [ctypes.sizeof(R)] + [getattr(R, f).offset for f in RD_FIELDS] + [ctypes.sizeof(H)] + [getattr(H, f).offset for f in HEAD_FIELDS]
    assert sizes == mine
    assert [getattr(H, f).offset for f in HEAD_FIELDS] == [getattr(R, f).offset for f in HEAD_FIELDS]      # the loss head's block is the prefix


def test_library_exports_the_entry_points():
    lib = _lib_or_build()
    h = lib.load()
    for name in ENTRIES:
        assert name in lib.SYMBOLS and getattr(h, name) is not None
    assert lib.SYMBOLS["mtn_rlosshead_fwd"][1][0] == ctypes.POINTER(lib.RLossHeadArgs)
    assert lib.SYMBOLS["mtn_rlosshead_bwd"][1][:2] == [ctypes.c_int, ctypes.POINTER(lib.RLossHeadArgs)]


def _head(lib, **kw):
    """A well-formed block (the pointers are never followed on the host), then ``kw`` over it."""
    a = lib.RLossHeadArgs()
    a.n_seg = 2
    for s in range(2):
        a.rows[s], a.target[s], a.norm[s], a.coef[s], a.pair[s] = 6, 64 * (s + 1), 1024 + 64 * s, 1.0, (3, 0)[s]
    a.V, a.ldz, a.pad, a.smoothing, a.ldd = 104, 104, 1, 0.1, 104
    a.logits, a.lse, a.rowloss, a.gloss, a.dlogits = 2048, 4096, 8192, 16384, 32768
    a.rd_alpha, a.rowrd, a.rowkl = 0.5, 65536, 131072
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


HEAD_BAD = [
    dict(rd_alpha=-0.5), dict(rd_alpha=float("nan")), dict(rd_alpha=float("inf")), dict(pair=(0, -1)), dict(pair=(1, -3)),
    dict(pair=(0, 2)), dict(pair=(0, 6)), dict(pair=(1, 6)), dict(pair=(1, 2)), dict(rows=(0, 7)), dict(rowkl=None),
    dict(V=102), dict(V=0), dict(n_seg=5), dict(n_seg=0), dict(rows=(1, 0)), dict(ldz=100), dict(pad=104), dict(pad=-1),
    dict(logits=None), dict(lse=None), dict(target=(1, None)), dict(norm=(0, None)),
]


@pytest.mark.parametrize("kw", HEAD_BAD, ids=_ids)
def test_paired_head_refuses_bad_arguments_before_any_launch(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_rlosshead_fwd(ctypes.byref(_head(lib, **kw)), None) == 1           # MTN_ERR_ARG
    assert b"mtn_rlosshead_fwd" in h.mtn_last_error()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_rlosshead_bwd(code, ctypes.byref(_head(lib, **kw)), None) == 1
        assert b"mtn_rlosshead_bwd" in h.mtn_last_error()


def test_the_refusals_name_what_they_refuse():
    lib = _lib_or_build()
    h = lib.load()
    for kw, word in ((dict(rd_alpha=-0.5), b"rd_alpha"), (dict(pair=(0, -1)), b"pair < 0"), (dict(pair=(0, 2)), b"2 * pair rows"),
                     (dict(rowkl=None), b"rowkl")):
        assert h.mtn_rlosshead_fwd(ctypes.byref(_head(lib, **kw)), None) == 1
        assert word in h.mtn_last_error(), (kw, h.mtn_last_error())
        assert h.mtn_rlosshead_bwd(lib.MTN_BF16, ctypes.byref(_head(lib, **kw)), None) == 1
        assert word in h.mtn_last_error(), (kw, h.mtn_last_error())


@pytest.mark.parametrize("kw", [dict(ldd=100), dict(ldd=106), dict(gloss=None), dict(dlogits=None)], ids=_ids)
def test_paired_head_refuses_bad_backward_arguments(kw):
    lib = _lib_or_build()
    h = lib.load()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_rlosshead_bwd(code, ctypes.byref(_head(lib, **kw)), None) == 1
        assert b"mtn_rlosshead_bwd" in h.mtn_last_error()
    assert h.mtn_rlosshead_bwd(7, ctypes.byref(_head(lib)), None) == 1              # a dtype code that does not exist
    assert h.mtn_rlosshead_fwd(ctypes.byref(_head(lib, rowloss=None)), None) == 1
    assert h.mtn_rlosshead_fwd(None, None) == 1 and h.mtn_rlosshead_bwd(0, None, None) == 1


def test_pair_distances_past_n_seg_are_not_looked_at():
    """Segments 2 and 3 do not exist in the well-formed block: a bad pair there changes nothing — the refusal is that of the last
    segment's rows, which the walk over the segments reaches last."""
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_rlosshead_fwd(ctypes.byref(_head(lib, pair=(3, -5), rows=(1, 0))), None) == 1
    assert b"bad segment" in h.mtn_last_error()
    assert h.mtn_rlosshead_bwd(lib.MTN_BF16, ctypes.byref(_head(lib, pair=(2, 7), rows=(1, 0))), None) == 1
    assert b"bad segment" in h.mtn_last_error()
