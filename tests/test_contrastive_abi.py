"""CPU-side checks of the contrastive-search kernel's boundary, as tests/test_sched_abi.py does them: the header declares the entry point
and its argument block and restates the definition, the ctypes mirror has the C layout, the library exports the entry (detected by symbol:
the version stays what it was, tests/test_sched_abi.py pins it), contrastive.hip is one of the sources, and every argument the header
names as refused is refused before anything is launched (so no GPU is needed to see it; the pointers are never followed on the host)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID, TOP, TOK, POS, LP, STEP, DONE, LT, LL, LPN, LR = (4096 * (i + 1) for i in range(11))     # well-formed "device pointers"


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _args(lib, **kw):
    a = lib.ContrastiveArgs()
    f = dict(dialogues=2, k=5, L=20, d=512, k_top=7, alpha=0.6, eos=2, min_len=1, n_banned=1, hidden=HID, row_stride=20 * 512, pos_stride=512,
             top=TOP, tokens=TOK, pos=POS, cand_logp=LP, step=STEP, done=DONE, log_tok=LT, log_logp=LL, log_pen=LPN, log_rank=LR)
    f.update(kw)
    for k, v in f.items():
        setattr(a, k, v)
    a.banned[0] = 3
    return a


def test_header_declares_the_entry_point_and_restates_the_definition():
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"int\s+mtn_contrastive_advance\s*\(\s*const\s+mtn_contrastive_args\s*\*\s*\w+\s*(/\*.*?\*/)?\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"\}\s*mtn_contrastive_args\s*;", hdr)
    body = hdr[hdr.index("Contrastive search (csrc/contrastive.hip"):hdr.index("} mtn_contrastive_args;")]
    for field in ("dialogues", "k", "L", "d", "k_top", "alpha", "eos", "min_len", "n_banned", "banned[4]", "hidden", "row_stride", "pos_stride", "top",
                  "tokens", "pos", "cand_logp", "step", "done", "log_tok", "log_logp", "log_pen", "log_rank"):
        assert re.search(r"\b%s\s*[;,]" % re.escape(field), body), field
    for formula in ("pen_r = max over 0 <= j < l of  dot(h[r][l], h[r][j]) / ( sqrt(|h[r][l]|^2) * sqrt(|h[r][j]|^2) )", "(0 when either norm is 0)",
                    "s_r   = fl32( fl32((1 - alpha) * expf(cand_logp[r])) - fl32(alpha * pen_r) )", "never an fma", "ties to the lowest row",
                    "never wins", "r* is row 0", "a pure function of d", "ADMITTED", "eos while l < min_len", "cand_logp = -inf",
                    "min(max(l + 1, 0), L - 1)", "l == 0 is the bootstrap", "only advances its step", "alpha = 0 is greedy",
                    "k_top outside min(16, k + n_banned + 1)..16", "mtn_version() stays 125", "dialogues == 0 returns MTN_OK"):
        assert formula in body, formula


def test_args_layout_matches_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lib = _lib_or_build()
    fields = [f[0] for f in lib.ContrastiveArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){printf("%zu", sizeof(mtn_contrastive_args));\n'
                   + "".join('printf(" %%zu", offsetof(mtn_contrastive_args, %s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(lib.ContrastiveArgs)] + [getattr(lib.ContrastiveArgs, f).offset for f in fields]


def test_library_exports_the_entry_point():
    lib = _lib_or_build()
    assert lib.SYMBOLS["mtn_contrastive_advance"] == (ctypes.c_int, [ctypes.POINTER(lib.ContrastiveArgs), ctypes.c_void_p])
    h = lib.load()
    assert h.mtn_contrastive_advance is not None
    assert h.mtn_version() == 125
    assert "contrastive.hip" in __import__("mtn_amd.build", fromlist=["SOURCES"]).SOURCES


BAD = [
    dict(hidden=None), dict(top=None), dict(tokens=None), dict(pos=None), dict(cand_logp=None), dict(step=None), dict(done=None),   # null pointers
    dict(log_tok=None), dict(log_logp=None), dict(log_pen=None), dict(log_rank=None),
    dict(hidden=HID + 2), dict(top=TOP + 1), dict(cand_logp=LP + 2), dict(step=STEP + 3), dict(done=DONE + 2),                      # misaligned words
    dict(log_tok=LT + 2), dict(log_logp=LL + 1), dict(log_pen=LPN + 2), dict(log_rank=LR + 2),
    dict(tokens=TOK + 4), dict(pos=POS + 4),                                                                                       # misaligned 64-bit words
    dict(k=0), dict(k=17), dict(k=-1), dict(k_top=17, k=16), dict(k_top=0), dict(d=0), dict(d=1025, pos_stride=1025, row_stride=20 * 1025), dict(d=-4),
    dict(L=0), dict(L=-1), dict(L=(1 << 20) + 1, row_stride=((1 << 20) + 1) * 512), dict(n_banned=5, k_top=16), dict(n_banned=-1),
    dict(k_top=6), dict(k_top=5), dict(k=12, k_top=13), dict(k=16, k_top=15), dict(k=5, n_banned=4, k_top=9),                        # k_top < min(16, k + n_banned + 1)
    dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=float("-inf")),
    dict(pos_stride=511), dict(pos_stride=0), dict(row_stride=20 * 512 - 1), dict(pos_stride=516), dict(row_stride=0),             # below the dense strides
    dict(dialogues=-1), dict(dialogues=(1 << 31) - 1, k=2, k_top=4), dict(dialogues=1 << 28, k=16, k_top=16),                       # dialogues * k overflows int
    dict(dialogues=0, alpha=2.0), dict(dialogues=0, hidden=None), dict(dialogues=0, k=17),                                         # refused on an empty call too
]


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_refusals(kw):
    lib = _lib_or_build()
    h = lib.load()
    a = _args(lib, **kw)
    assert h.mtn_contrastive_advance(ctypes.byref(a), None) == 1             # MTN_ERR_ARG
    assert b"mtn_contrastive_advance" in h.mtn_last_error()


def test_null_args_are_refused():
    h = _lib_or_build().load()
    assert h.mtn_contrastive_advance(None, None) == 1
    assert b"mtn_contrastive_advance" in h.mtn_last_error()


@pytest.mark.parametrize("kw", [dict(dialogues=0), dict(dialogues=0, k=1, k_top=3), dict(dialogues=0, alpha=0.0), dict(dialogues=0, alpha=1.0, k=16, k_top=16)],
                         ids=str)
def test_an_empty_call_is_ok_and_launches_nothing(kw):
    """dialogues == 0 with well-formed arguments returns MTN_OK before any launch: no device is needed to see it."""
    lib = _lib_or_build()
    assert lib.load().mtn_contrastive_advance(ctypes.byref(_args(lib, **kw)), None) == 0


def test_the_operator_refuses_cpu_tensors():
    import torch
    from mtn_amd import ops
    lib = _lib_or_build()
    z = torch.zeros
    log = (z(4, 1, dtype=torch.int32), z(4, 1), z(4, 1), z(4, 1, dtype=torch.int32))
    with pytest.raises(lib.MtnHipError):
        ops.contrastive_advance(z(2, 4, 8), z(2, 9), z(2, 4, dtype=torch.long), z(1, dtype=torch.long), z(2), z(1, dtype=torch.int32),
                                z(1, dtype=torch.int32), log, k=2, alpha=0.5)
