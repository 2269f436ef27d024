"""CPU-side checks of the self-critical-training entry points' boundary, as tests/test_distill_abi.py does them: the header declares
them, the ctypes mirrors have the C structs' sizes and field offsets (mtn_losshead_args is the prefix of mtn_wlosshead_args), the library
exports them at version 125, and every argument the header names as refused is refused before anything is launched (so no GPU is needed
to see it)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_FIELDS = ["n_seg", "rows", "target", "norm", "coef", "V", "ldz", "pad", "smoothing", "logits", "lse", "rowloss", "gloss", "dlogits", "ldd"]
STRUCTS = {
    "mtn_wlosshead_args": ("WLossHeadArgs", HEAD_FIELDS + ["roww", "smoothing_seg"]),
    "mtn_eval_rows_args": ("EvalRowsArgs", ["Qc", "R", "L", "ldl", "ref", "ref_len", "n_ref", "workspace", "workspace_bytes", "N", "hyp", "hyp_len",
                                            "item", "stats", "rouge", "cider"]),
    "mtn_scst_assemble_args": ("ScstAssembleArgs", ["rows", "L", "T", "log_tok", "sos", "eos", "pad", "trg", "trg_y", "hyp", "ldh", "hyp_len"]),
    "mtn_scst_advantage_args": ("ScstAdvantageArgs", ["D", "S", "T", "reward", "baseline", "roww", "adv", "mean_reward", "mean_baseline"]),
}
ENTRIES = ["mtn_wlosshead_fwd", "mtn_wlosshead_bwd", "mtn_eval_table_build", "mtn_eval_score_rows", "mtn_scst_assemble", "mtn_scst_advantage"]


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _ids(kw):
    return ",".join("%s=%s" % i for i in kw.items())


def test_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"int\s+mtn_wlosshead_fwd\s*\(\s*const\s+mtn_wlosshead_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)
    assert re.search(r"int\s+mtn_wlosshead_bwd\s*\(\s*int\s+\w+\s*,\s*const\s+mtn_wlosshead_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", hdr)
    for fn, st in (("mtn_eval_table_build", "mtn_eval_rows_args"), ("mtn_eval_score_rows", "mtn_eval_rows_args"),
                   ("mtn_scst_assemble", "mtn_scst_assemble_args"), ("mtn_scst_advantage", "mtn_scst_advantage_args")):
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s\s*\*\s*\w*\s*(/\*.*?\*/)?\s*,\s*void\s*\*\s*\w*\s*\)\s*;" % (fn, st), hdr), fn


def test_struct_layouts_match_c(tmp_path):
    lib = _lib_or_build()
    exprs = []
    for st, (_, fields) in STRUCTS.items():
        exprs.append("sizeof(%s)" % st)
        exprs += ["offsetof(%s, %s)" % (st, f) for f in fields]
    exprs += ["offsetof(mtn_losshead_args, %s)" % f for f in HEAD_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){size_t v[] = {%s};\n'
                   'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);\nreturn 0;}\n' % ", ".join(exprs))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mine = []
    for _, (cls, fields) in STRUCTS.items():
        c = getattr(lib, cls)
        assert [f for f, _ in c._fields_] == fields
        mine.append(ctypes.sizeof(c))
        mine += [getattr(c, f).offset for f in fields]
    mine += [getattr(lib.WLossHeadArgs, f).offset for f in HEAD_FIELDS]                      # the loss head's block is the prefix
    assert sizes == mine
    assert [getattr(lib.LossHeadArgs, f).offset for f in HEAD_FIELDS] == [getattr(lib.WLossHeadArgs, f).offset for f in HEAD_FIELDS]


def test_library_exports_the_entry_points():
    lib = _lib_or_build()
    h = lib.load()
    for name in ENTRIES:
        assert name in lib.SYMBOLS and getattr(h, name) is not None
    assert lib.SYMBOLS["mtn_wlosshead_fwd"][1][0] == ctypes.POINTER(lib.WLossHeadArgs)
    assert lib.SYMBOLS["mtn_wlosshead_bwd"][1][:2] == [ctypes.c_int, ctypes.POINTER(lib.WLossHeadArgs)]
    assert h.mtn_version() == 125


# ------------------------------------------------------------------------------------------ weighted loss head
def _head(lib, **kw):
    """A well-formed block (the pointers are never followed on the host), then ``kw`` over it."""
    a = lib.WLossHeadArgs()
    a.n_seg = 2
    for s in range(2):
        a.rows[s], a.target[s], a.norm[s], a.coef[s], a.smoothing_seg[s] = 3, 64 * (s + 1), 1024 + 64 * s, 1.0, (0.0, -1.0)[s]
    a.V, a.ldz, a.pad, a.smoothing, a.ldd = 104, 104, 1, 0.1, 104
    a.logits, a.lse, a.rowloss, a.gloss, a.dlogits = 2048, 4096, 8192, 16384, 32768
    a.roww[0] = 131072
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


HEAD_BAD = [
    dict(roww=(0, 131072 + 2)), dict(roww=(1, 131072 + 1)), dict(smoothing_seg=(0, float("nan"))),
    dict(V=102), dict(V=0), dict(n_seg=5), dict(n_seg=0), dict(rows=(1, 0)), dict(ldz=100), dict(pad=104), dict(pad=-1),
    dict(logits=None), dict(lse=None), dict(target=(1, None)), dict(norm=(0, None)),
]


@pytest.mark.parametrize("kw", HEAD_BAD, ids=_ids)
def test_weighted_head_refuses_bad_arguments_before_any_launch(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_wlosshead_fwd(ctypes.byref(_head(lib, **kw)), None) == 1           # MTN_ERR_ARG
    assert b"mtn_wlosshead_fwd" in h.mtn_last_error()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_wlosshead_bwd(code, ctypes.byref(_head(lib, **kw)), None) == 1
        assert b"mtn_wlosshead_bwd" in h.mtn_last_error()


@pytest.mark.parametrize("kw", [dict(ldd=100), dict(ldd=106), dict(gloss=None), dict(dlogits=None)], ids=_ids)
def test_weighted_head_refuses_bad_backward_arguments(kw):
    lib = _lib_or_build()
    h = lib.load()
    for code in (lib.MTN_F32, lib.MTN_BF16):
        assert h.mtn_wlosshead_bwd(code, ctypes.byref(_head(lib, **kw)), None) == 1
    assert h.mtn_wlosshead_bwd(7, ctypes.byref(_head(lib)), None) == 1              # a dtype code that does not exist
    assert h.mtn_wlosshead_fwd(ctypes.byref(_head(lib, rowloss=None)), None) == 1
    assert h.mtn_wlosshead_fwd(None, None) == 1 and h.mtn_wlosshead_bwd(0, None, None) == 1


def test_weight_pointers_past_n_seg_are_not_looked_at():
    """Segments 2 and 3 do not exist in the well-formed block: a misaligned pointer there changes nothing — the refusal is V's."""
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_wlosshead_fwd(ctypes.byref(_head(lib, roww=(3, 7), V=102)), None) == 1
    assert b"V and ldz" in h.mtn_last_error()


# ------------------------------------------------------------------------------------------ rewards against a fixed corpus
def _rows(lib, **kw):
    a = lib.EvalRowsArgs()
    a.Qc, a.R, a.L, a.ldl = 7, 3, 12, 12
    a.ref, a.ref_len, a.n_ref = 4096, 8192, 12288
    a.workspace, a.workspace_bytes = 1 << 20, lib.load().mtn_eval_workspace_bytes(7, 3, 12)
    a.N, a.hyp, a.hyp_len, a.item = 10, 16384, 20480, 24576
    a.stats, a.rouge, a.cider = 28672, 32768, 36864
    for k, v in kw.items():
        setattr(a, k, v)
    return a


CORPUS_BAD = [dict(Qc=0), dict(R=0), dict(R=9), dict(L=0), dict(L=129), dict(ldl=11), dict(ref=None), dict(ref_len=None), dict(n_ref=None),
              dict(workspace=None), dict(workspace=(1 << 20) + 8), dict(workspace_bytes=1024), dict(Qc=1 << 27)]
ROWS_BAD = [dict(N=0), dict(N=-3), dict(hyp=None), dict(hyp_len=None), dict(item=None), dict(stats=None), dict(rouge=None), dict(cider=None)]


@pytest.mark.parametrize("kw", CORPUS_BAD, ids=_ids)
def test_table_build_and_score_rows_refuse_a_bad_corpus(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_eval_workspace_bytes(7, 3, 12) > 0
    assert h.mtn_eval_table_build(ctypes.byref(_rows(lib, **kw)), None) == 1
    assert b"mtn_eval_table_build" in h.mtn_last_error()
    assert h.mtn_eval_score_rows(ctypes.byref(_rows(lib, **kw)), None) == 1
    assert b"mtn_eval_score_rows" in h.mtn_last_error()


@pytest.mark.parametrize("kw", ROWS_BAD, ids=_ids)
def test_score_rows_refuses_bad_rows(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_eval_score_rows(ctypes.byref(_rows(lib, **kw)), None) == 1
    assert b"mtn_eval_score_rows" in h.mtn_last_error()
    assert h.mtn_eval_score_rows(None, None) == 1 and h.mtn_eval_table_build(None, None) == 1


# ------------------------------------------------------------------------------------------ assemble and advantage
def _asm(lib, **kw):
    a = lib.ScstAssembleArgs()
    a.rows, a.L, a.T, a.log_tok, a.sos, a.eos, a.pad = 6, 5, 5, 4096, 0, 2, 1
    a.trg, a.trg_y, a.hyp, a.ldh, a.hyp_len = 8192, 12288, 16384, 5, 20480
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _adv(lib, **kw):
    a = lib.ScstAdvantageArgs()
    a.D, a.S, a.T, a.reward, a.roww, a.mean_reward, a.mean_baseline = 3, 2, 5, 4096, 8192, 12288, 12296
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw", [dict(rows=0), dict(L=0), dict(T=4), dict(ldh=4), dict(log_tok=None), dict(trg=None), dict(trg_y=None),
                                dict(hyp=None), dict(hyp_len=None)], ids=_ids)
def test_assemble_refuses_bad_arguments(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_scst_assemble(ctypes.byref(_asm(lib, **kw)), None) == 1
    assert b"mtn_scst_assemble" in h.mtn_last_error()
    assert h.mtn_scst_assemble(None, None) == 1


@pytest.mark.parametrize("kw", [dict(D=0), dict(D=1025), dict(S=0), dict(S=65), dict(S=1), dict(T=0), dict(reward=None), dict(roww=None),
                                dict(mean_reward=None), dict(mean_baseline=None)], ids=_ids)
def test_advantage_refuses_bad_arguments(kw):
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_scst_advantage(ctypes.byref(_adv(lib, **kw)), None) == 1
    assert b"mtn_scst_advantage" in h.mtn_last_error()
    assert h.mtn_scst_advantage(None, None) == 1


def test_one_sample_is_refused_only_without_a_baseline():
    """S = 1 has no leave-one-out mean; with a baseline the refusal below comes from T alone."""
    lib = _lib_or_build()
    h = lib.load()
    assert h.mtn_scst_advantage(ctypes.byref(_adv(lib, S=1, baseline=16384, T=0)), None) == 1
    assert b"T >= 1" in h.mtn_last_error()
