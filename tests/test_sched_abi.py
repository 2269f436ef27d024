"""CPU-side checks of the scheduled-sampling kernel's boundary, as tests/test_accum_abi.py does them: the header declares the entry point,
its argument block and its two picks, the library exports it (detected by symbol: the version stays what it was, tests/test_scst_abi.py
pins it), sched.hip is one of the sources, and every argument the header names as refused is refused before anything is launched (so no
GPU is needed to see it; the pointers are never followed on the host)."""
import ctypes
import os
import re

import pytest

from tests import sched_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, TRG, KEY, ST, MIX, STATS, SCORE = 4096, 8192, 16384, 32768 + 4, 65536, 131072 + 8, 262144 + 4     # well-formed "device pointers"


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _args(lib, **kw):
    a = lib.SchedArgs()
    f = dict(B=2, T=5, V=100, ldx=104, logits=Z, trg=TRG, key=KEY, state=ST, pad=1, n_banned=1, p_max=0.25, start=0, ramp=0,
             pick=R.ARGMAX, inv_temperature=1.0, seed=0, mixed=MIX, stats=STATS, pick_score=SCORE)
    f.update(kw)
    for k, v in f.items():
        setattr(a, k, v)
    a.banned[0] = 2
    return a


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"int\s+mtn_sched_mix\s*\(\s*const\s+mtn_sched_args\s*\*\s*\w+\s*(/\*.*?\*/)?\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"\}\s*mtn_sched_args\s*;", hdr)
    for name, value in (("ARGMAX", R.ARGMAX), ("SAMPLE", R.SAMPLE)):
        assert re.search(r"#define\s+MTN_SCHED_%s\s+%d\b" % (name, value), hdr)
    body = hdr[hdr.index("Scheduled sampling, the token mix"):hdr.index("} mtn_sched_args;")]
    for field in ("logits", "trg", "key", "state", "pad", "n_banned", "banned[4]", "p_max", "start", "ramp", "pick", "inv_temperature", "seed",
                  "mixed", "stats", "pick_score"):
        assert re.search(r"\b%s\s*[;,]" % re.escape(field), body), field
    for formula in ("p_max * min(1, max(0, step - start) / ramp)", "0xFFFFFFFF", "<< 12", "2^-24", "-log(-log(u_c))", "inv_temperature + g_c",
                    "ties to the lowest", "T >= 4096", "V >= 2^24", "mixed == trg"):
        assert formula in body, formula


def test_library_exports_the_entry_point():
    lib = _lib_or_build()
    assert lib.SYMBOLS["mtn_sched_mix"] == (ctypes.c_int, [ctypes.POINTER(lib.SchedArgs), ctypes.c_void_p])
    assert (lib.MTN_SCHED_ARGMAX, lib.MTN_SCHED_SAMPLE) == (R.ARGMAX, R.SAMPLE)
    h = lib.load()
    assert h.mtn_sched_mix is not None
    assert h.mtn_version() == 125
    assert "sched.hip" in __import__("mtn_amd.build", fromlist=["SOURCES"]).SOURCES


BAD = [
    dict(logits=None), dict(trg=None), dict(key=None), dict(state=None), dict(mixed=None), dict(stats=None),      # null pointers
    dict(logits=Z + 2), dict(state=ST + 1), dict(pick_score=SCORE + 2),                                         # misaligned floats
    dict(trg=TRG + 4), dict(key=KEY + 4), dict(mixed=MIX + 4), dict(stats=STATS + 4),                           # misaligned 64-bit words
    dict(mixed=TRG),                                                                                           # aliasing the gold ids
    dict(V=1 << 24), dict(V=(1 << 24) + 5, ldx=(1 << 24) + 8), dict(V=0), dict(V=-3),                            # V outside [1, 2^24)
    dict(T=4096), dict(T=5000), dict(T=-1), dict(B=-1),                                                        # T >= 4096; negative sizes
    dict(ldx=99), dict(ldx=0),                                                                                 # ldx < V
    dict(pick=2), dict(pick=-1),                                                                               # an unknown pick
    dict(p_max=-0.01), dict(p_max=1.01), dict(p_max=float("nan")),                                             # p outside [0, 1]
    dict(n_banned=5), dict(n_banned=-1),                                                                       # more than 4 banned ids
    dict(start=-1), dict(ramp=-1),
    dict(inv_temperature=0.0), dict(inv_temperature=-1.0), dict(inv_temperature=float("inf")), dict(inv_temperature=float("nan")),
    dict(B=0, mixed=TRG), dict(T=0, p_max=2.0), dict(B=0, V=1 << 24),                                            # refused on an empty batch too
]


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_refusals(kw):
    lib = _lib_or_build()
    h = lib.load()
    a = _args(lib, **kw)
    assert h.mtn_sched_mix(ctypes.byref(a), None) == 1             # MTN_ERR_ARG
    assert b"mtn_sched_mix" in h.mtn_last_error()


def test_null_args_are_refused():
    h = _lib_or_build().load()
    assert h.mtn_sched_mix(None, None) == 1


@pytest.mark.parametrize("kw", [dict(B=0), dict(T=0), dict(B=0, T=0), dict(B=0, pick_score=None), dict(T=0, pick=R.SAMPLE, p_max=1.0)], ids=str)
def test_an_empty_batch_is_ok_and_launches_nothing(kw):
    """B == 0 or T == 0 with well-formed arguments returns MTN_OK before any launch: no device is needed to see it."""
    lib = _lib_or_build()
    assert lib.load().mtn_sched_mix(ctypes.byref(_args(lib, **kw)), None) == 0


def test_config_validation():
    from mtn_amd.train_step import SchedConfig
    c = SchedConfig(0.25)
    assert (c.prob, c.start, c.ramp, c.pick, c.temperature, c.seed, c.banned) == (0.25, 0, 0, "argmax", 1.0, 0, (2,))
    SchedConfig(1.0, start=10, ramp=100, pick="sample", temperature=0.5, seed=7, banned=(2, 3, 4, 5))
    for kw in (dict(prob=0.0), dict(prob=-0.1), dict(prob=1.5), dict(prob=float("nan")), dict(prob=0.5, start=-1), dict(prob=0.5, ramp=-2),
               dict(prob=0.5, start=1.5), dict(prob=0.5, pick="greedy"), dict(prob=0.5, temperature=0.0), dict(prob=0.5, temperature=float("inf")),
               dict(prob=0.5, seed=-1), dict(prob=0.5, seed=1 << 62), dict(prob=0.5, banned=(1, 2, 3, 4, 5)), dict(prob=0.5, banned=(-1,))):
        with pytest.raises(ValueError):
            SchedConfig(**kw)
