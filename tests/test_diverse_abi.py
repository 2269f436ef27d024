"""CPU-side checks of the diverse beam search's boundary, as tests/test_abi.py does them: the ctypes mirror of mtn_diverse_args has the
C struct's size (and its two own fields sit where C puts them), and the library exports the entry point."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_or_build():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_diverse_args_layout_matches_c(tmp_path):
    lib = _lib_or_build()
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(mtn_diverse_args),'
                   ' sizeof(mtn_beam_args), offsetof(mtn_diverse_args, groups), offsetof(mtn_diverse_args, diversity));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(lib.DiverseArgs), ctypes.sizeof(lib.BeamArgs), lib.DiverseArgs.groups.offset, lib.DiverseArgs.diversity.offset]


def test_library_exports_the_entry_point():
    lib = _lib_or_build()
    assert "mtn_diverse_advance" in lib.SYMBOLS
    h = lib.load()
    assert h.mtn_diverse_advance is not None and h.mtn_version() >= 119
