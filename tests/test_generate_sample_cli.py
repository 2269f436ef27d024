"""--decode-style sample at the command line and at the ABI boundary (no GPU needed)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_accepts_the_sample_style_and_its_flags():
    from mtn_amd import generate as G
    a = G.parse(["--decode-style", "sample", "--temperature", "0.7", "--top-k", "40", "--top-p", "0.9", "--samples", "4", "--sample-seed", "11"])
    assert (a.decode_style, a.temperature, a.top_k, a.top_p, a.samples, a.sample_seed) == ("sample", 0.7, 40, 0.9, 4, 11)
    d = G.parse(["--decode-style", "sample"])
    assert (d.temperature, d.top_k, d.top_p, d.samples, d.sample_seed) == (1.0, 0, 1.0, 1, 1)
    assert G.parse(["--decode-style", "sample", "--samples", "16"]).samples == 16
    # the other styles are parsed as before
    assert G.parse([]).decode_style == "greedy" and G.parse(["--decode-style", "beam_search"]).decode_style == "beam_search"


@pytest.mark.parametrize("argv", [["--samples", "17"], ["--samples", "0"], ["--top-p", "0"], ["--top-p", "1.5"], ["--top-k", "-1"],
                                  ["--temperature", "-0.5"]])
def test_parse_rejects_bad_sampling_arguments(argv, capsys):
    from mtn_amd import generate as G
    with pytest.raises(SystemExit) as e:
        G.parse(["--decode-style", "sample"] + argv)
    assert e.value.code == 2
    assert argv[0] in capsys.readouterr().err
    with pytest.raises(SystemExit):
        G.parse(["--decode-style", "nucleus"])


def test_abi_declares_and_binds_the_sampling_kernel():
    import ctypes
    from mtn_amd import lib
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    assert re.search(r"\bint\s+mtn_sample_rows\s*\(\s*const\s+mtn_sample_args\s*\*", hdr)
    assert "mtn_sample_rows" in lib.SYMBOLS and lib.SYMBOLS["mtn_sample_rows"][1][0]._type_ is lib.SampleArgs
    # the ctypes mirror follows the C struct field by field
    body = re.search(r"typedef struct \{([^}]*)\} mtn_sample_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip().lstrip("*").strip()) for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].replace("float*", "").replace("long*", "").replace("int*", "").split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == [f[0] for f in lib.SampleArgs._fields_], names
    assert ctypes.sizeof(lib.SampleArgs) % 8 == 0


def test_sample_args_struct_size_matches_c(tmp_path):
    import ctypes
    import subprocess
    from mtn_amd import lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(mtn_sample_args),'
                   ' offsetof(mtn_sample_args, seed), offsetof(mtn_sample_args, log_tok), offsetof(mtn_sample_args, anc));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = lib.SampleArgs
    assert sizes == [ctypes.sizeof(S), S.seed.offset, S.log_tok.offset, S.anc.offset]


def test_decode_exposes_the_sampling_search():
    import inspect
    from mtn_amd import decode, ops
    sig = inspect.signature(decode.sample_decode_many)
    assert list(sig.parameters)[:6] == ["model", "batch", "max_len", "start", "eos", "pad"]
    for name, default in (("samples", 1), ("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("seed", 0), ("keys", None), ("banned", ()),
                          ("min_len", 1), ("penalty", 0.0)):
        assert sig.parameters[name].default == default and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(ops.sample_rows)
