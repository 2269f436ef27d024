"""`python generate.py --evaluate` (mtn_amd.generate) on the GPU, end to end, on the mini AVSD fixture and the one-epoch checkpoint of
test_generate_gpu.py: the six logged lines and the result JSON's "eval" equal the Python definition (tests/eval_refs.py) applied to the
answers the run wrote, and evaluate.py on the written file prints the same six lines."""
import json
import logging

import pytest

from tests import eval_refs as R
from tests.test_generate_gpu import _argv, run  # noqa: F401  (run: the module's fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-9                                                       # tests/test_eval_kernel_gpu.py says why


@pytest.mark.parametrize("style,beam,undisclosed", [("greedy", 5, 0), ("beam_search", 3, 0), ("greedy", 5, 1)],
                         ids=["greedy", "beam3", "greedy-undisclosed"])
def test_generate_evaluate_logs_and_writes_what_the_definition_gives(run, style, beam, undisclosed, caplog, capsys):
    from mtn_amd import evaluate as E
    from mtn_amd import generate as G
    out = str(run["tmp"] / f"eval_{style}_{undisclosed}.json")
    argv = _argv(run, style, "bf16", undisclosed, out)
    argv[argv.index("--beam") + 1] = str(beam)
    caplog.set_level(logging.INFO)
    caplog.clear()
    result = G.main(argv + ["--evaluate"])
    written = json.load(open(out))
    assert written == result and set(written) == {"dialogs", "eval"}

    labelled = json.load(open(run["full"]))
    pairs = E.pair(written, labelled, last=bool(undisclosed))
    assert len(pairs) == sum(1 if undisclosed else len(d["dialog"]) for d in labelled["dialogs"])
    hyps, refs = E.to_ids(pairs)
    want = R.evaluate(hyps, refs)
    lines = ["%s: %.3f" % (k, v) for k, v in zip(R.NAMES, want["corpus"][:6])]
    msgs = [r.getMessage() for r in caplog.records]
    i = msgs.index(lines[0])
    assert msgs[i:i + 6] == lines and sum(m.startswith("CIDEr: ") for m in msgs) == 1
    ev = written["eval"]
    print({k: (ev[k], float(w)) for k, w in zip(R.NAMES, want["corpus"][:6])})
    assert all(abs(ev[k] - float(w)) <= TOL for k, w in zip(R.NAMES, want["corpus"][:6]))
    assert (ev["hyp_len"], ev["ref_len"], ev["n_items"]) == (int(want["corpus"][6]), int(want["corpus"][7]), len(pairs))

    capsys.readouterr()
    res = E.main([out, run["full"]] + (["--last"] if undisclosed else []))
    assert capsys.readouterr().out.splitlines() == lines
    assert {k: res[k] for k in R.NAMES} == {k: ev[k] for k in R.NAMES}       # the same launch on the same ids: the same bits

    # without the flag: the same answers, and no "eval"
    plain = G.main(argv)
    assert plain == {"dialogs": written["dialogs"]} and json.load(open(out)) == plain
