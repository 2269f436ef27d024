"""--cut-a on the host (mtn_amd.data_handler.draw_cuts / cut_a_stream, mtn_amd.train.cut_a_applies) against the REFERENCE's
own outputs: tests/golden/cut_a.npz was produced by running the reference's make_batch with cut_a=True
(data_handler.py:255-260) after np.random.seed(seed) on fixtures.det_corpus (tools/make_cut_a_golden.py)."""
import ctypes
import logging
import os
import subprocess

import numpy as np
import pytest

from oracle import fixtures as fx

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = fx.load_golden(os.path.join(HERE, "golden", "cut_a.npz"))
CASES = [(cap, bsz, mlen, seed) for cap in (True, False) for bsz, mlen in ((4, 8), (6, 20)) for seed in (1, 7)]


def _plan(cap, bsz, mlen):
    from mtn_amd.data_handler import make_batch_indices
    data = fx.det_corpus(caption=cap)
    idx, _ = make_batch_indices(data, batchsize=bsz, max_length=mlen, separate_caption=cap)
    ans_len = np.array([len(d[4]) for d in sorted(data["dialogs"], key=lambda d: d[1])], dtype=np.int32)
    return data, idx, ans_len


def _final_state_matches(rs, tag):
    _, keys, pos, has_gauss, gauss = rs.get_state()
    return (np.array_equal(keys, GOLD[f"{tag}.state_keys"]) and pos == int(GOLD[f"{tag}.state_pos"])
            and [has_gauss, gauss] == GOLD[f"{tag}.state_gauss"].tolist())


@pytest.mark.parametrize("cap,bsz,mlen,seed", CASES)
def test_draw_plan_matches_reference(cap, bsz, mlen, seed):
    """The cut ends drawn here are the reference's (read off its truncated rows) and the stream ends where the reference's did."""
    from mtn_amd.data_handler import draw_cuts
    _, idx, ans_len = _plan(cap, bsz, mlen)
    tag = f"cap{int(cap)}.b{bsz}.s{seed}"
    rs = np.random.RandomState(seed)
    n_cut = 0
    for v, k in enumerate(GOLD[f"{tag}.visits"].tolist()):
        qa = list(idx[k][1])
        row_len = draw_cuts(ans_len, qa, 0.5, rs)
        want = (GOLD[f"{tag}.{v}.trg"] != fx.PAD).sum(axis=1)             # det_corpus tokens are >= 4: no pad inside an answer
        assert np.array_equal(want, (GOLD[f"{tag}.{v}.trg_y"] != fx.PAD).sum(axis=1))
        have = np.where(row_len >= 0, row_len, ans_len[qa])
        assert have.tolist() == want.tolist(), v
        assert np.all(row_len < ans_len[qa])                              # a cut always shortens the row
        n_cut += int((row_len >= 0).sum())
    assert n_cut > 0
    assert _final_state_matches(rs, tag)


def test_global_stream_is_the_default():
    """rng=None draws from the global np.random, as the reference does."""
    from mtn_amd.data_handler import draw_cuts
    _, idx, ans_len = _plan(True, 4, 8)
    tag = "cap1.b4.s1"
    saved = np.random.get_state()
    try:
        np.random.seed(1)
        for k in GOLD[f"{tag}.visits"].tolist():
            draw_cuts(ans_len, list(idx[k][1]))
        g = np.random.mtrand._rand
        assert _final_state_matches(g, tag)
    finally:
        np.random.set_state(saved)


def test_cut_a_p_zero_draws_but_never_cuts():
    from mtn_amd.data_handler import draw_cuts
    ans_len = np.array([5, 3, 9, 2, 7, 4], dtype=np.int32)
    rs, ref = np.random.RandomState(3), np.random.RandomState(3)
    for _ in range(20):
        assert (draw_cuts(ans_len, [0, 1, 2, 3, 4, 5], 0.0, rs) == -1).all()
    for _ in range(20 * 6):
        ref.uniform()                                                     # exactly one uniform per sample
    assert np.array_equal(rs.get_state()[1], ref.get_state()[1]) and rs.get_state()[2] == ref.get_state()[2]


def test_too_short_answer_names_the_qa_id():
    from mtn_amd.data_handler import draw_cuts
    with pytest.raises(ValueError, match="qa id 1 "):
        draw_cuts(np.array([4, 1], dtype=np.int32), [1], 1.0, np.random.RandomState(0))


def test_tokens_desc_layout_matches_c(tmp_path):
    from mtn_amd import lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\n'
                   'int main(){printf("%zu %zu\\n", sizeof(mtn_assemble_tokens_desc), offsetof(mtn_assemble_tokens_desc, row_len));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert size == ctypes.sizeof(lib.AssembleTokensDesc) and off == lib.AssembleTokensDesc.row_len.offset
    assert lib.AssembleTokensDesc().row_len is None                       # a zeroed struct: no cut


def test_library_version_has_row_len():
    from mtn_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    assert lib.load().mtn_version() >= 114


def test_rank_streams():
    from mtn_amd.data_handler import cut_a_stream
    r0, r1, ref = cut_a_stream(5, 0), cut_a_stream(5, 1), np.random.RandomState(5)
    a0, a1 = r0.uniform(size=16), r1.uniform(size=16)
    assert np.array_equal(a0, ref.uniform(size=16))
    assert not np.array_equal(a0, a1)
    assert np.array_equal(cut_a_stream(5, 1).uniform(size=16), a1) and not np.array_equal(cut_a_stream(6, 1).uniform(size=16), a1)


def test_fixed_batch_mode_warns(caplog):
    from mtn_amd.train import cut_a_applies, parse
    with caplog.at_level(logging.WARNING):
        assert not cut_a_applies(parse(["--cut-a", "1"]))
    assert any("corpus mode only" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert cut_a_applies(parse(["--cut-a", "1", "--corpus-videos", "4"]))
        assert not cut_a_applies(parse(["--corpus-videos", "4"]))
        assert not cut_a_applies(parse([]))
    assert not caplog.records


def test_corpus_checks_answer_fields_once():
    """A cut row is both answer fields cut to one length: DeviceCorpus refuses a corpus where that is not the reference's cut."""
    from mtn_amd.data_handler import DeviceCorpus
    data = fx.det_corpus(caption=True)
    corpus = DeviceCorpus(data, "cpu")
    corpus.check_cut_a()
    assert corpus.answer_lengths().tolist() == [len(d[4]) for d in sorted(data["dialogs"], key=lambda d: d[1])]
    bad = fx.det_corpus(caption=True)
    bad["dialogs"][4][5] = bad["dialogs"][4][5].copy()
    bad["dialogs"][4][5][0] += 1
    with pytest.raises(ValueError, match=r"qa id\(s\) \[%d\]" % bad["dialogs"][4][1]):
        DeviceCorpus(bad, "cpu").check_cut_a()
