"""The float64 reference of tests/test_score_kernel_gpu.py (tests/score_refs.py) checked without a GPU: tok_logp against
torch.log_softmax(...).gather in float64, tok_rank against a stable descending argsort, the sequence sums, what the case list plants,
and the recorded float32 yardstick the GPU bound is a multiple of."""
import pytest
import torch

from tests import score_refs as sr

CASES = sr.score_cases()
IDS = [sr.score_case_id(c) for c in CASES]


def test_case_list_covers_what_the_issue_names():
    assert {(c.n_seq, c.L, c.V, c.ldz) for c in CASES} == {(1, 1, 7, 8), (3, 5, 64, 64), (2, 20, 257, 264), (2, 9, 3004, 3008),
                                                          (1, 3, 4099, 4100), (1, 2, 40000, 40000)}
    for shape in sr.SHAPES:
        assert {c.offset for c in CASES if (c.n_seq, c.L, c.V, c.ldz) == shape} == {0.0, 50.0, -50.0}
    planted = set()
    for i, c in enumerate(CASES):
        planted |= set(sr.score_inputs(c, sr.SCORE_SEED + i)[2])
    assert planted == {"edge columns", "pads", "all-pad sequence", "two-sided tie", "duplicated maximum"}


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_reference_matches_log_softmax_and_stable_sort(idx):
    c = CASES[idx]
    z, t, planted = sr.score_inputs(c, sr.SCORE_SEED + idx)
    logp, rank, seq_logp, seq_len = sr.score_ref64(z, t, c.V)
    assert bool(torch.isnan(z[:, c.V:]).all()) and not bool(torch.isnan(z[:, :c.V]).any())
    ok = sr.valid_targets(t, c.V)
    flat_ok, flat_t = ok.reshape(-1), t.reshape(-1)
    ls = torch.log_softmax(z[:, :c.V].double(), dim=1)
    order = torch.argsort(z[:, :c.V], dim=1, descending=True, stable=True)       # equal values keep ascending column
    for r in range(flat_t.numel()):
        s, l = divmod(r, c.L)
        if not bool(flat_ok[r]):
            assert float(logp[s, l]) == 0.0 and int(rank[s, l]) == -1
            continue
        assert abs(float(logp[s, l]) - float(ls[r, flat_t[r]])) <= 1e-12 * max(1.0, abs(float(ls[r, flat_t[r]])))
        assert int(rank[s, l]) == int((order[r] == flat_t[r]).nonzero()[0, 0])
    assert torch.equal(seq_len, ok.sum(1).to(torch.int32))
    assert float((seq_logp - logp.sum(1)).abs().max()) <= 1e-12 * max(1.0, float(logp.sum(1).abs().max()))
    # what the case plants is there
    if "edge columns" in planted:
        assert int(t[0, 0]) == 0 and int(t[0, 1]) == c.V - 1 and float(z[1, 3]) == float(z[1, c.V - 1])
    if "pads" in planted:
        assert int(t[0, 2]) == sr.PAD and int(t[0, c.L - 1]) == sr.PAD and int(t[0, 3]) >= c.V and not bool(ok[0, 3])
    if "all-pad sequence" in planted:
        assert int(seq_len[-1]) == 0 and float(seq_logp[-1]) == 0.0 and bool((rank[-1] == -1).all())
    if "two-sided tie" in planted:
        hit = [(r, int(flat_t[r])) for r in range(flat_t.numel()) if bool(flat_ok[r]) and int(flat_t[r]) == c.V // 2
               and float(z[r, c.V // 2 - 2]) == float(z[r, c.V // 2]) == float(z[r, c.V // 2 + 2])]
        assert hit
        r, tt = hit[0]
        assert int(rank.reshape(-1)[r]) == int((z[r, :c.V] > z[r, tt]).sum()) + 1          # the lower equal column only
    if "duplicated maximum" in planted:
        top = z[:, :c.V].max(1).values
        assert bool(((z[:, :c.V] == top.unsqueeze(1)).sum(1) == 2).any())


def test_float32_yardstick_is_what_the_cpu_measures():
    """The constant the GPU bound is 4x of: the float32 CPU evaluation of the closed form against float64, re-measured."""
    worst = 0.0
    for i, c in enumerate(CASES):
        z, t, _ = sr.score_inputs(c, sr.SCORE_SEED + i)
        worst = max(worst, float((sr.closed_form_f32(z, t, c.V).double() - sr.score_ref64(z, t, c.V)[0]).abs().max()))
    assert sr.CPU_F32_TOK_LOGP_ABS / 2 <= worst <= sr.CPU_F32_TOK_LOGP_ABS * 2, worst
