"""The numpy definition of contrastive search (tests/contrastive_refs.py) held to itself: the error bound against a float32 emulation of
the kernel's arithmetic, the condition on the GPU cases that keeps tests/test_contrastive_kernel_gpu.py from hinging on rounding (every
scored step is decided by at least 4 bounds), the two greedy limits, and the state machine's done / min_len / banned / short-head rules."""
import numpy as np
import pytest

from tests import contrastive_refs as R


@pytest.mark.parametrize("d", [8, 20, 128, 512])
def test_bound_holds_against_a_float32_emulation(d):
    rng = np.random.default_rng(d)
    worst_s = worst_c = 0.0
    for alpha in (0.0, 0.3, 0.6, 1.0):
        for trial in range(6):
            k, l = 5, 7
            h = (rng.standard_normal((k, 1, d)) * rng.uniform(-1, 1.5, size=(k, l + 1, 1)) + 0.6 * rng.standard_normal((k, l + 1, d))).astype(np.float32)
            lp = np.log(rng.dirichlet(np.ones(k))).astype(np.float32)
            s32, p32 = R.emulate_f32(h, l, alpha, lp)
            p64 = R.penalties(h, l)
            s64 = R.scores(alpha, lp, p64)
            worst_c = max(worst_c, float(np.abs(p32.astype(np.float64) - p64).max()))
            assert np.abs(p32.astype(np.float64) - p64).max() <= R.cos_bound(d)
            assert np.abs(s32.astype(np.float64) - s64).max() <= R.bound(float(np.float32(alpha)), d)
            worst_s = max(worst_s, float(np.abs(s32.astype(np.float64) - s64).max()))
    print("d=%d: worst cosine error %.3g (bound %.3g), worst score error %.3g" % (d, worst_c, R.cos_bound(d), worst_s))


@pytest.mark.parametrize("c", R.GPU_CASES, ids=lambda c: c["name"])
def test_every_gpu_case_is_decided_by_four_bounds(c):
    """A condition on the inputs, asserted for every scored step of every case: nothing is skipped."""
    states = R.run_case(c)
    margins = states[-1].margins
    scored = [(l, dlg) for l in range(max(c["l0"], 1), min(c["l0"] + c["n"], c["L"])) for dlg in range(c["D"])]
    assert set(margins) <= set(scored)
    if c["special"] is None:
        assert set(margins) == set(scored)                          # no dialogue of a plain case finishes early
    B = R.bound(float(np.float32(c["alpha"])), c["d"])
    for at, m in sorted(margins.items()):
        print(c["name"], at, "margin %.3g = %.1f B" % (m, m / B))
        assert m >= 4 * B, (c["name"], at, m, B)


def _step(h, lp, l, alpha):
    pen = R.penalties(h, l)
    return R.winner(R.scores(alpha, lp, pen), lp)[0], pen


def test_alpha_zero_and_k_one_are_the_arg_max():
    rng = np.random.default_rng(5)
    for _ in range(20):
        h = rng.standard_normal((5, 6, 16)).astype(np.float32)
        lp = np.log(rng.dirichlet(np.ones(5))).astype(np.float32)
        assert _step(h, lp, 5, 0.0)[0] == int(np.argmax(lp))
        assert _step(h[:1], lp[:1], 5, float(rng.uniform()))[0] == 0
    # through the state machine: the head is sorted, so row 0 wins every step and the tokens are the heads' first columns
    c = next(c for c in R.GPU_CASES if c["name"] == "alpha0")
    states = R.run_case(c)
    st, launches, _ = R.make_case(c)
    assert (states[-1].log_rank == 0).all()
    for i in range(1, c["n"]):
        for dlg in range(c["D"]):
            assert states[-1].log_tok[i, dlg] == int(launches[i - 1][1][dlg * c["k"], c["k_top"]])


def test_penalty_definition():
    h = np.zeros((2, 3, 4), dtype=np.float32)
    h[0, 0], h[0, 1], h[0, 2] = [1, 0, 0, 0], [0, 2, 0, 0], [3, 3, 0, 0]
    h[1, 0], h[1, 2] = [1, 1, 1, 1], [-2, -2, -2, -2]               # h[1][1] is zero: its cosine counts as 0
    np.testing.assert_allclose(R.penalties(h, 2), [np.sqrt(0.5), 0.0], rtol=1e-15)
    h[1, 2, 0] = np.nan
    assert np.isnan(R.penalties(h, 2)[1])
    s = R.scores(0.5, np.float32([-1.0, 0.0]), R.penalties(h, 2))
    assert R.winner(s, np.float32([-1.0, 0.0])) == (0, np.inf)       # the NaN row never wins
    assert R.winner(np.array([0.25, 0.25, 0.1]), np.float32([-1, -1, -2]))[0] == 0       # ties to the lowest row
    assert R.winner(np.array([0.5, 0.2]), np.float32([-np.inf, -1]))[0] == 1             # a row at -inf never wins
    assert R.winner(np.array([np.nan, 0.2]), np.float32([-1, -np.inf])) == (0, np.inf)   # nobody can: row 0


def _head(vals, cols):
    return np.array(list(vals) + list(cols) + [0.0], dtype=np.float32)


def test_deal_rules():
    head = _head([-0.5, -1, -2, -3, -4, -5], [2, 7, 30, 31, 11, 32])
    cols, vals = R.deal(head, 3, 0, eos=2, min_len=1, banned=(7, 11))              # <eos> barred at l < min_len, banned ids skipped
    assert cols.tolist() == [30, 31, 32] and vals.tolist() == [-2, -3, -5]
    cols, vals = R.deal(head, 3, 1, eos=2, min_len=1, banned=(7, 11))              # <eos> admitted from min_len on
    assert cols.tolist() == [2, 30, 31] and vals.tolist() == [-0.5, -2, -3]
    cols, vals = R.deal(head, 5, 0, eos=2, min_len=1, banned=(7, 11))              # three admitted entries for five rows
    assert cols.tolist() == [30, 31, 32, 32, 32] and vals[:3].tolist() == [-2, -3, -5] and np.isneginf(vals[3:]).all()
    short = _head([-0.1, -2.5, -4, -np.inf, -np.inf, -np.inf], [1, 2, 0, 0, 0, 0])   # V = 3 under k = 5
    cols, vals = R.deal(short, 5, 3, eos=-1, min_len=1, banned=())
    assert cols.tolist() == [1, 2, 0, 0, 0] and np.isneginf(vals[3:]).all()


def test_state_machine_done_and_limits():
    c = next(c for c in R.GPU_CASES if c["name"] == "eos_done")
    states = R.run_case(c)
    mid, l0 = c["D"] // 2, c["l0"]
    assert states[1].done.tolist() == [int(d == mid) for d in range(c["D"])]
    rows = slice(mid * c["k"], mid * c["k"] + c["k"])
    for a, b in zip(states[1:], states[2:]):                         # the finished dialogue only advances its step
        assert b.step[mid] == a.step[mid] + 1
        assert (b.tokens[rows] == a.tokens[rows]).all() and (b.cand_logp[rows] == a.cand_logp[rows]).all()
        assert (b.log_tok[:, mid] == a.log_tok[:, mid]).all()
    assert (states[1].tokens[rows, l0 + 1] == states[0].tokens[rows, l0 + 1]).all()  # ... and got no candidates when it finished
    # the last position writes no candidates, a step past L only counts
    c = next(c for c in R.GPU_CASES if c["name"] == "L9_l8")
    states = R.run_case(c)
    assert states[1].step.tolist() == [9] and states[2].step.tolist() == [10] and states[1].pos == states[2].pos == 8
    assert (states[2].tokens == states[1].tokens).all() and (states[1].tokens[:, 8] == states[1].log_tok[8, 0]).all()
    # <eos> heads under min_len = 4: barred while l < 4
    c = next(c for c in R.GPU_CASES if c["name"] == "eos_barred")
    states = R.run_case(c)
    assert (states[1].tokens[:, 3] != c["eos"]).all() and (states[2].tokens[:, 4] != c["eos"]).all() and (states[3].tokens[::c["k"], 5] == c["eos"]).all()
    c = next(c for c in R.GPU_CASES if c["name"] == "eos_allowed")
    states = R.run_case(c)
    assert states[2].done.all() and (states[2].log_tok[3] == c["eos"]).all()
    for name, admitted in (("banned", 5), ("few_admitted", 13)):
        c = next(c for c in R.GPU_CASES if c["name"] == name)
        st = R.run_case(c)[-1]
        assert not np.isin(st.tokens, c["banned"]).any()
        assert name == "banned" or not (st.tokens == c["eos"]).any()      # (min_len = 9 bars <eos> at every step of that case)
        assert (~np.isneginf(st.cand_logp.reshape(c["D"], c["k"]))).sum(1).tolist() == [admitted] * c["D"]
    c = next(c for c in R.GPU_CASES if c["name"] == "tie")
    states = R.run_case(c)
    assert (states[1].log_rank[c["l0"]] == 0).all()                  # rows 0 and 1 hold the same score: the lower one
    st, launches, _ = R.make_case(c)
    for dlg in range(c["D"]):
        s = R.scores(c["alpha"], st.cand_logp[dlg * 5:dlg * 5 + 5], R.penalties(launches[0][0][dlg * 5:dlg * 5 + 5], c["l0"]))
        assert s[0] == s[1] == s.max()
    c = next(c for c in R.GPU_CASES if c["name"] == "nan_row")
    assert (R.run_case(c)[1].log_rank[c["l0"]] >= 2).all()


def test_response_and_score():
    log_tok = np.array([[0], [5], [6], [2], [9]], dtype=np.int32)
    log_logp = np.array([[0], [-1], [-2], [-0.5], [-7]], dtype=np.float32)
    assert R.response(log_tok, log_logp, 0, eos=2, penalty=0.5) == ([5, 6], -3.5 + 0.5 * 3, 3)
    assert R.response(log_tok, log_logp, 0, eos=99, penalty=1.0) == ([5, 6, 2, 9], -10.5 + 5.0, 4)
