"""The K = 512 projection kernels (csrc/gemm_k512.hip, csrc/gemm_k512_tile.h: y = x W^T + b, bf16 in, bf16 out) and the host queue
behind mtn_kv_project, through the C ABI, against the float64 reference and the derived elementwise bound of tests/k512_refs.py.

(a) the wide 128 x 256 tile (gk_wide_tile) as stand-alone gemm_k512w_kernel launches of any size: mtn_kv_project with
    n_now = count - 1 flushes the head of the queue at once and mtn_riders_flush the rest.  What the lists of k512_refs.CASES reach:
      one_row_tile  M = 1, 16, 127 (partial row tile), M = 128 (a full last row tile); N = 256 and 512; lda = 512, 520, 1024;
                    ldb = 512, 528; ldc = N, N + 8 and 2 N (128 x 256 into the second column block of a [*, 512] buffer); null bias
      row_tiles     tiles_m = 2 (M = 129, 257: a last row tile of one row) and 3 (M = 384, all full) with 1, 2 and 3 column tiles:
                    tn = t / tiles_m past the first column tile; 129 x 512 into the second block of a [*, 1024] buffer
      nine_tiles    384 x 768 (3 x 3 tiles) behind a one-tile problem (tile_start > 0), lda = 520, ldb = 528, ldc = N + 8, null bias;
                    the problem that waits for the flush has two row tiles and writes the second block of a [*, 1536] buffer
    In every list x starts 16 bytes into its allocation and every output 8 rows (and, for ldc = 2 N, N columns) into its buffer.
(b) the queue, on one-tile problems (8 x 256): groups of MTN_GEMM_MAX_GROUP, the n_now head, leftovers of an earlier call, lists
    that do not defer (a problem the kernels do not take for the wide tile, nothing to defer, riders off), the counters, the order.
(c) the three forms on one problem set just above the 512-tile minimum of mtn_gemm (k512_refs.FORMS, 514 tiles of 128 x 128): wide
    (default, 257 workgroups), 128 x 128 (MTN_K512_WIDE=0, 514), persistent (MTN_K512_PERSIST=1, 256); each against the bound, then
    bit for bit against each other.

Every output lives in a buffer of NaN with 8 guard rows before and after and pad columns where ldc > N; afterwards every in-range
element is finite and inside the bound and everything else still holds the NaN bit for bit.  The three forms share one census name:
the workgroup count tells which one ran, and every problem set here gives the forms it could take different counts."""
import ctypes as C
import os
from contextlib import contextmanager

import pytest
import torch

from tests import k512_refs as R

pytestmark = pytest.mark.gpu

GUARD = 8                     # sentinel rows before and after every output (8 rows keep any row stride 16-byte aligned)
SWITCHES = ("MTN_RIDERS", "MTN_RIDER_MAX_SLOTS", "MTN_K512_PERSIST", "MTN_K512_WIDE")
K512 = "gemm_k512_kernel"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _set_env(env):
    from mtn_amd import lib as L
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    L.reload_env()


def _counters():
    """[tiles computed by riders, tiles flushed stand-alone, stand-alone flush launches, tiles pending]"""
    from mtn_amd import lib as L
    out = (C.c_long * 4)()
    L.check(L.load().mtn_rider_counters(out))
    return list(out)


def _delta(c0):
    c1 = _counters()
    return [c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2], c1[3]]


@contextmanager
def _queue(env=None):
    """The switches as given (all others unset), an empty queue, the counters at entry; on the way out whatever is pending is computed
    while the caller's tensors are still alive, nothing may be left, and the switches are unset again."""
    from mtn_amd import lib as L
    lib = L.load()
    _set_env(env or {})
    try:
        L.check(lib.mtn_riders_flush(L.stream_ptr()))
        torch.cuda.synchronize()
        c0 = _counters()
        assert c0[3] == 0
        try:
            yield c0
        finally:
            L.check(lib.mtn_riders_flush(L.stream_ptr()))
            torch.cuda.synchronize()
            assert _counters()[3] == 0
    finally:
        _set_env({})


@contextmanager
def _census(log):
    """Appends (variant name, workgroups, problems, M of the first four, N of the first four) per launch to `log`."""
    from mtn_amd import lib as L
    lib = L.load()
    lib.mtn_census_begin()
    try:
        yield
    finally:
        for i in range(lib.mtn_census_end()):
            info = L.CensusLaunch()
            L.check(lib.mtn_census_info(i, C.byref(info)))
            k = min(info.count, 4)
            log.append((lib.mtn_census_variant_name(info.variant).decode(), info.workgroups, info.count, list(info.M)[:k], list(info.N)[:k]))


class _Out:
    """An output [GUARD + M + GUARD, ldc] of NaN; the problem's N columns start at column `col` (ldc = 2 N: the second block)."""

    def __init__(self, dev, M, N, ldc):
        self.M, self.N, self.ldc, self.col = M, N, ldc, (N if ldc == 2 * N else 0)
        self.full = torch.full((M + 2 * GUARD, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
        self.sentinel = self.full[:1, :1].view(torch.int16).clone()

    def ptr(self):
        return self.full.data_ptr() + (GUARD * self.ldc + self.col) * 2

    def untouched(self):
        return bool((self.full.view(torch.int16) == self.sentinel).all())

    def value(self):
        return self.full[GUARD:GUARD + self.M, self.col:self.col + self.N]

    def check(self, case, what):
        """Guard rows, pad columns and the other column block still the sentinel bit for bit; in-range elements finite and inside the bound."""
        inside = torch.zeros(self.full.shape, dtype=torch.bool, device=self.full.device)
        inside[GUARD:GUARD + self.M, self.col:self.col + self.N] = True
        same = self.full.view(torch.int16) == self.sentinel
        assert bool(same[~inside].all()), f"{what} {case.shape}: {int((~same[~inside]).sum())} guard / pad elements were written"
        return R.assert_within(self.value(), case, what)


class _Problems:
    """Device copies of a list of cases and their outputs, as a GemmProblem array.  x sits 16 bytes into its allocation."""

    def __init__(self, dev, cases):
        from mtn_amd import lib as L
        self.cases, self.outs, self.keep = cases, [], []
        self.arr = (L.GemmProblem * len(cases))()
        for p, c in zip(self.arr, cases):
            xb = torch.full((8 + c.M * c.lda,), float("nan"), dtype=torch.bfloat16, device=dev)
            xb[8:] = c.x.reshape(-1).to(dev)
            w = c.w.to(dev)
            b = None if c.bias is None else c.bias.to(dev)
            o = _Out(dev, c.M, c.N, c.ldc)
            p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K = xb.data_ptr() + 16, w.data_ptr(), c.lda, c.ldb, c.M, c.N, R.K
            p.bias, p.gate_scale, p.out_lp, p.ldc = (None if b is None else b.data_ptr()), 1.0, o.ptr(), c.ldc
            assert p.A % 16 == 0 and p.out_lp % 16 == 0 and p.A != xb.data_ptr() and p.out_lp != o.full.data_ptr()
            self.keep += [xb, w, b]
            self.outs.append(o)

    def fresh_outputs(self, dev):
        self.outs = [_Out(dev, c.M, c.N, c.ldc) for c in self.cases]
        for p, o in zip(self.arr, self.outs):
            p.out_lp = o.ptr()

    def check(self, what, which=None):
        worst = max(self.outs[i].check(self.cases[i], f"{what}[{i}]") for i in (range(len(self.cases)) if which is None else which))
        print(f"{what}: worst |out - ref| / bound = {worst:.4f}")
        return worst


def _kv_project(P, n_now):
    from mtn_amd import lib as L
    L.check(L.load().mtn_kv_project(L.MTN_BF16, len(P.cases), P.arr, n_now, L.stream_ptr()))


def _flush():
    from mtn_amd import lib as L
    L.check(L.load().mtn_riders_flush(L.stream_ptr()))


_case_cache = {}


def _case(shape, seed):
    """Cases and their float64 references are built once per (shape, seed) and only read afterwards."""
    if (shape, seed) not in _case_cache:
        _case_cache[(shape, seed)] = R.with_refs(R.make_case(shape, seed))
    return _case_cache[(shape, seed)]


# ------------------------------------------------------------------------------------------ (a) the wide tile, stand-alone
@pytest.mark.parametrize("name", list(R.CASES))
def test_wide_tile_stand_alone(dev, name):
    shapes = R.CASES[name]
    cases = [_case(s, 100 + i) for i, s in enumerate(shapes)]
    n = len(shapes)
    log = []
    with _queue() as c0:
        P = _Problems(dev, cases)
        with _census(log):
            _kv_project(P, n - 1)
            torch.cuda.synchronize()
            last = R.tiles(shapes[-1:], 256)
            assert _delta(c0) == [0, R.tiles(shapes[:-1], 256), 1, last]
            assert P.outs[-1].untouched()                        # the problem that waits has not been computed
            worst = P.check(name, range(n - 1))
            _flush()
            torch.cuda.synchronize()
        assert _delta(c0) == [0, R.tiles(shapes, 256), 2, 0]
        worst = max(worst, P.check(name))
    # only K = 512 launches, of sum tiles_m * N / 256 workgroups: the wide form ran, in the order passed in
    assert log == [(K512, R.tiles(shapes[:-1], 256), n - 1, [s[0] for s in shapes[:-1]][:4], [s[1] for s in shapes[:-1]][:4]),
                   (K512, last, 1, [shapes[-1][0]], [shapes[-1][1]])], log
    assert 0.0 < worst <= 1.0


# ------------------------------------------------------------------------------------------ (b) the queue
def _queue_cases(n, seed0=200):
    return [_case(R.QUEUE_SHAPE, seed0 + i) for i in range(n)]


def test_queue_flushes_in_groups_of_sixteen(dev):
    from mtn_amd import lib as L
    assert L.GEMM_MAX_GROUP == 16
    call, flush = [], []
    with _queue() as c0:
        P = _Problems(dev, _queue_cases(18))
        with _census(call):
            _kv_project(P, 17)
            torch.cuda.synchronize()
        assert _delta(c0) == [0, 17, 2, 1]
        assert P.outs[17].untouched()
        P.check("head of 17", range(17))
        with _census(flush):
            _flush()
            torch.cuda.synchronize()
        assert _delta(c0) == [0, 18, 3, 0]
        P.check("all 18")
    assert [e[:3] for e in call] == [(K512, 16, 16), (K512, 1, 1)] and [e[:3] for e in flush] == [(K512, 1, 1)], (call, flush)


def test_queue_flushes_leftovers_of_an_earlier_call_first(dev):
    log = []
    with _queue() as c0:
        P = _Problems(dev, _queue_cases(2))
        Q = _Problems(dev, _queue_cases(2, seed0=230))
        with _census(log):
            _kv_project(P, 1)
            torch.cuda.synchronize()
            assert _delta(c0) == [0, 1, 1, 1] and P.outs[1].untouched()
            _kv_project(Q, 1)                                    # P[1] leaves first, in a launch of its own; then Q[0]
            torch.cuda.synchronize()
            assert _delta(c0) == [0, 3, 3, 1] and Q.outs[1].untouched()
            P.check("first call")
            Q.check("second call, head", [0])
            _flush()
            torch.cuda.synchronize()
            assert _delta(c0) == [0, 4, 4, 0]
        Q.check("second call")
    assert [(e[0], e[1], e[2]) for e in log] == [(K512, 1, 1)] * 4, log


def test_queue_keeps_the_order_passed_in(dev):
    """One-tile problems told apart by their row counts.  The census lists a launch's first four problems: two flush launches of four."""
    Ms = [8, 7, 6, 5, 4, 3, 2, 1]
    cases = [_case((M,) + R.QUEUE_SHAPE[1:], 260 + M) for M in Ms]
    log = []
    with _queue() as c0:
        P = _Problems(dev, cases)
        with _census(log):
            _kv_project(P, 4)
            _flush()
            torch.cuda.synchronize()
        assert _delta(c0) == [0, 8, 2, 0]
        P.check("order")
    assert log == [(K512, 4, 4, Ms[:4], [256] * 4), (K512, 4, 4, Ms[4:], [256] * 4)], log


def _assert_grouped_general_launches(dev, cases, n_now, env):
    """The list does not defer: the grouped mtn_gemm launches of all of it, now, on a general kernel (far below the 512-tile minimum
    of the K = 512 kernels); the counters do not move; the outputs are inside the bound all the same."""
    log = []
    with _queue(env) as c0:
        P = _Problems(dev, cases)
        with _census(log):
            _kv_project(P, n_now)
            torch.cuda.synchronize()
        assert _delta(c0) == [0, 0, 0, 0]
        P.check("not deferred")
    n = len(cases)
    assert [e[2] for e in log] == [min(16, n - i) for i in range(0, n, 16)], log
    assert all(e[0] != K512 and e[0].startswith("gemm_") for e in log), log


def test_queue_does_not_defer_a_list_with_a_problem_the_wide_tile_does_not_take(dev):
    cases = _queue_cases(18)
    cases[5] = _case((8, 264, 512, 512, 272, True), 290)         # N = 264 is no multiple of 256
    _assert_grouped_general_launches(dev, cases, 17, {})


def test_queue_does_not_defer_when_everything_is_wanted_now(dev):
    _assert_grouped_general_launches(dev, _queue_cases(18), 18, {})


def test_queue_does_not_defer_with_riders_off(dev):
    _assert_grouped_general_launches(dev, _queue_cases(18), 17, {"MTN_RIDERS": "0"})


# ------------------------------------------------------------------------------------------ (c) the three forms
FORM_ENV = {"wide": {}, "narrow": {"MTN_K512_WIDE": "0"}, "persistent": {"MTN_K512_PERSIST": "1"}}
# one census name for the three forms: only these counts (257, 514, 256; pinned by tests/test_k512_refs.py) tell which one ran
FORM_WORKGROUPS = {"wide": R.tiles(R.FORMS, 256), "narrow": R.tiles(R.FORMS, 128), "persistent": R.PERSISTENT_GRID}
assert len(set(FORM_WORKGROUPS.values())) == 3


@pytest.fixture(scope="module")
def forms(dev):
    """The problem set with its float64 reference (computed once), run through mtn_gemm in each of the three forms."""
    from mtn_amd import lib as L
    lib = L.load()
    P = _Problems(dev, [R.with_refs(R.make_case(s, 300 + i)) for i, s in enumerate(R.FORMS)])
    runs = {}
    for form, env in FORM_ENV.items():
        log = []
        with _queue(env):
            P.fresh_outputs(dev)
            with _census(log):
                L.check(lib.mtn_gemm(L.MTN_BF16, len(R.FORMS), P.arr, L.stream_ptr()))
                torch.cuda.synchronize()
        runs[form] = (P.outs, log)
    return P, runs


@pytest.mark.parametrize("form", list(FORM_ENV))
def test_form_at_the_512_tile_minimum(forms, form):
    P, runs = forms
    outs, log = runs[form]
    assert [(e[0], e[1], e[2]) for e in log] == [(K512, FORM_WORKGROUPS[form], len(R.FORMS))], log
    worst = max(o.check(c, f"{form}[{i}]") for i, (o, c) in enumerate(zip(outs, P.cases)))
    print(f"{form}: worst |out - ref| / bound = {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_forms_agree_bit_for_bit(forms):
    """One accumulator per output element, sixteen 32-deep steps in ascending k, a float32 bias add and one rounding, in all three."""
    P, runs = forms
    for other in ("narrow", "persistent"):
        for i, (a, b) in enumerate(zip(runs["wide"][0], runs[other][0])):
            differ = int((a.value().view(torch.int16) != b.value().view(torch.int16)).sum())
            assert differ == 0, f"wide vs {other}, problem {i} {P.cases[i].shape}: {differ} of {a.value().numel()} elements differ in their bits"
