"""csrc/average.hip on the GPU against tests/average_refs.py, bit for bit: every size at which the kernels take another path (n < 4: tail
only; n % 4 != 0; one size past a full pass of the capped grid, so that the grid-stride loop wraps and the tail runs), ranges that start
inside a larger buffer whose guard bands must not change, and a captured graph of schedule tick + EMA update."""
import numpy as np
import pytest
import torch

from tests import average_refs as R

pytestmark = pytest.mark.gpu
SIZES = [1, 3, 4, 5, 63, 64, 4096, 4099, (1 << 21) + 7]      # 2048 workgroups x 256 lanes x 4 floats = 1 << 21: one full pass of the capped grid
OFFSETS = [0, 4, 4092]
GUARD = 64
F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from mtn_amd import lib
    return lib.load()


def _values(rs, n):
    """normal floats with magnitudes from 1e-6 to 1e3 and both signs, plus exact zeros; no denormals, infinities or NaNs"""
    x = (10.0 ** rs.uniform(-6, 3, n) * rs.choice([-1.0, 1.0], n)).astype(F)
    x[rs.rand(n) < 0.05] = 0.0
    return x


@pytest.fixture(scope="module")
def pool():
    """Two host buffers of the largest size every case takes its ranges from (left unchanged)."""
    rs = np.random.RandomState(11)
    total = GUARD + max(OFFSETS) + max(SIZES) + GUARD
    return _values(rs, total), _values(rs, total)


def _case(pool, dev, off, n):
    """(host a, host b, device a, device b, slice of the range) — a buffer of guard + off + n + guard elements"""
    total = GUARD + off + n + GUARD
    a, b = pool[0][:total].copy(), pool[1][:total].copy()
    return a, b, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), slice(GUARD + off, GUARD + off + n)


def _bits(t):
    return t.cpu().numpy().view(np.int32) if torch.is_tensor(t) else np.asarray(t, dtype=F).view(np.int32)


def _ptr(t, sl):
    assert (t.data_ptr() + 4 * sl.start) % 16 == 0
    return t.data_ptr() + 4 * sl.start


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_lerp_is_bit_equal_to_the_definition(hip, dev, pool, n, off):
    for coef in (0.0, 1.0 / 3.0, 0.5, 1.0):
        a, b, da, db, sl = _case(pool, dev, off, n)
        assert hip.mtn_lerp_f32(n, _ptr(da, sl), _ptr(db, sl), coef, _stream()) == 0, hip.mtn_last_error()
        want = a.copy()
        want[sl] = R.lerp(a[sl], b[sl], F(coef))
        assert np.array_equal(_bits(da), _bits(want)), (n, off, coef)         # the range bit for bit, the guard bands and the gap untouched
        assert np.array_equal(_bits(db), _bits(b))                           # x is read only


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_ema_step_is_bit_equal_to_the_definition(hip, dev, pool, n, off):
    steps, decays = [1, 79, 80, 81, 10000], [0.0, 0.9, 0.999, 0.9999]
    # every (step, decay) pair at the sizes that fit one pass; at the size that wraps the grid, every step and every decay once
    combos = [(t, d) for t in steps for d in decays] if n <= 4099 else [(1, 0.0), (79, 0.9), (80, 0.9), (81, 0.999), (10000, 0.9999)]
    state = torch.zeros(8, device=dev)
    coef_out = torch.zeros(1, device=dev)
    for i, (t, decay) in enumerate(combos):
        a, b, da, db, sl = _case(pool, dev, off, n)
        state[0] = float(t)
        assert hip.mtn_ema_step(n, _ptr(da, sl), _ptr(db, sl), state.data_ptr(), decay, coef_out.data_ptr(), _stream()) == 0, hip.mtn_last_error()
        c = coef_out.cpu().numpy()[0]
        ref_c = R.ema_coef(decay, t)
        # the definition asks for a correctly rounded division; one ulp in case the compiler's is not
        assert abs(int(np.array(c, dtype=F).view(np.int32)) - int(np.array(ref_c, dtype=F).view(np.int32))) <= 1, (t, decay, c, ref_c)
        want = a.copy()
        want[sl] = R.lerp(a[sl], b[sl], c)
        assert np.array_equal(_bits(da), _bits(want)), (n, off, t, decay)
        assert np.array_equal(_bits(db), _bits(b))                           # p is read only
        if i % 7 == 0:                                                       # coef_out is optional: without it the same elements
            a2, b2, da2, db2, _ = _case(pool, dev, off, n)
            assert hip.mtn_ema_step(n, _ptr(da2, sl), _ptr(db2, sl), state.data_ptr(), decay, None, _stream()) == 0
            assert torch.equal(da2.view(torch.int32), da.view(torch.int32))
        assert float(state[0]) == float(t) and float(state[1:].abs().sum()) == 0.0      # the state is read only


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_exactly_and_twice_is_the_identity(hip, dev, pool, n, off):
    a, b, da, db, sl = _case(pool, dev, off, n)
    assert hip.mtn_swap_f32(n, _ptr(da, sl), _ptr(db, sl), _stream()) == 0, hip.mtn_last_error()
    wa, wb = a.copy(), b.copy()
    wa[sl], wb[sl] = b[sl], a[sl]
    assert np.array_equal(_bits(da), _bits(wa)) and np.array_equal(_bits(db), _bits(wb))
    assert hip.mtn_swap_f32(n, _ptr(da, sl), _ptr(db, sl), _stream()) == 0
    assert np.array_equal(_bits(da), _bits(a)) and np.array_equal(_bits(db), _bits(b))


def test_an_empty_range_touches_nothing(hip, dev, pool):
    a, b, da, db, sl = _case(pool, dev, 4, 8)
    st = torch.ones(8, device=dev)
    assert hip.mtn_lerp_f32(0, _ptr(da, sl), _ptr(db, sl), 0.5, _stream()) == 0
    assert hip.mtn_ema_step(0, _ptr(da, sl), _ptr(db, sl), st.data_ptr(), 0.9, None, _stream()) == 0
    assert hip.mtn_swap_f32(0, _ptr(da, sl), _ptr(db, sl), _stream()) == 0
    assert np.array_equal(_bits(da), _bits(a)) and np.array_equal(_bits(db), _bits(b))


def test_tick_and_ema_step_in_a_captured_graph(hip, dev, pool):
    """A hipGraph holding mtn_noam_tick and mtn_ema_step, replayed three times (the masters change between replays), equals three
    eager calls and ema_run with the coefficients of t = 1..3."""
    n, decay = 4099, 0.999
    masters = [pool[1][k * 5000:k * 5000 + n].copy() for k in range(3)]
    start = pool[0][:n].copy()

    def tick_and_update(state, ema, p):
        assert hip.mtn_noam_tick(state.data_ptr(), 1.0, 64, 10, 0.9, 0.98, _stream()) == 0
        assert hip.mtn_ema_step(n, ema.data_ptr(), p.data_ptr(), state.data_ptr(), decay, None, _stream()) == 0

    e_state, e_ema, e_p = torch.zeros(8, device=dev), torch.from_numpy(start).to(dev), torch.empty(n, device=dev)
    for m in masters:
        e_p.copy_(torch.from_numpy(m))
        tick_and_update(e_state, e_ema, e_p)
    g_state, g_ema, g_p = torch.zeros(8, device=dev), torch.from_numpy(start).to(dev), torch.empty(n, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick_and_update(g_state, g_ema, g_p)
    assert float(g_state[0]) == 0.0 and np.array_equal(_bits(g_ema), _bits(start))       # capture ran nothing
    for m in masters:
        g_p.copy_(torch.from_numpy(m))
        graph.replay()
    torch.cuda.synchronize()
    assert float(g_state[0]) == 3.0 and torch.equal(g_state, e_state)
    assert torch.equal(g_ema.view(torch.int32), e_ema.view(torch.int32))
    assert np.array_equal(_bits(g_ema), _bits(R.ema_run(masters, decay, start=start)))
