"""Rider workgroups (csrc/fused.hip, csrc/gemm_k512.hip): the K|V projections of the constant memories for decoder layers >= 1 leave the head
of the step and travel as extra workgroups of the layers' fused forward launches, on compute units those launches leave empty.  A tile
is computed by one device function wherever it travels, so everything here is compared BIT FOR BIT with the schedule of MTN_RIDERS=0:
hoisted K|V buffers, fold vectors, gradients, and whole captured train steps (loss, weights, Adam moments).

Shapes: the fused path's fixed widths (d_model 512, 8 heads, d_ff 2048) at small extents — 2 layers, batch 4, Q/H/C/T = 8/24/16/8, 8 frames per
modality: 24 main workgroups in a fused launch, every memory one partial 128-row tile; and H = 34 (4 x 34 = 128 + 8 rows): a memory
of two row tiles, the second partial."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCHES = ("MTN_RIDERS", "MTN_RIDER_MAX_SLOTS", "MTN_RIDER_FFN_HOSTS")
K512 = "gemm_k512_kernel"


def _set_env(env):
    from mtn_amd import lib as L
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    L.load().mtn_reload_env()


def _counters():
    from mtn_amd import lib as L
    out = (C.c_long * 4)()
    L.check(L.load().mtn_rider_counters(out))
    return list(out)


def _make(H, dropout=0.1):
    """dropout: of the sublayers and of the attention probabilities alike"""
    from mtn_amd import make_model
    from mtn_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    model = make_model(100, 100, N=2, d_model=512, d_ff=2048, h=8, dropout=dropout, ft_sizes=[2048, 128], diff_encoder=True,
                       auto_encoder_ft="query", compute_dtype=torch.bfloat16, attn_dropout=dropout).to(dev).train()
    batch = synthetic_batch(100, 4, 8, H, 16, 8, [8, 8], [2048, 128], device=dev, seed=5)
    return model, batch


def _eager(env, H=24):
    """One eager forward + backward: K|V buffers, fold vectors, gradients, the GEMM launch census, rider counters."""
    from mtn_amd import lib as L
    from mtn_amd.train_step import TrainStep
    _set_env(env)
    try:
        model, batch = _make(H)
        ts = TrainStep(model, batch, 100, use_graph=False, fuse_optimizer=False)
        lib = L.load()
        c0 = _counters()
        lib.mtn_census_begin()
        loss = ts._fwd_bwd()
        torch.cuda.synchronize()
        n = lib.mtn_census_end()
        c1 = _counters()
        census = []
        for i in range(n):
            info = L.CensusLaunch()
            L.check(lib.mtn_census_info(i, C.byref(info)))
            census.append((lib.mtn_census_variant_name(info.variant).decode(), info.workgroups, info.count))
        kvs = [kv.clone() for _, kv in model._kv_targets]
        assert len(kvs) == 10                     # 2 layers x (3 text + 2 video memories)
        return dict(loss=loss.clone(), kvs=kvs, fold=model._ln_fold_buf.clone(), grad=model.flat_buffers()[2].clone(), census=census,
                    rode=c1[0] - c0[0], flushed=c1[1] - c0[1], flush_launches=c1[2] - c0[2], pending=c1[3])
    finally:
        _set_env({})


def _graph(env, use_graph=True, H=24, dropout=0.1):
    """Two train steps (captured and replayed, or eager): losses, weights, Adam moments."""
    from mtn_amd.train_step import TrainStep
    _set_env(env)
    try:
        model, batch = _make(H, dropout)
        step = TrainStep(model, batch, 100, pad=1, warmup=4000, use_graph=use_graph)
        losses = [step().clone() for _ in range(2)]
        torch.cuda.synchronize()
        adam = step.opt.optimizer
        return dict(losses=losses, flat=model._flat.detach().clone(), m=adam.m.clone(), v=adam.v.clone())
    finally:
        _set_env({})


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))          # bits, not values: -0 / NaN payloads count


def _assert_eager_equal(a, b):
    assert _same(a["loss"], b["loss"])
    for i, (x, y) in enumerate(zip(a["kvs"], b["kvs"])):
        assert _same(x, y), f"K|V buffer {i}"
    assert _same(a["fold"], b["fold"])
    assert _same(a["grad"], b["grad"])


_cache = {}


def _ref(kind, H=24):
    """MTN_RIDERS=0 results, computed once per shape and shared."""
    key = (kind, H)
    if key not in _cache:
        _cache[key] = _eager({"MTN_RIDERS": "0"}, H) if kind == "eager" else _graph({"MTN_RIDERS": "0"}, kind == "graph", H)
    return _cache[key]


def _k512(census):
    return [c for c in census if c[0] == K512]


def test_forward_backward_bitwise_and_every_deferred_tile_rides():
    ref, on = _ref("eager"), _eager({})
    _assert_eager_equal(on, ref)
    # layer 1's five projections: 1 row tile x 4 column tiles (128 x 256) each, all in the first fused launch of layer 0 (232 empty CUs)
    assert on["rode"] == 20 and on["flushed"] == 20 and on["flush_launches"] == 1 and on["pending"] == 0, on
    # the census: layer 0's projections as one wide K = 512 launch of 20 tiles, no K = 512 launch after it; without riders none at all
    # (the grouped launch of both layers, 40 tiles, goes to a general kernel) — the one launch in which the two censuses differ
    assert _k512(on["census"]) == [(K512, 20, 5)]
    assert _k512(ref["census"]) == [] and ref["rode"] == 0 and ref["flush_launches"] == 0
    first = [i for i, c in enumerate(on["census"]) if c[0] == K512][0]
    assert on["census"][:first] == ref["census"][:first] and on["census"][first + 1:] == ref["census"][first + 1:]


def test_row_tile_edge_memory_of_128_plus_8_rows():
    ref, on = _ref("eager", 34), _eager({}, 34)
    _assert_eager_equal(on, ref)
    assert on["rode"] == 24 and on["pending"] == 0, on      # the history memory: two row tiles x 4 column tiles


def test_leftover_path_flushes_stand_alone():
    """Two slots per launch: in first-use order the 8 launches in front of layer 1's first reader carry its 12 tiles and the others
    follow in time — nothing is left.  Without the feed-forward hosts (5 hosts per layer) or with one slot, projections are still
    pending when their reader comes: they leave as stand-alone wide launches, which the census shows."""
    ref = _ref("eager")
    for env, leftover in (({"MTN_RIDER_MAX_SLOTS": "2"}, False), ({"MTN_RIDER_MAX_SLOTS": "2", "MTN_RIDER_FFN_HOSTS": "0"}, True),
                          ({"MTN_RIDER_MAX_SLOTS": "1"}, True)):
        on = _eager(env)
        _assert_eager_equal(on, ref)
        s = {k: on[k] for k in ("rode", "flushed", "flush_launches", "pending")}
        assert on["pending"] == 0 and on["rode"] + on["flushed"] == 40 and on["rode"] > 0, (env, s)
        k = _k512(on["census"])
        assert len(k) == on["flush_launches"] and sum(c[1] for c in k) == on["flushed"] and k[0] == (K512, 20, 5), (env, k, s)
        assert (on["rode"] < 20 and len(k) >= 2) if leftover else (on["rode"] == 20 and len(k) == 1), (env, k, s)


def test_no_slots_is_the_schedule_without_riders():
    ref, off = _ref("eager"), _eager({"MTN_RIDER_MAX_SLOTS": "0"})
    _assert_eager_equal(off, ref)
    assert off["census"] == ref["census"] and off["rode"] == 0 and off["flush_launches"] == 0


def test_switches_change_nothing_but_the_carrier():
    ref = _ref("eager")
    for v in ("0", "1"):
        _assert_eager_equal(_eager({"MTN_RIDER_FFN_HOSTS": v, "MTN_RIDER_MAX_SLOTS": "3"}), ref)


def _assert_steps_equal(a, b):
    for i, (x, y) in enumerate(zip(a["losses"], b["losses"])):
        assert _same(x, y), f"loss of step {i}: {float(x)} vs {float(y)}"
    for k in ("flat", "m", "v"):
        assert _same(a[k], b[k]), k
    assert all(bool(torch.isfinite(l)) for l in a["losses"])


def test_captured_steps_bitwise():
    _assert_steps_equal(_graph({}), _ref("graph"))


def test_eager_steps_equal_replayed_steps():
    """Dropout off: the warm-up passes of a capture advance the dropout seed, so an eager step and a replayed one draw different masks
    (with riders or without); everything else of the two runs is the same arithmetic."""
    on = _graph({}, dropout=0.0)
    _assert_steps_equal(on, _graph({}, use_graph=False, dropout=0.0))
    _assert_steps_equal(on, _graph({"MTN_RIDERS": "0"}, dropout=0.0))
