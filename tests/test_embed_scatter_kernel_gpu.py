"""Direct tests of mtn_embed_bwd_group (csrc/layernorm.hip) on both of its kernels — embed_bwd_det_kernel (the default) and the
float-atomic embed_bwd_kernel (MTN_EMBED_DETERMINISTIC=0) — against the float64 scatter and the derived, order-independent bound of
tests/ln_row_refs.py embed64:  (4 + n + EMB_W + 1) 2^-24 (|dlut before| + sum |addend|) for an entry with n addends.  The cases sit on
the deterministic kernel's bookkeeping edges: EMB_HEAVY = 24 (24 hits light, 25 all waves), EMB_CH = 8192 (8192 tokens resident, 8193
restaged per pass), stream boundaries inside a 64-token ballot, V no multiple of EMB_W = 8, two tables of different V and d in one
launch, the second 512-column pass (d = 640) under dropout, and a table that already holds values (+=).  Every token list states its
own hit counts; tokens stay inside [0, V).  Keep masks come from tests/dropout_refs.py at index row * d + c."""
import os

import numpy as np
import pytest
import torch

from tests import ln_row_refs as lr

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 2
ENV = "MTN_EMBED_DETERMINISTIC"
# hits of each entry of the V = 13 table: 0, 1, 6, 7, 24 (the last light count), 25 (the first heavy one), 200; the last workgroup
# owns entries 8 .. 12 only
COUNTS13 = (200, 0, 1, 6, 7, 24, 25, 0, 3, 0, 12, 1, 2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from mtn_amd import lib as L
    return L, L.load()


@pytest.fixture(scope="module")
def seed(dev):
    return torch.tensor([lr.SEED], dtype=torch.int64, device=dev)


def tokens_with_counts(counts, rng):
    """a shuffled token list in which entry v occurs exactly counts[v] times"""
    t = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(t)
    return t


def make_stream(table, tokens, d, emb_scale, p, salt, rng):
    rows = len(tokens)
    dx = (rng.standard_normal((rows, d)) * np.linspace(0.5, 1.5, d)).astype(np.float32)
    return dict(table=table, tokens=np.asarray(tokens, dtype=np.int64), dx=dx, emb_scale=float(np.float32(emb_scale)), p=p, salt=salt,
                keep=lr.keep2d(salt, p, rows, d) if p > 0 else None)


def make_table(V, d, rng):
    return rng.standard_normal((V, d)).astype(np.float32)          # the table already holds values: the kernels add into it


def _launch(L, lib, dev, seed, tables, streams, det):
    """One mtn_embed_bwd_group call -> the tables on the host (guard rows before and after each verified NaN)."""
    full = []
    for t in tables:
        f = torch.full((t.shape[0] + 2 * G, t.shape[1]), NAN, device=dev)
        f[G:G + t.shape[0]] = torch.from_numpy(t).to(dev)
        full.append(f)
    keep_alive, descs = [], (L.EmbedBwdDesc * len(streams))()
    for D, s in zip(descs, streams):
        tok, dx = torch.from_numpy(s["tokens"]).to(dev), torch.from_numpy(s["dx"]).to(dev)
        keep_alive += [tok, dx]
        D.rows, D.d, D.tokens, D.dx, D.emb_scale = s["dx"].shape[0], s["dx"].shape[1], tok.data_ptr(), dx.data_ptr(), s["emb_scale"]
        if s["p"] > 0:
            D.drop = L.Dropout(float(s["p"]), s["salt"], seed.data_ptr())
        D.dlut, D.lut_rows = full[s["table"]][G:].data_ptr(), tables[s["table"]].shape[0]
    old = os.environ.get(ENV)
    try:
        os.environ[ENV] = "1" if det else "0"
        L.reload_env()
        L.check(lib.mtn_embed_bwd_group(len(streams), descs, L.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old
        L.reload_env()                                       # later tests see the default again
    out = []
    for f, t in zip(full, tables):
        h = f.cpu()
        assert bool(torch.isnan(h[:G]).all()) and bool(torch.isnan(h[G + t.shape[0]:]).all()), "guard rows around the table written"
        out.append(h[G:G + t.shape[0]].numpy())
    return out


def _run_both(L, lib, dev, seed, tables, streams, expect_hits=None, what=""):
    """Both kernels inside the bound (the reference is computed once), rows no token names bit-unchanged, the deterministic kernel
    three times with the same bits."""
    refs = [lr.embed64(t, [s for s in streams if s["table"] == i]) for i, t in enumerate(tables)]
    if expect_hits is not None:
        for (_, _, hits), want in zip(refs, expect_hits):
            assert hits.tolist() == list(want), "the token list does not have the stated hit counts"
    worst = {}
    first = None
    for det, run in ((True, 0), (True, 1), (True, 2), (False, 0)):
        got = _launch(L, lib, dev, seed, tables, streams, det)
        for i, (t, g, (ref, bound, hits)) in enumerate(zip(tables, got, refs)):
            name = "deterministic" if det else "atomic"
            worst[name] = max(worst.get(name, 0.0), lr.assert_within(g, ref, bound, f"{what} table {i} ({name} kernel)"))
            untouched = hits == 0
            assert np.array_equal(g[untouched].view(np.int32), t[untouched].view(np.int32)), "a row no token names changed"
        if det and first is None:
            first = got
        elif det:
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first, got)), f"run {run}: other bits"
    print(f"{what}: worst |kernel - float64| / bound  " + " | ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("d", [4, 96, 512, 640])
def test_hit_counts_around_the_heavy_threshold(dev, hip, seed, d, p):
    """V = 13 (no multiple of 8) with entries of exactly 0, 1, 6, 7, 24, 25 and 200 hits, dropout on; d = 640 takes the second
    512-column pass, where the mask index row * d + c needs the absolute column."""
    L, lib = hip
    rng = np.random.default_rng(1000 + d)
    s = make_stream(0, tokens_with_counts(COUNTS13, rng), d, np.sqrt(d), p, 0x51 + d, rng)
    _run_both(L, lib, dev, seed, [make_table(13, d, rng)], [s], expect_hits=[COUNTS13], what=f"d {d} p {p}")


def test_three_streams_on_one_table(dev, hip, seed):
    """rows = 70, 1 and 210 on one table, each with its own emb_scale, p and salt: both stream boundaries (70, 71) fall inside the
    second 64-token ballot.  The hit counts are those of COUNTS13, dealt over the three streams."""
    L, lib = hip
    rng = np.random.default_rng(7)
    tok = tokens_with_counts(COUNTS13, rng)
    assert len(tok) == 281
    d = 96
    streams = [make_stream(0, tok[:70], d, 2.0, 0.1, 0x61, rng), make_stream(0, tok[70:71], d, 0.75, 0.5, 0x62, rng),
               make_stream(0, tok[71:], d, 9.5, 0.0, 0x63, rng)]
    _run_both(L, lib, dev, seed, [make_table(13, d, rng)], streams, expect_hits=[COUNTS13], what="three streams")


@pytest.mark.parametrize("total", [lr.EMB_CH, lr.EMB_CH + 1])
def test_chunk_boundary(dev, hip, seed, total):
    """8192 tokens stay resident in LDS, 8193 are restaged for every column pass and every heavy entry.  Entry 7 has exactly 25 hits,
    the last 25 tokens of the list: with 8193 tokens its last hit is token 8192, alone in the second chunk.  Two streams (5000 rows, the
    rest), d = 640 (two column passes), V = 1000; the other entries share the remaining tokens (8 or 9 hits each: light)."""
    L, lib = hip
    rng = np.random.default_rng(total)
    V, d = 1000, 640
    others = np.array([v for v in range(V) if v != 7])
    tok = np.concatenate([others[np.arange(total - 25) % len(others)], np.full(25, 7)])
    rng.shuffle(tok[:total - 25])
    want = np.bincount(tok, minlength=V)
    assert want[7] == 25 and want.max() == 25 and len(tok) == total and (total == lr.EMB_CH or tok[lr.EMB_CH] == 7)
    streams = [make_stream(0, tok[:5000], d, 1.5, 0.1, 0x71, rng), make_stream(0, tok[5000:], d, 0.5, 0.5, 0x72, rng)]
    _run_both(L, lib, dev, seed, [make_table(V, d, rng)], streams, expect_hits=[want], what=f"{total} tokens")


def test_two_tables_in_one_launch(dev, hip, seed):
    """V = 13 with d = 640 and V = 300 with d = 96 in one launch (the grid covers the longer table; the shorter one's surplus
    workgroups leave), streams of the two tables interleaved."""
    L, lib = hip
    rng = np.random.default_rng(11)
    t13 = tokens_with_counts(COUNTS13, rng)
    c300 = np.zeros(300, dtype=np.int64)
    c300[[0, 5, 17, 150, 298, 299]] = (30, 1, 24, 25, 7, 2)
    t300 = tokens_with_counts(c300, rng)
    streams = [make_stream(1, t300[:40], 96, 3.0, 0.1, 0x81, rng), make_stream(0, t13[:100], 640, 1.0, 0.5, 0x82, rng),
               make_stream(1, t300[40:], 96, 0.5, 0.0, 0x83, rng), make_stream(0, t13[100:], 640, 2.0, 0.1, 0x84, rng)]
    _run_both(L, lib, dev, seed, [make_table(13, 640, rng), make_table(300, 96, rng)], streams, expect_hits=[COUNTS13, c300], what="two tables")


def test_argument_checks(dev, hip, seed):
    """Streams of one table that disagree on its shape, d % 4 != 0, a count of 9: MtnHipError, nothing launched."""
    L, lib = hip
    rng = np.random.default_rng(3)
    table = make_table(13, 8, rng)
    tok = tokens_with_counts((2,) * 13, rng)

    def expect_error(streams, tables, mutate=None, count=None):
        full = [torch.full(t.shape, NAN, device=dev) for t in tables]
        keep_alive, descs = [], (L.EmbedBwdDesc * max(len(streams), count or 0))()
        for D, s in zip(descs, streams):
            t_, x_ = torch.from_numpy(s["tokens"]).to(dev), torch.from_numpy(s["dx"]).to(dev)
            keep_alive += [t_, x_]
            D.rows, D.d, D.tokens, D.dx, D.emb_scale = len(s["tokens"]), s["dx"].shape[1], t_.data_ptr(), x_.data_ptr(), 1.0
            D.dlut, D.lut_rows = full[s["table"]].data_ptr(), s.get("lut_rows", tables[s["table"]].shape[0])
        if mutate:
            mutate(descs)
        L.reload_env()
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_embed_bwd_group(count or len(streams), descs, L.stream_ptr()))
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(f).all()) for f in full)

    a, b = make_stream(0, tok[:10], 8, 1.0, 0.0, 0, rng), make_stream(0, tok[10:], 8, 1.0, 0.0, 0, rng)
    expect_error([a, dict(b, lut_rows=12)], [table])                               # one table, two vocabulary sizes
    expect_error([a, dict(b, dx=np.zeros((len(b["tokens"]), 4), dtype=np.float32))], [table])    # one table, two widths
    expect_error([dict(a, dx=np.zeros((10, 6), dtype=np.float32))], [table])       # d % 4 != 0
    expect_error([a], [table], count=9)
    expect_error([a], [table], mutate=lambda D: setattr(D[0], "tokens", 0))
    expect_error([a], [table], mutate=lambda D: setattr(D[0], "rows", 0))
