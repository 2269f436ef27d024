"""Minimum-Bayes-risk selection through mtn_amd.decode on the GPU: decode.mbr_rerank against tests/mbr_refs.py for both weight modes, and
sample_decode_many(mbr=N) on the small model of the sampling tests — the selection changes no draw, its order and expected utilities are
the definition applied to the search's own token log, and on bf16 it rides in the one captured sampling graph of the persistent step."""
import random

import pytest
import torch

from tests import mbr_refs as R

pytestmark = pytest.mark.gpu


def _lists(seed, sizes, max_len, n_values):
    rng = random.Random(seed)
    return [[(h, -rng.random() * 12.0) for h in R.random_set(rng, k, max_len, n_values)] for k in sizes]


@pytest.mark.parametrize("weights,temperature", [("uniform", 1.0), ("score", 1.0), ("score", 0.35)])
def test_mbr_rerank_equals_the_definition(weights, temperature):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import decode as D
    lists = _lists(3, [16, 5, 0, 1, 9, 16], 30, 12)
    lists[1][2] = ([], lists[1][2][1])                                            # an empty hypothesis
    lists[4][7] = (list(lists[4][1][0]), lists[4][7][1])                          # a duplicate
    got = D.mbr_rerank(lists, 4, weights=weights, temperature=temperature)
    assert len(got) == len(lists)
    moved = 0
    for l, g in zip(lists, got):
        w = R.score_weights([s for _, s in l], temperature) if weights == "score" and l else None
        _, expected, best, order = R.select([h for h, _ in l], 4, w)
        assert g == [(l[j][0], l[j][1], float(expected[j])) for j in order.tolist()]
        moved += bool(l) and best != 0
    assert moved >= 1
    if weights == "score":
        assert D.mbr_weights([s for _, s in lists[0]], temperature) == R.score_weights([s for _, s in lists[0]], temperature)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_sample_decode_many_selects_in_the_search(dtype):
    from mtn_amd import decode as D
    from mtn_amd import make_model
    from mtn_amd.synthetic import CONFIGS, synthetic_batch
    dev = torch.device("cuda:0")
    cfg = dict(CONFIGS["cfg2"])
    torch.manual_seed(4)
    model = make_model(cfg["vocab"], cfg["vocab"], N=2, d_model=cfg["d_model"], d_ff=cfg["d_ff"], h=cfg["h"], dropout=0.1,
                       ft_sizes=cfg["ft_sizes"], diff_encoder=True, auto_encoder_ft="query",
                       compute_dtype=torch.bfloat16 if dtype == "bf16" else torch.float32).to(dev).eval()
    b = synthetic_batch(cfg["vocab"], 2, cfg["Q"], cfg["H"], cfg["C"], cfg["T"], cfg["frames"], cfg["ft_sizes"], device=dev, seed=500, ragged=True)
    eos, S, N, L = 3, 4, 2, 12
    search = lambda **kw: D.sample_decode_many(model, b, L, 2, eos, 1, samples=S, temperature=0.9, top_k=4, seed=3, banned=(0, 1, 2), penalty=1.0, **kw)
    D._SESSIONS.clear()
    fallbacks = D.MegaDecodeSession.FALLBACKS
    plain_trace, trace = [], []
    plain = search(trace=plain_trace)
    got = search(trace=trace, mbr=N)
    assert plain_trace[0][0] == trace[0][0]
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(plain_trace[0][1:], trace[0][1:]))      # the selection changes no draw
    hyps = R.cut_log(trace[0][1], eos)
    assert len(got) == 2
    for d in range(2):
        mine = hyps[d * S:d * S + S]
        _, expected, _, order = R.select(mine, N)
        assert [t for t, _, _ in got[d]] == [mine[j] for j in order.tolist()]
        assert [e for _, _, e in got[d]] == [float(expected[j]) for j in order.tolist()]
        assert sorted((t, s) for t, s, _ in got[d]) == sorted(plain[d])               # the same hypotheses with the same scores
        assert all(len(h) == 2 for h in plain[d])                                    # mbr = 0 returns today's pairs
    assert search(mbr=N) == got
    mega = [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.MegaDecodeSession)]
    if dtype == "bf16":
        assert len(mega) == 1 and hasattr(mega[0], "_sample_graph") and mega[0]._sample_key[-1] == N, "bf16 must sample on the persistent step"
        graph = mega[0]._sample_graph
        assert search(mbr=N) == got and mega[0]._sample_graph is graph              # one graph serves every search of the shape
        assert D.MegaDecodeSession.FALLBACKS == fallbacks
    else:
        assert not mega
    D._SESSIONS.clear()
