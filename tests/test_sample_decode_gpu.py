"""`generate.py --decode-style sample` on the GPU, end to end, on the mini AVSD fixture and the one-epoch checkpoint of
test_generate_gpu.py: reproducible per seed, arg-max at --top-k 1, and every sampled token admissible for ITS OWN random number
u(seed, qa_id * S + s, position) on the log-probabilities of a single-QA, unpadded pass — whatever the bucket, D or padding."""
import json
import logging
import os
import time

import numpy as np
import pytest
import torch

from tests import sample_refs as R
from tests.test_generate_gpu import MAXLEN, PENALTY, _argv, _logged_hyps, _reference_side, run  # noqa: F401  (run: the module's fixture)

pytestmark = pytest.mark.gpu
T, TOP_K, TOP_P = 0.9, 20, 0.9


def _sample_argv(run, dtype, out, seed, samples=1, extra=(), t=T, top_k=TOP_K, top_p=TOP_P):
    return _argv(run, "sample", dtype, 0, out) + ["--temperature", str(t), "--top-k", str(top_k), "--top-p", str(top_p), "--samples", str(samples),
                                                 "--sample-seed", str(seed)] + list(extra)


def _main(run, caplog, argv):
    from mtn_amd import generate as G
    caplog.clear()
    caplog.set_level(logging.INFO)
    result = G.main(argv)
    return result, _logged_hyps(caplog.records)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_same_seed_same_result_and_another_seed_another(run, dtype, caplog):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    fallbacks = D.MegaDecodeSession.FALLBACKS
    out = str(run["tmp"] / f"sample_{dtype}.json")
    a, log_a = _main(run, caplog, _sample_argv(run, dtype, out, 5, samples=2))
    assert json.load(open(out)) == a
    mega = [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.MegaDecodeSession)]
    b, log_b = _main(run, caplog, _sample_argv(run, dtype, out, 5, samples=2))
    c, log_c = _main(run, caplog, _sample_argv(run, dtype, out, 6, samples=2))
    assert a == b and log_a == log_b
    assert a != c and log_a != log_c
    assert all(len(h) == 2 and h[0][1] >= h[1][1] for h in log_a)                 # one HYP line per sample, best first
    answers = [t["answer"] for d in a["dialogs"] for t in d["dialog"]]
    assert answers == [h[0][0] for h in log_a]
    if dtype == "bf16":
        assert mega and all(hasattr(s, "_sample_graph") for s in mega), "bf16 at d_model 128 must sample on the persistent step"
        assert D.MegaDecodeSession.FALLBACKS == fallbacks
    else:
        assert not mega


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_top_k_one_is_greedy(run, dtype, caplog):
    out = str(run["tmp"] / f"sample_k1_{dtype}.json")
    greedy, _ = _main(run, caplog, _argv(run, "greedy", dtype, 0, out))
    k1, _ = _main(run, caplog, _sample_argv(run, dtype, out, 3, top_k=1))
    t0, _ = _main(run, caplog, _sample_argv(run, dtype, out, 4, t=0.0, top_k=0, top_p=1.0))       # temperature 0 = top_k 1
    assert k1 == greedy and t0 == greedy


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("plan", ["buckets", "no-buckets", "one-per-search"])
def test_fp32_tokens_are_admissible_on_a_single_qa_pass(run, plan, samples, caplog, monkeypatch):
    """Path-independent admissibility (eps = 1e-3, the project's fp32 parity bar): the sampled prefix of every (QA, sample) replayed
    through a single-QA unpadded DecodeSession.step; every token in admissible(row, u(seed, qa_id * S + s, position)).  And the logged
    scores are sum(logp) + penalty * (len + 1), recomputed from the search's own log."""
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    seed, S = 9, samples
    traces = []
    real = D.sample_decode_many
    monkeypatch.setattr(D, "sample_decode_many", lambda *a, **k: real(*a, **dict(k, trace=traces)))
    extra = {"buckets": [], "no-buckets": ["--no-buckets"], "one-per-search": ["--dialogues-per-search", "1"]}[plan]
    out = str(run["tmp"] / f"sample_adm_{plan}_{S}.json")
    D._SESSIONS.clear()
    _, logged = _main(run, caplog, _sample_argv(run, "fp32", out, seed, samples=S, extra=extra))
    monkeypatch.undo()

    vocab, targs, data, corpus, model, _ = _reference_side(run, "fp32", False)
    sos, eos, unk, pad = vocab["<sos>"], vocab["<eos>"], vocab["<unk>"], vocab["<blank>"]
    prm = R.Params(T, TOP_K, TOP_P, banned=(unk, pad, sos), eos=eos, min_len=1)
    n_qa = len(data["dialogs"])
    idx, _ = dh.make_batch_indices(data, 1, separate_caption=True)
    by_key = {}
    for keys, tok, lp, u in traces:
        for r, k in enumerate(keys):
            by_key.setdefault(k, (tok[:, r], lp[:, r], u[:, r]))                  # (padding copies repeat a key: same stream)
    assert sorted(by_key) == list(range(n_qa * S))
    checked, worst = 0, 0.0
    for qa in range(n_qa):
        sess = D.DecodeSession(model, dh.make_batch(corpus, idx[qa], vocab, separate_caption=True), MAXLEN, 1, pad=pad, use_graph=False)
        scores = []
        for s in range(S):
            tok, lp, u = by_key[qa * S + s]
            prefix = [sos]
            for l in range(MAXLEN):
                want_u = float(R.uniform24(seed, qa * S + s, l))
                assert float(u[l]) == want_u, (qa, s, l)
                row = sess.step([prefix])[0].double().cpu().numpy()
                assert int(tok[l]) in R.admissible(row, want_u, prm, 1e-3, position=l), (qa, s, l, int(tok[l]))
                worst = max(worst, abs(float(lp[l]) - row[int(tok[l])]))
                checked += 1
                prefix.append(int(tok[l]))
                if tok[l] == eos:
                    break
            ended = prefix[-1] == eos
            n = len(prefix) - 2 if ended else MAXLEN - 1                             # tokens of the response (at most max_len - 1)
            scores.append(float(lp[:n + 1 if ended else n].astype(np.float64).sum()) + PENALTY * (n + 1))
        got = [sc for _, sc in logged[qa]]
        assert len(got) == S and np.allclose(sorted(scores, reverse=True), got, atol=2e-6, rtol=0), (qa, scores, got)
    print(f"{plan}, S = {S}: {checked} tokens admissible; logged log-probabilities within {worst:.2e} of the single-QA pass")
    assert worst < 1e-3


def _stream_beside_the_current_one(L, dev):
    """A side stream whose kernels run BESIDE the current stream's.  The runtime deals its streams onto a few hardware queues, and two
    streams on one queue take turns: a holder launched there would only delay the search, not take compute units from under it.  So a
    20 ms holder goes to a candidate stream, one tiny kernel to the current one: when that returns before the holder is through, the
    two overlap.  Consecutive streams of the pool sit on different queues, so one of the first few does."""
    probe = torch.zeros(64, device=dev)
    probe.add_(1)
    for _ in range(8):
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.check(L.load().mtn_debug_hold_cus(128, 150 * 1024, 20000, L.stream_ptr()))
        t0 = time.time()
        probe.add_(1)
        torch.cuda.current_stream().synchronize()
        dt = time.time() - t0
        torch.cuda.synchronize()
        if dt < 0.010:
            return side
    pytest.fail("no stream of the pool runs beside the current one")


def test_sampling_falls_back_when_compute_units_are_taken():
    """The sampling twin of test_decode_gpu's provoked timeout, once: 128 compute units held on a second stream while a sampling search
    starts — its persistent step times out, the search re-runs on the launch-per-sublayer pass (FALLBACKS counts it) and returns that
    pass's own samples; afterwards the same session samples on the persistent step as before."""
    from mtn_amd import decode as D
    from mtn_amd import lib as L
    from mtn_amd import make_model
    from mtn_amd.synthetic import CONFIGS, synthetic_batch
    dev = torch.device("cuda:0")
    cfg = dict(CONFIGS["cfg2"])
    torch.manual_seed(4)
    model = make_model(cfg["vocab"], cfg["vocab"], N=2, d_model=cfg["d_model"], d_ff=cfg["d_ff"], h=cfg["h"], dropout=0.1,
                       ft_sizes=cfg["ft_sizes"], diff_encoder=True, auto_encoder_ft="query", compute_dtype=torch.bfloat16).to(dev).eval()
    b = synthetic_batch(cfg["vocab"], 1, cfg["Q"], cfg["H"], cfg["C"], cfg["T"], cfg["frames"], cfg["ft_sizes"], device=dev, seed=500, ragged=True)
    search = lambda: D.sample_decode_many(model, b, 12, 2, 3, 1, samples=4, temperature=0.9, top_k=30, seed=3, banned=(0, 1, 2), penalty=1.0)
    D._SESSIONS.clear()
    clean = search()
    sess = [s_[0] for s_ in D._SESSIONS.values() if isinstance(s_[0], D.MegaDecodeSession)]
    assert len(sess) == 1 and not sess[0].timed_out()
    os.environ["MTN_DECODE_MEGA"] = "0"
    try:
        launch = search()
    finally:
        del os.environ["MTN_DECODE_MEGA"]
    before = D.MegaDecodeSession.FALLBACKS
    side = _stream_beside_the_current_one(L, dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        L.check(L.load().mtn_debug_hold_cus(128, 150 * 1024, 600000, L.stream_ptr()))
    time.sleep(0.05)
    held = search()
    assert D.MegaDecodeSession.FALLBACKS == before + 1, "the persistent step did not time out (were 128 compute units really held?)"
    assert held == launch
    torch.cuda.synchronize()
    again = search()
    assert D.MegaDecodeSession.FALLBACKS == before + 1 and not sess[0].timed_out()
    assert again == clean
    assert len(clean) == 1 and len(clean[0]) == 4 and all(clean[0][i][1] >= clean[0][i + 1][1] for i in range(3))
    D._SESSIONS.clear()
