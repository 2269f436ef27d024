"""--cut-a on the device: batch assembly with the reference's random answer truncation (data_handler.py:255-260) against the
REFERENCE's own outputs (tests/golden/cut_a.npz, tools/make_cut_a_golden.py), the captured-graph corpus loop with cutting
against the eager loop, and train.main with run.sh's flags plus --cut-a 1.  Integer / copy work: bit-exact."""
import json
import logging
import os
import random
import re

import numpy as np
import pytest
import torch

from oracle import fixtures as fx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = fx.load_golden(os.path.join(HERE, "golden", "cut_a.npz"))
CASES = [(cap, bsz, mlen, seed) for cap in (True, False) for bsz, mlen in ((4, 8), (6, 20)) for seed in (1, 7)]


def _plan(cap, bsz, mlen):
    from mtn_amd.data_handler import make_batch_indices
    data = fx.det_corpus(caption=cap)
    idx, _ = make_batch_indices(data, batchsize=bsz, max_length=mlen, separate_caption=cap)
    return data, idx


def _state(rs):
    _, keys, pos, has_gauss, gauss = rs.get_state()
    return keys.tolist(), pos, [has_gauss, gauss]


@pytest.mark.gpu
@pytest.mark.parametrize("cap,bsz,mlen,seed", CASES)
def test_device_cut_assembly_matches_reference(cap, bsz, mlen, seed):
    """Fresh batches and batches refilled in place (out=) on revisits: trg, trg_y, trg_mask, ntokens equal the reference's."""
    from mtn_amd.data_handler import DeviceCorpus, make_batch
    data, idx = _plan(cap, bsz, mlen)
    corpus = DeviceCorpus(data, "cuda:0")
    tag = f"cap{int(cap)}.b{bsz}.s{seed}"
    want_state = (GOLD[f"{tag}.state_keys"].tolist(), int(GOLD[f"{tag}.state_pos"]), GOLD[f"{tag}.state_gauss"].tolist())
    for refill in (False, True):
        rs, made = np.random.RandomState(seed), {}
        for v, k in enumerate(GOLD[f"{tag}.visits"].tolist()):
            reuse = made.get(k) if refill else None
            b = make_batch(corpus, idx[k], data["vocab"], separate_caption=cap, out=reuse, cut_a=True, rng=rs)
            if refill:
                assert reuse is None or b is reuse
                made[k] = b
            torch.cuda.synchronize()
            for name in ("trg", "trg_y", "trg_mask"):
                have, want = getattr(b, name).cpu().numpy(), GOLD[f"{tag}.{v}.{name}"]
                assert have.shape == want.shape and have.dtype == want.dtype and np.array_equal(have, want), (refill, v, name)
            assert int(b.ntokens) == int(GOLD[f"{tag}.{v}.ntokens"]), (refill, v)
        assert _state(rs) == want_state


@pytest.mark.gpu
@pytest.mark.parametrize("cap,bsz,mlen", [(True, 4, 8), (False, 6, 20)])
def test_cut_probability_zero_is_todays_batch(cap, bsz, mlen):
    """cut_a=True with cut_a_p=0 passes a row_len of all -1: every tensor equals the uncut (row_len NULL) batch."""
    from mtn_amd.data_handler import DeviceCorpus, make_batch
    data, idx = _plan(cap, bsz, mlen)
    corpus = DeviceCorpus(data, "cuda:0")
    rs = np.random.RandomState(0)
    names = ["query", "his", "trg", "trg_y", "query_mask", "his_mask", "trg_mask", "trg_pad_u8", "trg_y_pad_u8"]
    names += ["cap", "cap_mask"] if cap else []
    for ix in idx:
        a = make_batch(corpus, ix, fx.PAD, separate_caption=cap)
        b = make_batch(corpus, ix, fx.PAD, separate_caption=cap, cut_a=True, cut_a_p=0.0, rng=rs)
        for name in names:
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert int(a.ntokens) == int(b.ntokens)
        for f1, f2, m1, m2 in zip(a.fts, b.fts, a.fts_mask, b.fts_mask):
            assert torch.equal(f1, f2) and torch.equal(m1, m2)


@pytest.mark.gpu
def test_bucketed_graph_trainer_with_cuts_matches_eager_loop():
    """BucketedTrainer.step(cut_a=True) on the setup of test_bucketed_graph_trainer_matches_eager_loop: every refilled static
    batch equals a freshly assembled one with the same draws, and the losses follow the eager loop fed the same draws."""
    from mtn_amd import make_model, LabelSmoothing, NoamOpt, FusedAdam, SimpleLossCompute
    from mtn_amd.data_handler import DeviceCorpus, draw_cuts, make_batch, make_batch_indices
    from mtn_amd.train_step import BucketedTrainer
    data = fx.det_corpus(n_videos=12, turns=4, vocab=64, ft_sizes=(32, 16), seed=3)
    idx, _ = make_batch_indices(data, batchsize=6, max_length=20, separate_caption=True)
    corpus = DeviceCorpus(data, "cuda:0")

    def model():
        torch.manual_seed(0)
        return make_model(64, 64, N=2, d_model=64, d_ff=128, h=4, dropout=0.0, ft_sizes=[32, 16], diff_encoder=True, auto_encoder_ft="query",
                          compute_dtype="bf16", attn_dropout=0.0).to("cuda:0").train()

    order = [0, 3, 1, 0, 2, 3, 1] if len(idx) > 3 else list(range(len(idx))) * 2
    seed = 4
    replay = np.random.RandomState(seed)
    cut_rows = sum(int((draw_cuts(corpus.answer_lengths(), idx[k][1], 0.5, replay) >= 0).sum()) for k in order)
    assert cut_rows > 0
    m1 = model()
    tr = BucketedTrainer(m1, corpus, 64, pad=fx.PAD, warmup=50, bucket=4)
    rs, rs_fresh = np.random.RandomState(seed), np.random.RandomState(seed)
    graphed = []
    for k in order:
        loss, b = tr.step(idx[k], cut_a=True, rng=rs)
        graphed.append(float(loss))
        fresh = make_batch(corpus, tr._padded(idx[k]), fx.PAD, separate_caption=True, cut_a=True, rng=rs_fresh)
        for name in ("query", "his", "cap", "trg", "trg_y", "query_mask", "his_mask", "cap_mask", "trg_mask"):
            assert torch.equal(getattr(b, name), getattr(fresh, name)), name
        assert int(b.ntokens) == int(fresh.ntokens)
        for f1, f2, k1, k2 in zip(b.fts, fresh.fts, b.fts_mask, fresh.fts_mask):
            assert torch.equal(f1, f2) and torch.equal(k1, k2)
    assert _state(rs) == _state(replay)                      # one draw set per step, on the capture and the refill branch alike
    m2 = model()
    lc = SimpleLossCompute(m2.generator, m2.auto_encoder_generator, LabelSmoothing(64, fx.PAD, 0.1),
                           opt=NoamOpt(64, 1, 50, FusedAdam(m2)), sync=False)
    rs2 = np.random.RandomState(seed)
    eager = []
    for k in order:
        b = make_batch(corpus, idx[k], fx.PAD, separate_caption=True, cut_a=True, rng=rs2)
        out, ae_out = m2.forward(b)
        eager.append(float(lc(out, b.trg_y, b.ntokens, ae_out, b.query, (b.query != fx.PAD).sum())) / float(b.ntokens))
    assert max(abs(a - e) / abs(e) for a, e in zip(graphed, eager)) < 2e-2, (graphed, eager)


def _features(tmp_path, raw):
    rs = np.random.RandomState(3)
    dims = {"i3d": 12, "vgg": 5}
    for ft, F in dims.items():
        os.makedirs(tmp_path / ft, exist_ok=True)
        for d in raw["dialogs"]:
            np.save(tmp_path / ft / (d["image_id"] + ".npy"), rs.randn(rs.randint(3, 9), F).astype(np.float32))
    return str(tmp_path / "<FeaType>" / "<ImageID>.npy")


def _epoch_tokens(caplog):
    got = {}
    for r in caplog.records:
        m = re.match(r"epoch (\d+): (\d+) target tokens trained", r.getMessage())
        if m:
            got[int(m.group(1))] = int(m.group(2))
    return got


@pytest.mark.gpu
def test_run_sh_style_training_with_cut_a(tmp_path, caplog):
    """train.main with run.sh's data flags plus --cut-a 1 on the mini annotation file, two epochs with validation: finite
    losses, and epoch 1's logged target tokens equal a host replay of the plan's draws (captured-graph loop and --eager alike)
    and are fewer than with --cut-a 0."""
    from mtn_amd import data_handler as dh
    from mtn_amd import train
    jpath = os.path.join(HERE, "golden", "mini_avsd.json")
    fea_path = _features(tmp_path, json.load(open(jpath)))
    base = ["--fea-type", "i3d", "vgg", "--train-path", fea_path, "--train-set", jpath, "--valid-path", fea_path, "--valid-set", jpath,
            "--num-epochs", "2", "--batch-size", "4", "--max-length", "256", "--include-caption", "caption,summary",
            "--separate-caption", "1", "--max-history-length", "3", "--nb-blocks", "1", "--d-model", "64", "--d-ff", "128",
            "--att-h", "4", "--dropout", "0.1", "--warmup-steps", "20", "--report-interval", "1000", "--rand-seed", "1"]
    counts = {}
    for cut, extra in ((1, []), (0, []), ("eager", ["--eager"])):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            means = train.main(base + ["--cut-a", "0" if cut == 0 else "1"] + extra)
        assert len(means) == 2 and all(np.isfinite(means)) and all(m > 0 for m in means), means
        counts[cut] = _epoch_tokens(caplog)
        assert sorted(counts[cut]) == [1, 2], counts
    # host replay: the plan train.main makes, visited in its shuffled order, the draws of RandomState(--rand-seed)
    vocab = dh.get_vocabulary(jpath, include_caption="caption,summary")
    data = dh.load(["i3d", "vgg"], fea_path, jpath, vocab, include_caption="caption,summary", separate_caption=True,
                   max_history_length=3, merge_source=False)
    idx, _ = dh.make_batch_indices(data, batchsize=4, max_length=256, separate_caption=True)
    by_id = sorted(data["dialogs"], key=lambda d: d[1])
    ans_len = np.array([len(d[4]) for d in by_id], dtype=np.int32)
    order = list(range(len(idx)))
    random.Random(1).shuffle(order)
    rs = np.random.RandomState(1)
    cut_tokens = full_tokens = 0
    for k in order:
        row_len = dh.draw_cuts(ans_len, idx[k][1], 0.5, rs)
        for q, e in zip(idx[k][1], row_len):
            y = np.asarray(by_id[q][5])
            cut_tokens += int((y[:e if e >= 0 else len(y)] != 1).sum())
            full_tokens += int((y != 1).sum())
    assert counts[0][1] == full_tokens
    assert counts[1][1] == cut_tokens < full_tokens, (counts, cut_tokens, full_tokens)
    assert counts["eager"][1] == cut_tokens                   # the eager loop (--eager) draws the same cuts
