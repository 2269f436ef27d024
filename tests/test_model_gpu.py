"""GPU parity of the fused sublayers and of the whole model (forward, loss, gradients, optimiser steps, DP math)
against the CPU oracle and the committed golden outputs of the reference (tests/golden, made by oracle/make_golden.py).

Tolerances (BASELINE.json north_star): 1e-3 in fp32 mode, 1e-2 in bf16 mode, both as max|err| / max|ref| per tensor."""
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import mtn_oracle as orc
from tests.util import DTYPES, TOL, absmax, relmax

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def build_model(c, dtype, dev, dropout=0.0, attn_dropout=0.0, seed=0):
    """mtn_amd model loaded with the deterministic fixture weights."""
    from mtn_amd import make_model
    m = make_model(c["vocab"], c["vocab"], N=c["N"], d_model=c["d_model"], d_ff=c["d_ff"], h=c["h"], dropout=dropout,
                   ft_sizes=c["ft_sizes"], diff_encoder=c["diff_encoder"], diff_embed=c["diff_embed"], diff_gen=c["diff_gen"],
                   auto_encoder_ft=c["auto_encoder_ft"], compute_dtype=dtype, attn_dropout=attn_dropout)
    sd = fx.det_state_dict(fx.state_shapes(**c), seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    return m.to(dev)


def dev_batch(raw, dev):
    from mtn_amd import Batch
    t = torch.from_numpy
    return Batch(t(raw["query"]), t(raw["his"]), None, [t(f) for f in raw["fts"]], t(raw["cap"]), t(raw["trg"]), t(raw["trg_y"]),
                 pad=fx.PAD, device=dev)


def raw_batch(c, seed=1, **kw):
    return fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=seed, **kw)


# ------------------------------------------------------------------------------------------ fused sublayers
# The three ways a single sublayer delivers its parameter gradients (ops.MHASublayerFn / FFNSublayerFn): returned through autograd,
# written at once into fp32 destinations, deferred through a ParamGradQueue into the same destinations.
DELIVERY = ["returned", "written", "queued"]


def _delivery(ops, mode, params):
    """params: name -> device parameter.  -> (cfg.grads, cfg.queue, collect): collect() = name -> the delivered gradient.  The
    destinations start as NaN: a gradient that is never written fails the comparison."""
    if mode == "returned":
        return None, None, lambda: {k: p.grad for k, p in params.items()}
    dests = {k: torch.full_like(p, float("nan"), requires_grad=False) for k, p in params.items()}

    def collect():
        assert all(p.grad is None for p in params.values()), "a gradient went through autograd although a destination was set"
        return dests
    return dests, (ops.ParamGradQueue() if mode == "queued" else None), collect


@pytest.mark.parametrize("mode", DELIVERY)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cross", [False, True])
def test_mha_sublayer_fwd_bwd(dev, dtype, cross, mode):
    from mtn_amd import ops
    B, a, m, d, h = 3, 20, 37 if cross else 20, 128, 4
    g = torch.Generator().manual_seed(11 + cross)
    x = torch.randn(B, a, d, generator=g)
    mem = torch.randn(B, m, d, generator=g) if cross else None
    ln_a, ln_b = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    w = [torch.randn(d, d, generator=g) * d ** -0.5 for _ in range(4)]
    b = [0.1 * torch.randn(d, generator=g) for _ in range(4)]
    gy = torch.randn(B, a, d, generator=g)
    if cross:
        lens = torch.randint(1, m + 1, (B,), generator=g)
        mask = (torch.arange(m).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1)
        mask[1] = False
    else:
        mask = orc.make_std_mask(torch.randint(0, 3, (B, a), generator=g), 1)
    # oracle
    leaves = [t.clone().requires_grad_() for t in [x, ln_a, ln_b] + w + b + ([mem] if cross else [])]
    xr, ar, br = leaves[:3]
    wr, bbr = leaves[3:7], leaves[7:11]
    xn = orc.layer_norm(xr, ar, br)
    kv = leaves[11] if cross else xn
    yr = xr + orc.multi_head_attention(xn, kv, kv, mask, wr, bbr, h)
    yr.backward(gy)
    # HIP
    D = lambda t: t.to(dev).requires_grad_()
    xd, ad, bd = D(x), D(ln_a), D(ln_b)
    wqkv, bqkv = D(torch.cat(w[:3], 0)), D(torch.cat(b[:3], 0))
    wo, bo = D(w[3]), D(b[3])
    memd = D(mem) if cross else None
    grads, queue, collect = _delivery(ops, mode, dict(ln_a=ad, ln_b=bd, w_qkv=wqkv, b_qkv=bqkv, w_o=wo, b_o=bo))
    cfg = ops.MhaConfig(heads=h, lp_dtype=dtype, grads=grads, queue=queue)
    y = ops.MHASublayerFn.apply(xd, memd, None, mask.to(dev), ad, bd, wqkv, bqkv, wo, bo, cfg)
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    G = collect()
    tol = TOL[dtype]
    assert relmax(y, yr) < tol
    assert relmax(xd.grad, xr.grad) < tol * 2
    assert relmax(G["ln_a"], ar.grad) < tol * 2 and relmax(G["ln_b"], br.grad) < tol * 2
    assert relmax(G["w_qkv"], torch.cat([t.grad for t in wr[:3]], 0)) < tol * 2
    assert relmax(G["b_qkv"], torch.cat([t.grad for t in bbr[:3]], 0)) < tol * 2
    assert relmax(G["w_o"], wr[3].grad) < tol * 2 and relmax(G["b_o"], bbr[3].grad) < tol * 2
    if cross:
        assert relmax(memd.grad, leaves[11].grad) < tol * 2


class _RoundLP(torch.autograd.Function):
    """Straight-through rounding to the compute dtype in forward AND backward: lets the fp32 oracle see the operands the
    bf16 kernels see, so gradients can be compared tightly (bf16 rounding of an intermediate can be amplified by the
    LayerNorm backward projection, which is inherent to bf16 and not a kernel property)."""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.to(dtype).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).float(), None


@pytest.mark.parametrize("mode", DELIVERY)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ffn_sublayer_fwd_bwd(dev, dtype, mode):
    from mtn_amd import ops
    rows, d, ff = 70, 128, 512
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, rows // 2, d, generator=g)
    ln_a, ln_b = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    w1, b1 = torch.randn(ff, d, generator=g) * d ** -0.5, 0.1 * torch.randn(ff, generator=g)
    w2, b2 = torch.randn(d, ff, generator=g) * ff ** -0.5, 0.1 * torch.randn(d, generator=g)
    gy = torch.randn_like(x)
    leaves = [t.clone().requires_grad_() for t in (x, ln_a, ln_b, w1, b1, w2, b2)]
    rnd = lambda t: _RoundLP.apply(t, dtype)
    xn = rnd(orc.layer_norm(leaves[0], leaves[1], leaves[2]))
    hid = rnd(torch.relu(orc.linear(xn, rnd(leaves[3]), leaves[4])))
    yr = leaves[0] + orc.linear(hid, rnd(leaves[5]), leaves[6])
    yr.backward(gy)
    y_exact = x + orc.feed_forward(orc.layer_norm(x, ln_a, ln_b), w1, b1, w2, b2)
    dl = [t.to(dev).requires_grad_() for t in (x, ln_a, ln_b, w1, b1, w2, b2)]
    names = ("ln_a", "ln_b", "w1", "b1", "w2", "b2")
    grads, queue, collect = _delivery(ops, mode, dict(zip(names, dl[1:])))
    y = ops.FFNSublayerFn.apply(*dl, ops.FfnConfig(lp_dtype=dtype, grads=grads, queue=queue))
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    G = collect()
    tol = TOL[dtype]
    assert relmax(y, y_exact) < tol               # forward output vs the exact fp32 oracle
    for t, r in zip([dl[0].grad] + [G[k] for k in names], leaves):
        assert relmax(t, r.grad) < tol * 2        # gradients vs the oracle fed the same rounded operands


def _single_and_group_case(dev, kind):
    """One sublayer at the shapes of the two tests above, bf16, every dropout site at 0.1 under a fixed seed, destinations and a
    queue set.  -> run(grouped) = (y, dx, dmem or None, destinations) of a fresh forward + backward."""
    from mtn_amd import ops
    g = torch.Generator().manual_seed(29)
    bf16 = torch.bfloat16
    seed = torch.full((1,), 1234, device=dev, dtype=torch.int64)
    if kind == "ffn":
        rows, d, ff = 70, 128, 512
        x, mem, mask = torch.randn(2, rows // 2, d, generator=g), None, None
        P = dict(ln_a=1 + 0.1 * torch.randn(d, generator=g), ln_b=0.1 * torch.randn(d, generator=g),
                 w1=torch.randn(ff, d, generator=g) * d ** -0.5, b1=0.1 * torch.randn(ff, generator=g),
                 w2=torch.randn(d, ff, generator=g) * ff ** -0.5, b2=0.1 * torch.randn(d, generator=g))
    else:
        B, a, m, d, h = 3, 20, 37, 128, 4
        x, mem = torch.randn(B, a, d, generator=g), torch.randn(B, m, d, generator=g)
        lens = torch.randint(1, m + 1, (B,), generator=g)
        mask = (torch.arange(m).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1).to(dev)
        P = dict(ln_a=1 + 0.1 * torch.randn(d, generator=g), ln_b=0.1 * torch.randn(d, generator=g),
                 w_qkv=torch.randn(3 * d, d, generator=g) * d ** -0.5, b_qkv=0.1 * torch.randn(3 * d, generator=g),
                 w_o=torch.randn(d, d, generator=g) * d ** -0.5, b_o=0.1 * torch.randn(d, generator=g))
    gy = torch.randn(x.shape, generator=g).to(dev)
    P = {k: v.to(dev) for k, v in P.items()}
    lp = {k: v.to(bf16) for k, v in P.items() if k.startswith("w")}

    def run(grouped):
        xd = x.to(dev).requires_grad_()
        memd = mem.to(dev).requires_grad_() if mem is not None else None
        G = {k: torch.full_like(v, float("nan")) for k, v in P.items()}
        common = dict(p_out=0.1, salt=5, seed=seed, lp_dtype=bf16, grads=G, queue=ops.ParamGradQueue())
        if kind == "ffn":
            cfg = ops.FfnConfig(p_hidden=0.1, w1_lp=lp["w1"], w2_lp=lp["w2"], **common)
            params = (P["ln_a"], P["ln_b"], P["b1"], P["b2"])
        else:
            cfg = ops.MhaConfig(heads=h, p_attn=0.1, w_qkv_lp=lp["w_qkv"], w_o_lp=lp["w_o"], **common)
            params = (P["ln_a"], P["ln_b"], P["b_qkv"], P["b_o"])
        if grouped:
            y, = ops.SublayerGroupFn.apply([ops.GroupMember(kind, cfg, params, mask=mask)], xd, memd)
        elif kind == "ffn":
            y = ops.FFNSublayerFn.apply(xd, P["ln_a"], P["ln_b"], P["w1"], P["b1"], P["w2"], P["b2"], cfg)
        else:
            y = ops.MHASublayerFn.apply(xd, memd, None, mask, P["ln_a"], P["ln_b"], P["w_qkv"], P["b_qkv"], P["w_o"], P["b_o"], cfg)
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach(), xd.grad, (memd.grad if memd is not None else None), G
    return run


@pytest.mark.parametrize("kind", ["mha", "ffn"])
def test_single_sublayer_equals_one_member_group_bitwise(dev, kind):
    """A single-sublayer Function and a SublayerGroupFn of that one member pack the same arguments for the same C entry point:
    outputs, dx, dmem and every parameter-gradient destination are equal bit for bit (bf16, dropout 0.1 at every site)."""
    run = _single_and_group_case(dev, kind)
    y1, dx1, dmem1, G1 = run(grouped=False)
    y2, dx2, dmem2, G2 = run(grouped=True)
    assert bool(torch.isfinite(y1).all()) and not torch.equal(y1 - y1, y1)      # (not an all-zero comparison)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    assert (dmem1 is None) == (dmem2 is None) == (kind == "ffn")
    if dmem1 is not None:
        assert bool(torch.isfinite(dmem1).all()) and torch.equal(dmem1, dmem2)
    for k in G1:
        assert bool(torch.isfinite(G1[k]).all()), k
        assert torch.equal(G1[k], G2[k]), k


# ------------------------------------------------------------------------------------------ whole model vs golden
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(fx.GOLDEN_CONFIGS))
def test_model_forward_matches_reference_golden(dev, dtype, name):
    """encode outputs, every sublayer output of layer 0, final (out, [ae]) and generator log-probs against the outputs the
    REFERENCE produced for the same weights/inputs (ragged batch: padded tails, empty history row, padded frames)."""
    c = fx.GOLDEN_CONFIGS[name]
    g = fx.load_golden(os.path.join(GOLD, name + ".npz"))
    model = build_model(c, dtype, dev).eval()
    b = dev_batch(raw_batch(c), dev)
    taps = {}
    hooks = [sl.register_forward_hook(lambda mod, inp, out, k=k: taps.__setitem__(k, out.detach()))
             for k, sl in enumerate(model.decoder.layers[0].sublayer)]
    with torch.no_grad():
        q, v, cp, hs, ae = model.encode(b.query, b.query_mask, b.his, b.his_mask, b.cap, b.cap_mask, b.fts, b.fts_mask)
        out, ae_out = model.forward(b)
        logp = model.generator(out)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    T = lambda k: torch.from_numpy(g[k])
    tol = TOL[dtype]
    assert relmax(q, T("enc.q")) < tol and relmax(cp, T("enc.cap")) < tol and relmax(hs, T("enc.his")) < tol
    for i, x in enumerate(v):
        assert relmax(x, T(f"enc.vid.{i}")) < tol
    for k in range(5 + 4 * len(c["ft_sizes"])):
        assert relmax(taps[k], T(f"layer0.sublayer.{k}")) < tol, k
    assert relmax(out, T("out")) < tol
    for i, a in enumerate(ae_out):
        assert relmax(a, T(f"ae_out.{i}")) < tol
    assert relmax(logp, T("logp")) < tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["cfg1_query", "small_shared", "small_diffall", "wide_n1"])
def test_model_loss_and_grads_match_reference_golden(dev, dtype, name):
    from mtn_amd import LabelSmoothing, SimpleLossCompute
    c = fx.GOLDEN_CONFIGS[name]
    g = fx.load_golden(os.path.join(GOLD, name + ".npz"))
    model = build_model(c, dtype, dev).eval()        # eval(): dropout off, as in the golden run
    b = dev_batch(raw_batch(c), dev)
    crit = LabelSmoothing(c["vocab"], fx.PAD, 0.1)
    lc = SimpleLossCompute(model.generator, model.auto_encoder_generator, crit, opt=None)
    ae_y = b.cap if c["auto_encoder_ft"] in ("caption", "summary") else b.query
    model.prepare(); model.zero_glue_grads()
    out, ae_out = model.forward(b)
    loss = lc.loss(out, b.trg_y, b.ntokens, ae_out, ae_y, (ae_y != fx.PAD).sum())
    loss.backward()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    assert abs(float(loss) - float(g["loss"])) < tol * max(1.0, abs(float(g["loss"])))
    norms = dict(zip([str(s) for s in g["grad_names"]], g["grad_norms"]))
    params = dict(model.named_parameters())
    # bf16: the 1e-2 bound is stated for outputs; gradients accumulate rounding through 2 layers of LayerNorm-backward
    # projections, so per tensor they only get a loose 0.25 bound (bias gradients are sums of bf16-rounded rows with heavy cancellation);
    # the tight bf16 criterion is the cosine over all fully-stored tensors below.  fp32 mode keeps 3e-3 and proves the algebra.
    gtol = 3e-3 if dtype == torch.float32 else 0.25
    worst, dot, n1, n2 = 0.0, 0.0, 0.0, 0.0
    for k, n in norms.items():
        gr = params[k].grad
        assert gr is not None, k
        gn = float(gr.double().norm())
        if n < 1e-6:        # mathematically zero gradients (a key-projection bias shifts every score of a row equally)
            assert gn < (1e-5 if dtype == torch.float32 else 1e-3), (k, gn)
            continue
        if "grad." + k in g:
            ref = torch.from_numpy(g["grad." + k])
            e = relmax(gr, ref)
            dot += float((gr.double().cpu() * ref.double()).sum()); n1 += gn * gn; n2 += float(ref.double().norm()) ** 2
        else:
            e = relmax(gr.reshape(-1)[:256], torch.from_numpy(g["gradhead." + k]))
        e = max(e, abs(gn - n) / n)
        worst = max(worst, e)
        assert e < gtol, (k, e)
    cos = dot / (n1 ** 0.5 * n2 ** 0.5)
    assert cos > (0.999999 if dtype == torch.float32 else 0.9995), cos
    print(f"{name} {dtype}: worst grad rel err {worst:.2e}, cosine over fully-stored tensors {cos:.7f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_fused_adam_steps_match_reference_golden(dev, dtype):
    """forward -> loss -> backward -> fused Noam/Adam step, twice, vs the reference's NoamOpt(Adam) (train.py:190)."""
    from mtn_amd import FusedAdam, LabelSmoothing, NoamOpt, SimpleLossCompute
    name = "cfg1_query"
    c = fx.GOLDEN_CONFIGS[name]
    g = fx.load_golden(os.path.join(GOLD, name + ".npz"))
    model = build_model(c, dtype, dev).eval()
    b = dev_batch(raw_batch(c), dev)
    opt = NoamOpt(c["d_model"], 1, 10, FusedAdam(model))
    lc = SimpleLossCompute(model.generator, model.auto_encoder_generator, LabelSmoothing(c["vocab"], fx.PAD, 0.1), opt=opt)
    losses = []
    for _ in range(2):
        out, ae_out = model.forward(b)
        losses.append(lc(out, b.trg_y, b.ntokens, ae_out, b.query, (b.query != fx.PAD).sum()))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    np.testing.assert_allclose(losses, g["step_losses"], rtol=tol * 2)
    sd = model.state_dict()
    for k in g:
        if k.startswith("after2."):
            assert relmax(sd[k[7:]], torch.from_numpy(g[k])) < tol * 3, k
        elif k.startswith("after2head."):
            assert relmax(sd[k[11:]].reshape(-1)[:256], torch.from_numpy(g[k])) < tol * 3, k


def test_dropout_training_step_runs_and_is_seed_deterministic(dev, monkeypatch):
    """train() mode: in-kernel dropout on attention probabilities, FFN hidden and sublayer outputs.  Same seed -> same
    loss and gradients; advancing the seed changes them; gradients stay finite."""
    from mtn_amd import LabelSmoothing, SimpleLossCompute
    c = fx.GOLDEN_CONFIGS["cfg1_query"]
    model = build_model(c, torch.bfloat16, dev, dropout=0.1, attn_dropout=0.1).train()
    for mod in model.modules():                 # keep the PyTorch-side (glue) dropout out of the determinism check
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    b = dev_batch(raw_batch(c), dev)
    lc = SimpleLossCompute(model.generator, None, LabelSmoothing(c["vocab"], fx.PAD, 0.1), opt=None)

    def run(seed_val):
        model.prepare(); model.zero_glue_grads()
        model._seed.fill_(seed_val - (0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF))   # encode() advances it by this
        out, ae_out = model.forward(b)
        loss = lc.loss(out, b.trg_y, b.ntokens, ae_out, b.query, (b.query != fx.PAD).sum())
        loss.backward()
        return float(loss), model._flat_grad.clone()

    l1, g1 = run(1000)
    l2, g2 = run(1000)
    l3, g3 = run(2000)
    n_glue = model._glue_numel                   # embedding-table gradients are float atomics: order-dependent rounding
    assert l1 == l2 and torch.equal(g1[n_glue:], g2[n_glue:])
    assert (g1[:n_glue] - g2[:n_glue]).abs().max() <= 1e-5 * g1[:n_glue].abs().max()
    assert l1 != l3
    assert torch.isfinite(g1).all() and torch.isfinite(g3).all()
    monkeypatch.setenv("MTN_EMBED_DETERMINISTIC", "1")   # atomic-free table gradient: the whole step is bitwise reproducible
    __import__("mtn_amd.lib", fromlist=["lib"]).reload_env()
    l4, g4 = run(1000)
    l5, g5 = run(1000)
    assert l4 == l5 == l1 and torch.equal(g4, g5)
    assert (g4[:n_glue] - g1[:n_glue]).abs().max() <= 1e-5 * g1[:n_glue].abs().max()
    model.eval()
    with torch.no_grad():
        e1 = model.forward(b)[0]
        e2 = model.forward(b)[0]
    assert torch.equal(e1, e2)


def test_state_dict_roundtrip_and_lowp_refresh(dev):
    """load_state_dict into the flat buffers refreshes the compute-dtype weight copy (version-counter check)."""
    c = fx.GOLDEN_CONFIGS["small_shared"]
    m1 = build_model(c, torch.bfloat16, dev, seed=0).eval()
    m2 = build_model(c, torch.bfloat16, dev, seed=1).eval()
    b = dev_batch(raw_batch(c), dev)
    with torch.no_grad():
        o1 = m1.forward(b)[0]
        o2 = m2.forward(b)[0]
        assert relmax(o1, o2) > 1e-2
        m2.load_state_dict(m1.state_dict())
        o3 = m2.forward(b)[0]
    assert torch.equal(o1, o3)


@pytest.mark.parametrize("name", ["cfg1_query", "small_shared", "small_diffall"])
def test_lockstep_schedule_equals_sequential_schedule(dev, name):
    """The lockstep-group schedule (independent sublayers share launches) runs the same kernels on the same data as the
    reference's one-sublayer-at-a-time order: outputs and every gradient must be bitwise identical (dropout on)."""
    from mtn_amd import LabelSmoothing, SimpleLossCompute
    c = fx.GOLDEN_CONFIGS[name]
    model = build_model(c, torch.bfloat16, dev, dropout=0.1, attn_dropout=0.1).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    b = dev_batch(raw_batch(c), dev)
    lc = SimpleLossCompute(model.generator, model.auto_encoder_generator, LabelSmoothing(c["vocab"], fx.PAD, 0.1), opt=None)
    ae_y = b.cap if c["auto_encoder_ft"] in ("caption", "summary") else b.query

    def run(lockstep):
        model.lockstep = lockstep
        model.prepare(); model.zero_glue_grads()
        model._flat_grad[model._glue_numel:].fill_(float("nan"))      # every path gradient must be (re)written
        model._seed.fill_(777)
        out, ae_out = model.forward(b)
        loss = lc.loss(out, b.trg_y, b.ntokens, ae_out, ae_y, (ae_y != fx.PAD).sum())
        loss.backward()
        torch.cuda.synchronize()
        return out.detach().clone(), [a.detach().clone() for a in ae_out], model._flat_grad.clone()

    o1, a1, g1 = run(True)
    o2, a2, g2 = run(False)
    assert torch.equal(o1, o2)
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    assert torch.isfinite(g1).all()
    if c["diff_encoder"]:
        n_glue = model._glue_numel           # embedding-table gradients: float atomics, order-dependent rounding
        assert torch.equal(g1[n_glue:], g2[n_glue:]) and relmax(g1[:n_glue], g2[:n_glue]) < 1e-5
    else:   # one seed tensor feeds both auto-encoder chains: autograd sums its gradient contributions in schedule order
        assert relmax(g1, g2) < 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("quirk", [False, True])
def test_fused_loss_head_matches_composed_loss(dev, dtype, quirk):
    """Generator + log-softmax + LabelSmoothing KL + weighted sum as ONE fused head (csrc/losshead.hip) vs the same value
    composed from the oracle's functions: loss, d(loss)/d(hidden) and the generator's weight/bias gradients.  `quirk`:
    the only <pad> target sits at flat row 0 (label_smoothing.py:29 then does NOT zero that row)."""
    from mtn_amd import LabelSmoothing, SimpleLossCompute
    c = dict(fx.GOLDEN_CONFIGS["small_diffall"], vocab=104, diff_gen=False, diff_embed=False)
    model = build_model(c, dtype, dev).eval()
    model.prepare()
    g = torch.Generator().manual_seed(7)
    B, T, Q, d, V = 3, 6, 5, c["d_model"], c["vocab"]
    xs = [torch.randn(B, L, d, generator=g) for L in (T, Q)]
    y = torch.randint(4, V, (B, T), generator=g)
    ya = torch.randint(4, V, (B, Q), generator=g)
    if quirk:
        y[0, 0] = fx.PAD
    else:
        y[0, -2:] = fx.PAD; y[2, -1] = fx.PAD; ya[1, -3:] = fx.PAD
    norm, ae_norm = (y != fx.PAD).sum(), (ya != fx.PAD).sum()
    # oracle composition on CPU
    W = model.generator.proj.weight.detach().float().cpu().clone().requires_grad_()
    bb = model.generator.proj.bias.detach().float().cpu().clone().requires_grad_()
    xr = [x.clone().requires_grad_() for x in xs]
    lp = lambda x: torch.log_softmax(orc.linear(x, W, bb), -1)
    ref = orc.label_smoothing_kl(lp(xr[0]).reshape(-1, V), y.reshape(-1), fx.PAD, 0.1) / norm.float() \
        + 0.7 * orc.label_smoothing_kl(lp(xr[1]).reshape(-1, V), ya.reshape(-1), fx.PAD, 0.1) / ae_norm.float()
    ref.backward()
    # fused head on the GPU
    xd = [x.to(dev).requires_grad_() for x in xs]
    lc = SimpleLossCompute(model.generator, None, LabelSmoothing(V, fx.PAD, 0.1), opt=None, l=0.7)
    model.zero_glue_grads()
    loss = lc.loss(xd[0], y.to(dev), norm.to(dev), [xd[1]], ya.to(dev), ae_norm.to(dev))
    assert loss.grad_fn is not None and "GeneratorLossFn" in type(loss.grad_fn).__name__
    loss.backward()
    torch.cuda.synchronize()
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    assert abs(float(loss) - float(ref)) < tol * abs(float(ref))
    for a, r in zip(xd, xr):
        assert relmax(a.grad, r.grad) < tol
    assert relmax(model.generator.proj.weight.grad, W.grad) < tol
    assert relmax(model.generator.proj.bias.grad, bb.grad) < tol


class _NoSync:
    """Stands in for dp.GradSync on one rank: same call surface, no exchange."""
    world = 1

    def __init__(self):
        self.ranges = []

    def all_reduce_scalars(self, t):
        return t

    def reduce_range(self, lo, hi):
        self.ranges.append((lo, hi))
        return None

    def wait(self, handles):
        pass

    def __call__(self):
        pass


@pytest.mark.parametrize("sharded", [False, True], ids=["allreduce", "sharded-optimiser"])
@pytest.mark.parametrize("name", ["cfg1_query", "cfg1_caption", "small_shared"])
def test_layer_segmented_backward_equals_monolithic(dev, name, sharded, monkeypatch):
    """TrainStep under data parallelism cuts backward at the decoder-layer boundaries (forward_segmented) so that each
    layer's gradient slice can be exchanged while the next layer's backward runs: same loss, same gradients, and the slices
    handed to the exchange tile the flat gradient buffer exactly once."""
    from mtn_amd.train_step import TrainStep
    c = fx.GOLDEN_CONFIGS[name]
    model = build_model(c, torch.bfloat16, dev, dropout=0.1, attn_dropout=0.1).train()
    for mod in model.modules():                 # the feature streams' dropout is PyTorch's (its own RNG): keep it out
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    b = dev_batch(raw_batch(c), dev)
    sync = _NoSync()
    monkeypatch.setenv("MTN_DP_SHARDED", "1" if sharded else "0")
    ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, grad_sync=sync, use_graph=False, overlap=True)
    assert (ts.sharded is not None) == sharded
    model.prepare()
    model._seed.fill_(4242)
    l1 = ts._fwd_bwd()
    g1 = model._flat_grad.clone()
    model._flat_grad.fill_(float("nan"))
    model._seed.fill_(4242)
    ts._run_segmented(ts._segments())
    torch.cuda.synchronize()
    g2, l2 = model._flat_grad.clone(), ts._loss_t
    assert float(l1) == float(l2)
    n_glue = model._glue_numel
    assert torch.isfinite(g2).all()
    if c["diff_encoder"]:
        assert torch.equal(g1[n_glue:], g2[n_glue:])
    else:
        assert relmax(g1[n_glue:], g2[n_glue:]) < 1e-5
    assert relmax(g1[:n_glue], g2[:n_glue]) < 1e-5
    covered = sorted(ts.sharded.slices) if sharded else sorted(sync.ranges)     # what was handed to the exchange
    assert covered[0][0] == 0 and covered[-1][1] == g1.numel()
    assert all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1))


def test_segmented_graph_step_tracks_monolithic_graph_step(dev):
    """The N+3-graph schedule (segments + Adam) and the single-graph step train the same model: losses of 4 steps agree."""
    from mtn_amd.train_step import TrainStep
    c = fx.GOLDEN_CONFIGS["cfg1_query"]
    losses = []
    for overlap in (False, True):
        model = build_model(c, torch.bfloat16, dev, dropout=0.0, attn_dropout=0.0).train()
        b = dev_batch(raw_batch(c), dev)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, grad_sync=_NoSync() if overlap else None, use_graph=True, overlap=overlap)
        losses.append([float(ts()) for _ in range(4)])
    assert losses[0][0] == losses[1][0]
    assert max(abs(a - b) / abs(a) for a, b in zip(*losses)) < 1e-3
    assert losses[0][3] < losses[0][0]


def test_checkpoint_resume_continues_the_same_trajectory(dev, tmp_path):
    """model.state_dict() (reference key schema) + NoamOpt.state_dict() (moments by parameter name + the device-side schedule
    state) saved after 3 steps and loaded into a fresh model/optimiser: the next steps equal the uninterrupted run's."""
    from mtn_amd.train_step import TrainStep
    c = fx.GOLDEN_CONFIGS["cfg1_query"]
    b = dev_batch(raw_batch(c), dev)

    def fresh():
        m = build_model(c, torch.bfloat16, dev, dropout=0.0, attn_dropout=0.0).train()
        return m, TrainStep(m, b, c["vocab"], pad=fx.PAD, warmup=20, use_graph=False)

    m1, t1 = fresh()
    for _ in range(3):
        t1()
    path = tmp_path / "ck.pt"
    torch.save({"model": m1.state_dict(), "opt": t1.opt.state_dict()}, path)
    cont = [float(t1()) for _ in range(3)]
    m2, t2 = fresh()
    ck = torch.load(path)
    m2.load_state_dict(ck["model"], strict=False)
    m2.prepare()
    t2.opt.load_state_dict(ck["opt"])
    resumed = [float(t2()) for _ in range(3)]
    # (float atomics in the embedding-table gradients + Adam normalisation make two runs differ by ~1e-4; a lost optimiser state
    #  would show as ~1e-1)
    assert max(abs(a - r) / abs(a) for a, r in zip(cont, resumed)) < 3e-3, (cont, resumed)
    assert t2.opt._step == 6 and abs(t2.opt.rate() - t1.opt.rate()) < 1e-12


@pytest.mark.parametrize("name", [n for n in fx.GOLDEN_CONFIGS if n != "cfg1_query"])
def test_optimiser_epilogue_covers_every_model_variant(dev, name, monkeypatch):
    """The other reference configurations (caption / summary auto-encoder, shared encoder, separate embeddings and generators):
    every sublayer weight matrix receives exactly one parameter-gradient GEMM (the epilogue raises otherwise) and two fused
    steps equal two separate-optimiser steps bit for bit."""
    from mtn_amd.train_step import TrainStep
    monkeypatch.setenv("MTN_EMBED_DETERMINISTIC", "1")
    __import__("mtn_amd.lib", fromlist=["lib"]).reload_env()
    c = fx.GOLDEN_CONFIGS[name]
    b = dev_batch(raw_batch(c), dev)
    res = []
    for fused in (True, False):
        m = build_model(c, torch.bfloat16, dev, dropout=0.0, attn_dropout=0.0).train()
        ts = TrainStep(m, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, fuse_optimizer=None if fused else False)
        losses = [float(ts()) for _ in range(2)]
        torch.cuda.synchronize()
        assert ts._fused() == fused
        res.append((losses, m._flat.clone(), m._flat_lpT.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_optimiser_epilogue_equals_separate_adam(dev, dtype, use_graph, monkeypatch):
    """One rank: the Adam update of every sublayer weight matrix rides on the GEMM that produces its gradient (mtn_adam_fuse)
    and the rest of the flat buffer is updated chunk-wise.  Same arithmetic in the same order as the separate whole-buffer
    pass: parameters, both moments, the compute-dtype copy and its transposed copy must come out bit for bit the same over
    several steps (with the atomic-free table gradient, so that nothing else differs between two runs)."""
    from mtn_amd.train_step import TrainStep
    monkeypatch.setenv("MTN_EMBED_DETERMINISTIC", "1")
    __import__("mtn_amd.lib", fromlist=["lib"]).reload_env()
    c = fx.GOLDEN_CONFIGS["cfg1_query"]
    b = dev_batch(raw_batch(c), dev)
    res = []
    for fused in (True, False):
        if fused:
            monkeypatch.delenv("MTN_NO_FUSED_ADAM", raising=False)
        else:
            monkeypatch.setenv("MTN_NO_FUSED_ADAM", "1")
            __import__("mtn_amd.lib", fromlist=["lib"]).reload_env()
        m = build_model(c, dtype, dev, dropout=0.1, attn_dropout=0.1).train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        ts = TrainStep(m, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph)
        m.prepare()
        m._seed.fill_(99)
        losses = [float(ts()) for _ in range(3)]
        torch.cuda.synchronize()
        assert ts._fused() == fused
        res.append((losses, m._flat.clone(), ts.opt.optimizer.m.clone(), ts.opt.optimizer.v.clone(), m._flat_lp.clone(), m._flat_lpT.clone()))
    (la, *ta), (lb, *tb) = res
    assert la == lb
    for x, y in zip(ta, tb):
        assert torch.equal(x, y)
    assert la[2] < la[0]
