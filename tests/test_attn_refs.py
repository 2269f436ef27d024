"""tests/attn_refs.py checked on the CPU: attn_ref against float64 autograd through the oracle's attention, BARS against the values
measured here from attn_emulate (the reference side only), and the teeth of attn_check on deliberately wrong variants."""
import math

import pytest
import torch

from tests import attn_refs as A

ALL = [(c["id"], i, dt) for c in A.CASES for dt in c["dtypes"] for i in range(len(c["members"]))]


def _oracle_autograd(x, h):
    """O, dQ, dK, dV by float64 autograd through oracle.mtn_oracle.scaled_dot_attention; with dropout the same chain with the host
    mask multiplied into the probabilities (tests/test_dropout_parity_gpu._attn_ref)."""
    from oracle.mtn_oracle import scaled_dot_attention
    q, k, v = (x[n].double().requires_grad_() for n in ("q", "k", "v"))
    B, a, d = q.shape
    sp = lambda t: t.reshape(B, -1, h, d // h).transpose(1, 2)
    mask4 = None if x["mask"] is None else x["mask"].unsqueeze(1)
    o, p = scaled_dot_attention(sp(q), sp(k), sp(v), mask4)
    if x["keep"] is not None:
        o = (p * (x["keep"].double() * float(A.R.scale(x["p"])))) @ sp(v)
    o = o.transpose(1, 2).reshape(B, a, d)
    o.backward(x["d_o"].double())
    return p.detach(), dict(O=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)


@pytest.mark.parametrize("cid,idx,dtype", ALL, ids=[f"{c}-{i}-{dt}" for c, i, dt in ALL])
def test_ref_is_oracle_autograd(cid, idx, dtype):
    x = A.inputs(cid, idx, dtype)
    mem = A.CASE_BY_ID[cid]["members"][idx]
    ref, _ = A.reference(cid, idx, dtype)
    p, want = _oracle_autograd(x, mem["h"])
    for kind in A.KINDS:
        got, w = getattr(ref, kind), want[kind]
        scale = float(w.abs().max()) or 1.0           # m == 1: dQ and dK are 0 analytically; the inputs are of order 1
        assert float((got - w).abs().max()) <= 1e-12 * scale, (kind, float((got - w).abs().max()))
    # the saved statistics reproduce the oracle's probabilities: P = exp(S - rowmax) * invsum
    s = A._chain64(x["q"], x["k"], x["v"], x["d_o"], x["mask"], mem["h"], None, 0.0)["S"]
    p2 = torch.exp(s - ref.rowmax.unsqueeze(-1)) * ref.invsum.unsqueeze(-1)
    assert float((p2 - p).abs().max()) <= 1e-12
    if x["mask"] is not None:                       # a fully masked row: max == -1e9 and uniform over all m keys
        full = A._masked(x["mask"], *p.shape).all(dim=-1)
        assert bool((ref.rowmax[full] == -1e9).all()) and bool((ref.invsum[full] == 1.0 / mem["m"]).all())


def _structural_zero_checks(cid, idx, dtype):
    x = A.inputs(cid, idx, dtype)
    mem = A.CASE_BY_ID[cid]["members"][idx]
    ref, bnd = A.reference(cid, idx, dtype)
    for kind in A.KINDS:                             # the bound is 0 only where the true value is
        assert bool((getattr(ref, kind)[bnd[kind] == 0] == 0).all()), kind
    return x, mem, ref, bnd


def test_bound_zero_pattern():
    """B == 0 exactly on the structural zeros: dK / dV rows of a key masked for every query, dQ rows and dK of a fully masked sample
    (whose dV is not 0); and nowhere the true value is non-zero, with dropout on too."""
    x, mem, ref, bnd = _structural_zero_checks("cross_perq", 0, "bf16")
    assert bool((bnd["dK"][:, mem["m"] - 1] == 0).all()) and bool((bnd["dV"][0, mem["m"] - 1] == 0).all())
    assert bool((bnd["dV"][mem["B"] - 1, mem["m"] - 1] > 0).all())       # the fully masked row of the last sample is uniform over ALL keys
    assert bool((bnd["dQ"][mem["B"] - 1, mem["a"] // 2] == 0).all()) and bool((bnd["dQ"][0] > 0).all())
    x, mem, ref, bnd = _structural_zero_checks("dk128", 0, "fp32")
    last = mem["B"] - 1
    assert bool((bnd["dQ"][last] == 0).all()) and bool((bnd["dK"][last] == 0).all()) and bool((bnd["dV"][last] > 0).all())
    assert bool((bnd["O"] > 0).all())
    for i in (1, 3):                                 # the dropout members: a key dropped for every query row still has dK != 0
        x, mem, ref, bnd = _structural_zero_checks("g4", i, "bf16")
    dead = ~x["keep"].any(dim=2)                     # [B, h, m] of member 3 (a = 5, p = 0.5)
    assert int(dead.sum()) > 0


def _measure():
    worst = {name: dict.fromkeys(A.KINDS, 0.0) for name in ("fp32", "bf16", "bf16_passes")}
    for cid, idx, dtype in ALL:
        mem = A.CASE_BY_ID[cid]["members"][idx]
        x = A.inputs(cid, idx, dtype)
        ref, bnd = A.reference(cid, idx, dtype)
        pp = A.per_pass_rounding(mem, dtype)
        emu = A.attn_emulate(x["q"], x["k"], x["v"], x["d_o"], x["mask"], mem["h"], A.TORCH_DTYPE[dtype], x["keep"], x["p"], passes=pp)
        for kind in A.KINDS:
            r, _, nonzero = A.ratio(getattr(emu, kind), getattr(ref, kind), bnd[kind], A.U[dtype])
            assert nonzero == 0 and math.isfinite(r), (cid, idx, dtype, kind)
            name = "bf16_passes" if pp else dtype
            worst[name][kind] = max(worst[name][kind], r)
    for kind in A.KINDS:                              # a per-pass member is held to no less than the plain bf16 bar allows
        worst["bf16_passes"][kind] = max(worst["bf16_passes"][kind], worst["bf16"][kind])
    return worst


def test_bars_are_the_measured_ones():
    """BARS[dtype][kind] == max(4 max_cases r_emu, 4) with r_emu the ratio of attn_emulate against attn_ref: written down in
    attn_refs.py, measured here, never against a kernel."""
    worst = _measure()
    bars = {name: {kind: A.bar_of(v) for kind, v in w.items()} for name, w in worst.items()}
    print("r_emu", {n: {k: round(v, 3) for k, v in w.items()} for n, w in worst.items()})
    print("BARS ", bars)
    assert bars == A.BARS


TEETH_CASES = [("cross_perq", 0), ("valu_dk96", 0)]      # dropout-free: one per-query mask, one without a mask


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("cid,idx", TEETH_CASES)
def test_check_has_teeth(cid, idx, dtype):
    """The honest emulation passes attn_check under BARS; every wrong variant fails it on a ratio (not only on relmax)."""
    mem = A.CASE_BY_ID[cid]["members"][idx]
    x = A.inputs(cid, idx, dtype)
    ref, bnd = A.reference(cid, idx, dtype)
    bars = A.bars_for(mem, dtype)
    run = lambda wrong: A.attn_emulate(x["q"], x["k"], x["v"], x["d_o"], x["mask"], mem["h"], A.TORCH_DTYPE[dtype], wrong=wrong)
    as_dict = lambda e: {kind: getattr(e, kind) for kind in A.KINDS}
    ratios, failures = A.attn_check(as_dict(run(None)), ref, bnd, dtype, bars)
    assert not failures, failures
    for wrong in A.WRONG:
        if wrong == "mask_row_off" and x["mask"] is None:
            continue                                  # nothing to read a row off without a mask
        ratios, failures = A.attn_check(as_dict(run(wrong)), ref, bnd, dtype, bars)
        caught = [f for f in failures if "ratio" in f or "bound is 0" in f]
        print(cid, dtype, wrong, {k_: round(v[0], 1) for k_, v in ratios.items()})
        assert caught, (wrong, ratios)
