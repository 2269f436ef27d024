"""tests/decode_refs.py against the model's definition, on the CPU: step_ref fed step by step from position 0 reproduces the oracle's
decoder (oracle/mtn_oracle.py) on the whole prefix, a re-ordered cache with its permutation in `anc` changes no bit, the stored
CPU_EMUL_* constants are what step_emul - step_ref measures, and every case's planted keys hold their share of the probability."""
import math

import pytest
import torch

from oracle import mtn_oracle as O
from tests import decode_refs as R


def _oracle_state(g, n_layers, d, dff, V):
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = {"tgt_embed.0.lut.weight": rn(V, d) / math.sqrt(d)}

    def norm(name):
        p[name + ".a_2"], p[name + ".b_2"] = 1 + 0.1 * rn(d), 0.1 * rn(d)

    def mha(name):
        for i in range(4):
            p[f"{name}.linears.{i}.weight"], p[f"{name}.linears.{i}.bias"] = rn(d, d) / math.sqrt(d), 0.1 * rn(d)

    def ffn(name):
        p[name + ".w_1.weight"], p[name + ".w_1.bias"] = rn(dff, d) / math.sqrt(d), 0.1 * rn(dff)
        p[name + ".w_2.weight"], p[name + ".w_2.bias"] = rn(d, dff) / math.sqrt(dff), 0.1 * rn(d)

    for n in range(n_layers):
        L = f"decoder.layers.{n}"
        for a in ("self_attn", "his_attn", "cap_attn", "src_attn", "auto_encoder_self_attn.0", "auto_encoder_vid_attn.0", "auto_encoder_attn.0"):
            mha(f"{L}.{a}")
        ffn(L + ".feed_forward"); ffn(L + ".auto_encoder_feed_forward.0")
        for k in range(9):
            norm(f"{L}.sublayer.{k}.norm")
    norm("decoder.norm"); norm("decoder.ae_norm.0")
    return p


def test_step_ref_is_the_oracle_decoder():
    """d 128, 4 heads, 2 layers, the text memories and one feature stream, float64: step_ref walked from position 0 with identity
    ancestors and its own cache rows gives, at every position, the oracle decoder's output for that position of the whole prefix."""
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    nl, d, h, dff, V, W, T = 2, 128, 4, 256, 23, 3, 6
    cfg = O.OracleConfig(vocab=V, n_layers=nl, d_model=d, d_ff=dff, heads=h, ft_sizes=(16,), auto_encoder_ft="query")
    model = O.OracleMTN(cfg, _oracle_state(g, nl, d, dff, V))
    lens = dict(his=(9, [9, 4, 1]), cap=(5, [3, 5, 2]), q=(7, [7, 7, 3]))
    mem = {n: rn(W, m, d) for n, (m, _) in lens.items()}
    msk = {n: (torch.arange(m).unsqueeze(0) < torch.tensor(l).unsqueeze(1)).unsqueeze(1) for n, (m, l) in lens.items()}      # [W, 1, m]
    vid, ae0 = rn(W, 4, d), rn(W, 7, d)
    tgt = torch.randint(0, V, (W, T), generator=g)
    model.taps = {}
    want, _ = model.decode([vid], mem["his"], mem["cap"], mem["q"], [None], msk["his"], msk["cap"], msk["q"], tgt, O.subsequent_mask(T), [ae0])

    P = model.p
    ln = lambda name: dict(ln_a=P[name + ".a_2"], ln_b=P[name + ".b_2"], ln_eps=cfg.ln_eps)
    lin = lambda w, b: dict(N=w.shape[0], K=w.shape[1], w=w, bias=b)
    st, caches = [dict(kind=R.EMBED)], []
    for n in range(nl):
        L = f"decoder.layers.{n}"
        wb = lambda a, i: (P[f"{L}.{a}.linears.{i}.weight"], P[f"{L}.{a}.linears.{i}.bias"])
        caches.append(torch.full((W, T, 2 * d), float("nan"), dtype=torch.float64))
        st.append(dict(kind=R.SELF_QKV, cache=n, **lin(torch.cat([wb("self_attn", i)[0] for i in range(3)]), torch.cat([wb("self_attn", i)[1] for i in range(3)])),
                       **ln(f"{L}.sublayer.0.norm")))
        st.append(dict(kind=R.SELF_ATT, cache=n))
        st.append(dict(kind=R.OUT, **lin(*wb("self_attn", 3))))
        ae_now = model.taps[f"{L}.sublayer.6"]                    # the auto-encoder stream after this layer's own three sublayers
        for k, a, memory, mask in ((1, "his_attn", mem["his"], msk["his"]), (2, "cap_attn", mem["cap"], msk["cap"]),
                                   (3, "src_attn", mem["q"], msk["q"]), (7, "auto_encoder_attn.0", ae_now, msk["q"])):
            kv = torch.cat([O.linear(memory, *wb(a, 1)), O.linear(memory, *wb(a, 2))], dim=-1)
            st.append(dict(kind=R.CROSS, kv=kv, m=kv.shape[1], mask=mask[:, 0].to(torch.uint8), mask_stride=kv.shape[1], **lin(*wb(a, 0)),
                           **ln(f"{L}.sublayer.{k}.norm")))
            st.append(dict(kind=R.OUT, **lin(*wb(a, 3))))
        ff = L + ".feed_forward"
        st.append(dict(kind=R.FFN1, **lin(P[ff + ".w_1.weight"], P[ff + ".w_1.bias"]), **ln(f"{L}.sublayer.8.norm")))
        st.append(dict(kind=R.FFN2, **lin(P[ff + ".w_2.weight"], P[ff + ".w_2.bias"])))
    st.append(dict(kind=R.FINAL, **ln("decoder.norm")))
    anc = torch.arange(W, dtype=torch.int32).unsqueeze(1).expand(W, T).contiguous()
    case = dict(W=W, d=d, h=h, L=T, d_ff=dff, stages=st, caches=caches, lut=P["tgt_embed.0.lut.weight"], pe=O.positional_encoding(T, d, torch.float64),
                emb_scale=math.sqrt(d), steps=[dict(tokens=tgt[:, t], pos=t, anc=anc) for t in range(T)])
    res, after = R.run_case(case)
    for t in range(T):
        err = float((res[t]["out_lp"] - want[:, t]).abs().max() / want[:, t].abs().max())
        assert err <= 1e-9, f"position {t}: step_ref is {err:.3g} (relative) from the oracle decoder"
    assert all(bool(torch.isfinite(c).all()) for c in after), "a cache row was not written"


def _permuted(case, g):
    """The case with the cache slots of every position t < pos shuffled and the shuffle written into anc."""
    W, pos = case["W"], case["steps"][0]["pos"]
    caches = [c.clone() for c in case["caches"]]
    steps = [dict(s, anc=s["anc"].clone()) for s in case["steps"]]
    for t in range(pos):
        perm = torch.randperm(W, generator=g)
        for c, c0 in zip(caches, case["caches"]):
            c[perm, t] = c0[:, t]
        for s in steps:
            s["anc"][:, t] = perm[s["anc"][:, t].long()].to(torch.int32)
    return dict(case, steps=steps), caches


@pytest.mark.parametrize("cid", ["self_d128_pos255_w9", "self_d256_pos1_w1", "self_d256_pos256_w16", "whole_d128_w13"])
@pytest.mark.parametrize("emul", [False, True])
def test_reordered_cache_changes_no_bit(cid, emul):
    case = R.build_case(cid)
    twin, caches = _permuted(case, torch.Generator().manual_seed(3))
    assert any(not torch.equal(a["anc"], b["anc"]) for a, b in zip(case["steps"], twin["steps"])) or case["steps"][0]["pos"] * case["W"] <= 1
    want, _ = R.run_case(case, emul)
    got, _ = R.run_case(twin, emul, caches)
    for a, b in zip(want, got):
        assert torch.equal(a["out_lp"], b["out_lp"])
        for key in ("x", "qkv", "att", "hid", "cache_rows"):
            assert all(torch.equal(a[key][i], b[key][i]) for i in a[key]), key


def test_constants_are_what_the_emulation_measures():
    got = R.measure_constants()
    for k in R.CONSTANTS:
        stored = getattr(R, "CPU_EMUL_" + k)
        assert abs(got[k] - stored) <= 0.1 * stored, f"CPU_EMUL_{k} = {stored:.3g} stored, {got[k]:.3g} measured"


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_planted_keys_hold_their_share(cid):
    case = R.build_case(cid)
    ok, worst = R.planted_ok(case)
    assert ok, f"a planted key holds {worst:.3f} of its row"
    sp = R.CASE_BY_ID[cid]
    if sp["n_mid"] is None and sp["kind"] in ("cross", "self"):
        m = sp["m"] if sp["kind"] == "cross" else sp["pos"] + 1
        want = {e for e in (0, m - 1, 127, 128, 255, 256) if e < m} if m > 1 else set()
        got = {e for _, _, _, e in case["planted"]}
        if case["W"] * case["h"] >= len(want):                     # (one pair per edge: a single hypothesis has h pairs)
            assert got == want, f"edges planted {sorted(got)}, wanted {sorted(want)}"
        else:
            assert len(got) == case["W"] * case["h"] and got <= want
        assert len({(j, hd) for _, j, hd, _ in case["planted"]}) == len(case["planted"])
