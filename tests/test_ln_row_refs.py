"""CPU self-test of tests/ln_row_refs.py: the float32 emulation of every LayerNorm row kernel stays inside the derived bounds on every
case tests/test_ln_row_kernels_gpu.py runs (worst ratios printed; they are recorded in the refs docstring), and each listed mutation of
a kernel lands OUTSIDE them in every case family it applies to — the condition that keeps the bounds meaningful."""
import numpy as np
import pytest
import torch

from tests import ln_row_refs as lr

FWD, BWD = lr.fwd_cases(), lr.bwd_cases()
_CACHE = {}


def _fwd(rows, d, cls):
    """case + float64 reference + bounds, computed once and left unchanged"""
    k = ("f", rows, d, cls)
    if k not in _CACHE:
        c = lr.make_case(rows, d, cls)
        y, mean, rstd = lr.fwd64(c.x, c.a2, c.b2, c.eps)
        _CACHE[k] = (c, dict(y=y, mean=mean, rstd=rstd), lr.fwd_bounds(c.x, np.zeros((rows, d)), c.a2, c.b2, c.eps))
    return _CACHE[k]


def _bwd(rows, d, cls, has_dres):
    k = ("b", rows, d, cls, has_dres)
    if k not in _CACHE:
        c = lr.make_case(rows, d, cls)
        _, mean, rstd = lr.fwd64(c.x, c.a2, c.b2, c.eps)
        m32, r32 = mean.astype(np.float32), rstd.astype(np.float32)
        dres = c.dres if has_dres else None
        dx, da2, db2, part = lr.bwd64(c.x, c.a2, c.g, c.eps, dres)
        B = lr.bwd_bounds(c.x, c.a2, c.g, c.eps, m32, r32, has_dres, dx)
        _CACHE[k] = (c, m32, r32, dres, dict(dx=dx, da2=da2, db2=db2, partial=part), B)
    return _CACHE[k]


def _bwd_outputs(i, generic, **mut):
    """emulated outputs of the i-th backward case with their references and bounds: {name: (out, ref, bound)}"""
    rows, d, cls = BWD[i]
    has_dres, lp_dtype, lp_p = lr.bwd_variant(i)
    drop_last = mut.pop("drop_last_block", False)
    c, m32, r32, dres, ref, B = _bwd(rows, d, cls, has_dres)
    keep = lr.keep2d(0x700 + i, lp_p, rows, d) if lp_p > 0 else None
    em = lr.emulate_bwd(c.x, c.a2, c.g, c.eps, m32, r32, dres, generic=generic, lp=dict(keep=keep, p=lp_p, dtype=lp_dtype), **mut)
    part = em["partial"][:-1] if drop_last else em["partial"]
    fin = lr.emulate_finalize(part) if len(part) else np.zeros(2 * d, dtype=np.float32)
    lp_ref, v = lr.handoff64(ref["dx"], keep, lp_p, lp_dtype)
    return dict(dx=(em["dx"], ref["dx"], B["dx"]), partial=(em["partial"], ref["partial"], B["partial"]),
                da2=(fin[:d], ref["da2"], B["da2"]), db2=(fin[d:], ref["db2"], B["db2"]),
                dx_lp=(em["dx_lp"], lp_ref, lr.handoff_bound(v, B["dx"], keep, lp_p, lp_dtype)))


def _kernels(d):
    """the backward kernels a stream of width d can run on: the small one alone or, grouped with a wider stream, the generic one"""
    return (False, True) if d <= 512 else (True,)


def _src_outputs(case, **mut):
    mode, d, p = case
    c = lr.make_src(mode, d, p)
    per_row = mut.pop("drop_per_row", False)
    x64, bx = lr.src64(c.rows, d, **lr.src_args(c))
    keep = lr.keep2d(c.salt, p, c.rows, d, per_row=True) if per_row else c.keep
    v = lr.emulate_src(c.rows, d, **lr.src_args(c, keep=keep), **mut)
    out = dict(x_out=(v, x64, bx))
    if c.no_ln:
        out["y_f32"] = (v, x64, bx)
        return out
    y, mean, rstd = lr.fwd64(x64, c.a2, c.b2, c.eps)
    B = lr.fwd_bounds(x64, bx, c.a2, c.b2, c.eps)
    em = lr.emulate_fwd(v, c.a2, c.b2, c.eps)
    out.update(mean=(em["mean"], mean, B["mean"]), rstd=(em["rstd"], rstd, B["rstd"]), y_f32=(em["y"], y, B["y_f32"]),
               y_lp=(torch.from_numpy(em["y"]).to(torch.bfloat16), y, B["y_bf16"]))
    return out


def test_emulation_inside_the_bounds():
    """Every case of the GPU file, unmutated: all outputs inside their bounds, worst ratio per output below 1."""
    worst = {}

    def note(name, out, ref, bound, what):
        worst[name] = max(worst.get(name, 0.0), lr.assert_within(out, ref, bound, f"{name} {what}"))

    for rows, d, cls in FWD:
        c, ref, B = _fwd(rows, d, cls)
        em = lr.emulate_fwd(c.x, c.a2, c.b2, c.eps)
        note("mean", em["mean"], ref["mean"], B["mean"], (rows, d, cls))
        note("rstd", em["rstd"], ref["rstd"], B["rstd"], (rows, d, cls))
        note("y_f32", em["y"], ref["y"], B["y_f32"], (rows, d, cls))
        note("y_lp", torch.from_numpy(em["y"]).to(torch.bfloat16), ref["y"], B["y_bf16"], (rows, d, cls))
        if cls == "e":                                       # the constant row: exact
            k = c.const_row
            assert em["mean"][k] == np.float32(0.5) and em["rstd"][k] == np.float32(1.0) / np.float32(c.eps)
            assert np.array_equal(em["y"][k], c.b2) and np.isfinite(em["y"]).all()
    for case in lr.src_cases():
        for name, (out, ref, bound) in _src_outputs(case).items():
            note(name, out, ref, bound, case)
    for i, (rows, d, cls) in enumerate(BWD):
        for generic in _kernels(d):
            for name, (out, ref, bound) in _bwd_outputs(i, generic).items():
                note(name, out, ref, bound, (rows, d, cls, "generic" if generic else "small"))
    for n in lr.FIN_NPARTS:
        for d in lr.FIN_D:
            p = lr.make_partials(n, d, 31 * n + d)
            note("finalize", lr.emulate_finalize(p), lr.finalize64(p), lr.finalize_bound(p), (n, d))
    print("worst |emulation - float64| / bound:  " + " | ".join(f"{k} {v:.5f}" for k, v in worst.items()))
    assert set(worst) == {"x_out", "mean", "rstd", "y_f32", "y_lp", "dx", "dx_lp", "partial", "da2", "db2", "finalize"}
    assert max(worst.values()) < 1.0


def _rejected(out, ref, bound):
    return lr.violations(out, ref, bound)[0] > 0


D_MIN, D_MAX = min(d for _, d in lr.PAIRS), max(d for _, d in lr.PAIRS)
# mutation -> (switch of emulate_fwd, output it must break, the cases it applies to)
FWD_MUTATIONS = {
    "biased_variance": ("biased", "rstd", lambda r, d, k: d in (D_MIN, D_MAX)),
    # at eps = 1e-6 on rows of std 1 or 2 these two are below float32's resolution of rstd: classes b (low variance) and d (eps = 1e-3)
    "eps_inside_sqrt": ("eps_in_sqrt", "rstd", lambda r, d, k: k in "bd"),
    "rstd_without_eps": ("rstd_no_eps", "rstd", lambda r, d, k: k in "bd"),
    "last_float4_not_in_mean": ("mean_skip_last4", "mean", lambda r, d, k: True),
    "a2_columns_swapped": ("swap_a2", "y", lambda r, d, k: True),
}


@pytest.mark.parametrize("name", list(FWD_MUTATIONS))
def test_forward_mutation_rejected(name):
    switch, what, applies = FWD_MUTATIONS[name]
    n = 0
    for rows, d, cls in FWD:
        if not applies(rows, d, cls):
            continue
        c, ref, B = _fwd(rows, d, cls)
        em = lr.emulate_fwd(c.x, c.a2, c.b2, c.eps, **{switch: True})
        assert _rejected(em[what], ref[what], B["y_f32" if what == "y" else what]), f"{name} passes at {(rows, d, cls)}"
        if what == "y":
            assert _rejected(torch.from_numpy(em["y"]).to(torch.bfloat16), ref["y"], B["y_bf16"]), f"{name} passes in bf16 at {(rows, d, cls)}"
        n += 1
    assert n >= 8


SRC_MUTATIONS = {
    "pe_by_row": (dict(pe_by_row=True), lambda m: True),
    "dropout_index_per_row": (dict(drop_per_row=True), lambda m: True),
    "emb_scale_after_pe": (dict(scale_after_pe=True), lambda m: m != "x_pe"),
}


@pytest.mark.parametrize("name", list(SRC_MUTATIONS))
def test_source_mutation_rejected(name):
    mut, applies = SRC_MUTATIONS[name]
    n = 0
    for case in lr.src_cases():
        if applies(case[0]):
            out, ref, bound = _src_outputs(case, **mut)["x_out"]
            assert _rejected(out, ref, bound), f"{name} passes at {case}"
            n += 1
    assert n >= 12


# mutation -> (switch, outputs it must break, the cases it applies to: (case index, rows, d, class))
BWD_MUTATIONS = {
    "dres_dropped": ("drop_dres", ("dx",), lambda i, r, d, k: lr.bwd_variant(i)[0]),
    "c1_over_d_minus_1": ("c1_dm1", ("dx",), lambda i, r, d, k: True),
    "c2_over_d": ("c2_d", ("dx",), lambda i, r, d, k: True),
    "std_without_eps": ("std_no_eps", ("dx",), lambda i, r, d, k: k in "bd"),
    "da2_without_rstd": ("da2_no_rstd", ("partial", "da2"), lambda i, r, d, k: True),
    "last_partial_block_dropped": ("drop_last_block", ("da2", "db2"), lambda i, r, d, k: True),
    "clamped_row_counted": ("clamp_counted", ("partial", "da2", "db2"), lambda i, r, d, k: r % 8 != 0),
    "handoff_before_dres": ("lp_before_dres", ("dx_lp",), lambda i, r, d, k: lr.bwd_variant(i)[0]),
}


@pytest.mark.parametrize("name", list(BWD_MUTATIONS))
def test_backward_mutation_rejected(name):
    switch, outputs, applies = BWD_MUTATIONS[name]
    n = 0
    for i, (rows, d, cls) in enumerate(BWD):
        if not applies(i, rows, d, cls):
            continue
        for generic in _kernels(d):
            res = _bwd_outputs(i, generic, **{switch: True})
            for what in outputs:
                assert _rejected(*res[what]), f"{name} passes on {what} at {(rows, d, cls)} ({'generic' if generic else 'small'} kernel)"
            n += 1
    assert n >= 30


@pytest.mark.parametrize("name", ["tail_loop_dropped", "loop64_one_part_late"])
def test_finalize_mutation_rejected(name):
    for n in lr.FIN_NPARTS:
        if name == "tail_loop_dropped" and n % 64 == 0:
            continue                                         # 64 and 128 parts leave the tail loop nothing
        if name == "loop64_one_part_late" and n % 128 == 0:
            continue                                         # 128 parts are all taken by the 128-step loop
        for d in lr.FIN_D:
            p = lr.make_partials(n, d, 31 * n + d)
            out = lr.emulate_finalize(p, drop_tail=name == "tail_loop_dropped", late64=name == "loop64_one_part_late")
            assert _rejected(out, lr.finalize64(p), lr.finalize_bound(p)), f"{name} passes at nparts {n}, d {d}"


def test_finalize_boundaries_take_every_loop():
    """The part counts of the GPU file sit on both sides of every loop boundary of the kernel (16 k | 49 | 65 | 113 | 129)."""
    assert {15, 16, 17, 48, 49, 64, 65, 112, 113, 128, 129} <= set(lr.FIN_NPARTS)
    p = lr.make_partials(241, 4, 5)
    assert lr.violations(lr.emulate_finalize(p), lr.finalize64(p), lr.finalize_bound(p))[0] == 0


def test_embed_reference_counts_hits():
    tok = np.array([0, 3, 3, 5])
    dx = np.ones((4, 4), dtype=np.float32)
    ref, bound, hits = lr.embed64(np.zeros((6, 4)), [dict(tokens=tok, dx=dx, emb_scale=2.0, keep=None, p=0.0)])
    assert hits.tolist() == [1, 0, 0, 2, 0, 1] and ref[3, 0] == 4.0 and ref[1, 0] == 0.0
    assert bound[1, 0] == 0.0 and bound[3, 0] == lr.SECOND * (4 + 2 + lr.EMB_W + 1) * lr.U * 4.0
