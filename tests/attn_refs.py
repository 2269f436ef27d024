"""References for the unfused attention core (csrc/attention.hip, csrc/attn_mfma.h): plain torch on the CPU, no GPU imports.

  attn_ref      the operation in float64 (forward, backward and the {row max, 1 / row sum} pair the forward saves)
  attn_bound    the componentwise forward-error bound of the same chain: every operand by its absolute value, so nothing cancels
  attn_emulate  the chain in correctly rounded float32 with the kernels' documented rounding points (P, dS, O and the outputs are
                rounded to the compute type), optionally with the per-pass rounding of the no-workspace backward
  attn_check    the comparison both test files use: ratio = max |got - ref| / (u B) over B > 0, exact zeros where B == 0, relmax
  CASES         the shapes, shared by tests/test_attn_refs.py (CPU) and tests/test_attn_kernel_gpu.py
  BARS          the ratio each output may reach on the GPU; tests/test_attn_refs.py recomputes the table from attn_emulate against
                attn_ref (the reference side only, never the kernel) and asserts that it is what stands here

Tensors are packed-head [B, L, d] with d = h * dk, already rounded to the compute type.  A mask is bool [B | 1, 1 | a, m] with
False = masked, or None.  `keep` is the bool [B, h, a, m] dropout keep-mask of tests/dropout_refs.py, used with p.

Unit roundoffs: U["bf16"] = 2^-9 and U["fp32"] = 2^-24 scale the bound; the score / exponent error always enters with 2^-24 (the
kernels compute scores, exponentials and sums in float32 in both modes).

The bound, with S the masked scaled scores, P = softmax(S), c = keep / (1 - p) (1 without dropout):
  G    = |S - rowmax| + (|Q| |K|^T) / sqrt(dk)   where P > 0, else 0
  W0   = P (1 + (u32 / u) (G + rowsum(P G)))     W = W0 c
  B_O  = W |V|                                   B_dV = W^T |dO|
  B_dS = W (|dO| |V|^T) + W0 rowsum(|dO| B_O)    0 at masked scores
  B_dQ = B_dS |K| / sqrt(dk)                     B_dK = B_dS^T |Q| / sqrt(dk)
The second term of B_dS carries W0, not W: dS = P (c dP - D) keeps its -P D part where dropout removes the key from the row, so a
bound that scaled the whole of W by c would be 0 on elements whose true value is not (a key dropped for every one of a few query
rows), and the exact-zero rule below would then ask for zeros that are wrong.  Without dropout W0 = W.

Exact zeros: exp(-1e9 - max) is 0 in every precision, so in a row that is not fully masked a masked key has P == 0 exactly, and
B == 0 exactly where the true value is structurally 0: dK / dV rows of a key masked for every query, dQ rows and all dK of a fully
masked sample (its dV is not 0: the row is uniform over all m keys).  attn_check asks for got == 0 there.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from tests import dropout_refs as R

U = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -9}
U32 = 2.0 ** -24
TORCH_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16}
KINDS = ("O", "dQ", "dK", "dV")
RELMAX = {"fp32": 2e-5, "bf16": 1e-2}          # the project's bars on O (tests/test_kernels_gpu.py); twice that on the gradients
DROP_SEED = 0x1234567812345678

AttnRef = namedtuple("AttnRef", "O dQ dK dV rowmax invsum")


# ------------------------------------------------------------------------------------------ cases
def M(B, h, a, m, dk, mask, layout="plain", drop=None, kv_acc=None):
    """One member of a group launch.  mask: none | pad | perq | causal.  layout: plain | qkv3 | kv2 | padq.  drop: (p, salt) or None.
    kv_acc: None = as ops.attention_bwd does (an fp32 workspace for bf16 with a > 32), True = always given, False = NULL."""
    return dict(B=B, h=h, a=a, m=m, dk=dk, mask=mask, layout=layout, drop=drop, kv_acc=kv_acc)


def _case(cid, members, dtypes=("fp32", "bf16")):
    return dict(id=cid, members=list(members), dtypes=tuple(dtypes))


CASES = [
    _case("dk128", [M(2, 2, 20, 70, 128, "pad")]),
    _case("dk128_long", [M(1, 2, 70, 300, 128, "pad", "kv2")]),
    _case("valu_dk8", [M(2, 3, 33, 70, 8, "perq")]),
    _case("valu_dk48_a64", [M(2, 2, 64, 37, 48, "pad")]),
    _case("valu_dk96", [M(1, 2, 5, 33, 96, "none")]),
    _case("valu_stride", [M(2, 2, 20, 70, 64, "pad", "padq")], ("bf16",)),
    _case("nw4", [M(33, 8, 4, 260, 16, "pad")]),
    _case("self_packed", [M(2, 4, 70, 70, 32, "causal", "qkv3")]),
    _case("cross_perq", [M(2, 2, 37, 45, 64, "perq", "kv2")]),
    _case("nows_null", [M(2, 2, 70, 33, 64, "none", kv_acc=False)], ("bf16",)),
    _case("nows_ws", [M(2, 2, 70, 33, 64, "none", kv_acc=True)], ("bf16",)),
] + [
    _case(f"edge_a{a}_m{m}", [M(2, 2, a, m, 16, "pad")]) for a in (1, 32, 33, 64, 65) for m in (1, 33)
]
_G3 = [M(2, 2, 20, 20, 64, "causal", "qkv3"), M(3, 2, 70, 130, 64, "pad", "kv2", kv_acc=True),
       M(1, 2, 33, 300, 64, "perq", "plain", kv_acc=False)]
CASES += [
    _case("g3", _G3),
    _case("g3_reversed", _G3[::-1]),
    _case("g4", [M(2, 2, 7, 37, 32, "pad"), M(1, 4, 20, 20, 32, "causal", drop=(0.1, 5)), M(2, 2, 33, 70, 32, "perq"),
                 M(3, 2, 5, 130, 32, "pad", drop=(0.5, 9))]),
    _case("gmix", [M(2, 2, 20, 70, 64, "pad"), M(2, 2, 33, 37, 32, "perq")]),
]
CASE_BY_ID = {c["id"]: c for c in CASES}


def per_pass_rounding(mem, dtype):
    """True where the backward adds each 32-row query pass to bf16 sums in the output buffers (no fp32 workspace)."""
    ws = mem["kv_acc"] if mem["kv_acc"] is not None else True
    return dtype == "bf16" and mem["a"] > 32 and not ws


def bars_for(mem, dtype):
    return BARS["bf16_passes" if per_pass_rounding(mem, dtype) else dtype]


def make_mask(kind, B, a, m, g):
    if kind == "none":
        return None
    if kind == "causal":
        assert a == m
        return torch.tril(torch.ones(1, a, m, dtype=torch.bool))
    if kind == "pad":
        lens = torch.randint(min(m, max(2, m // 4)), m + 1, (B,), generator=g)    # at least two keys: one alone has no gradient
        mask = (torch.arange(m).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1)
        if B > 1:
            mask[B - 1] = False                   # an empty memory: uniform attention (with B == 1 it would be the whole case)
        return mask
    if kind == "perq":
        mask = torch.rand(B, a, m, generator=g) < 0.7
        mask[:, :, 0] = True                      # key 0 always kept ...
        mask[:, :, m - 1] = False                 # ... one key masked for every query ...
        mask[B - 1, a // 2, :] = False            # ... and one fully masked query row (it overrides key 0)
        return mask
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def inputs(case_id, idx, dtype):
    """dict(q, k, v, d_o, mask, keep, p) of member `idx` of a case: float32 tensors rounded to the compute type.  Cached and shared:
    never modify them."""
    case = CASE_BY_ID[case_id]
    mem = case["members"][idx]
    B, h, a, m, dk = (mem[k] for k in ("B", "h", "a", "m", "dk"))
    d = h * dk
    seed = 7919 * (B * 1000003 + h * 10007 + a * 101 + m * 13 + dk) + (1 if dtype == "bf16" else 0)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda L: torch.randn(B, L, d, generator=g).to(TORCH_DTYPE[dtype]).float()
    q, k, v, d_o = rnd(a), rnd(m), rnd(m), rnd(a)
    mask = make_mask(mem["mask"], B, a, m, g)
    keep, p = None, 0.0
    if mem["drop"]:
        p, salt = mem["drop"]
        keep = torch.from_numpy(R.keep_mask(DROP_SEED, salt, p, B * h * a * m)).reshape(B, h, a, m)
    return dict(q=q, k=k, v=v, d_o=d_o, mask=mask, keep=keep, p=p)


@functools.lru_cache(maxsize=None)
def reference(case_id, idx, dtype):
    """(AttnRef, bound dict) of a member, computed once."""
    x = inputs(case_id, idx, dtype)
    h = CASE_BY_ID[case_id]["members"][idx]["h"]
    ref = attn_ref(x["q"], x["k"], x["v"], x["d_o"], x["mask"], h, x["keep"], x["p"])
    bnd = attn_bound(x["q"], x["k"], x["v"], x["d_o"], x["mask"], h, U[dtype], x["keep"], x["p"])
    return ref, bnd


# ------------------------------------------------------------------------------------------ float64 chain
def _split(t, h):
    B, L, d = t.shape
    return t.reshape(B, L, h, d // h).transpose(1, 2)


def _merge(t):
    B, h, L, dk = t.shape
    return t.transpose(1, 2).reshape(B, L, h * dk)


def _masked(mask, B, h, a, m):
    if mask is None:
        return torch.zeros(B, h, a, m, dtype=torch.bool)
    return (mask == 0).unsqueeze(1).expand(B, h, a, m)


def _drop_scale(keep, p, dtype):
    """keep / (1 - p) with the kernels' float32 scale (dropout_refs.scale), or None."""
    if keep is None or not p > 0.0:
        return None
    return keep.to(dtype) * float(R.scale(p))


def _chain64(q, k, v, d_o, mask, h, keep, p):
    q, k, v, d_o = (_split(t.double(), h) for t in (q, k, v, d_o))
    B, _, a, dk = q.shape
    m = k.shape[2]
    rs = 1.0 / math.sqrt(dk)
    masked = _masked(mask, B, h, a, m)
    S = torch.where(masked, torch.full((), -1e9, dtype=torch.float64), (q @ k.transpose(-1, -2)) * rs)
    mx = S.max(dim=-1, keepdim=True).values
    E = torch.exp(S - mx)
    l = E.sum(dim=-1, keepdim=True)
    P = E / l
    c = _drop_scale(keep, p, torch.float64)
    return dict(q=q, k=k, v=v, d_o=d_o, rs=rs, masked=masked, S=S, mx=mx, l=l, P=P, c=c)


def attn_ref(q, k, v, d_o, mask, h, keep=None, p=0.0):
    """The attention core in float64: S = Q K^T / sqrt(dk) masked to -1e9, P = softmax(S), Pd = P keep / (1 - p), O = Pd V;
    D = rowsum(dO O), dP = (dO V^T) keep / (1 - p), dS = P (dP - D) with 0 at masked scores, dQ = dS K / sqrt(dk),
    dK = dS^T Q / sqrt(dk), dV = Pd^T dO.  rowmax / invsum are [B, h, a]: the row max of the masked scaled scores and
    1 / sum exp(S - max).  A fully masked row is uniform over all m keys."""
    x = _chain64(q, k, v, d_o, mask, h, keep, p)
    P, c = x["P"], x["c"]
    Pd = P if c is None else P * c
    O = Pd @ x["v"]
    D = (x["d_o"] * O).sum(dim=-1, keepdim=True)
    dP = x["d_o"] @ x["v"].transpose(-1, -2)
    if c is not None:
        dP = dP * c
    dS = torch.where(x["masked"], torch.zeros((), dtype=torch.float64), P * (dP - D))
    dQ = (dS @ x["k"]) * x["rs"]
    dK = (dS.transpose(-1, -2) @ x["q"]) * x["rs"]
    dV = Pd.transpose(-1, -2) @ x["d_o"]
    return AttnRef(_merge(O), _merge(dQ), _merge(dK), _merge(dV), x["mx"].squeeze(-1), (1.0 / x["l"]).squeeze(-1))


def attn_bound(q, k, v, d_o, mask, h, u, keep=None, p=0.0, u32=U32):
    """dict kind -> B, packed like the outputs (module docstring)."""
    x = _chain64(q, k, v, d_o, mask, h, keep, p)
    P, c = x["P"], x["c"]
    aq, ak, av, ado = x["q"].abs(), x["k"].abs(), x["v"].abs(), x["d_o"].abs()
    G = torch.where(P > 0, (x["S"] - x["mx"]).abs() + (aq @ ak.transpose(-1, -2)) * x["rs"], torch.zeros((), dtype=torch.float64))
    W0 = P * (1.0 + (u32 / u) * (G + (P * G).sum(dim=-1, keepdim=True)))
    W = W0 if c is None else W0 * c
    B_O = W @ av
    B_dV = W.transpose(-1, -2) @ ado
    B_dS = W * (ado @ av.transpose(-1, -2)) + W0 * (ado * B_O).sum(dim=-1, keepdim=True)
    B_dS = torch.where(x["masked"], torch.zeros((), dtype=torch.float64), B_dS)
    B_dQ = (B_dS @ ak) * x["rs"]
    B_dK = (B_dS.transpose(-1, -2) @ aq) * x["rs"]
    return dict(O=_merge(B_O), dQ=_merge(B_dQ), dK=_merge(B_dK), dV=_merge(B_dV))


# ------------------------------------------------------------------------------------------ emulation
def _f32(t):
    return t.float().double()


def _lp(t, lp):
    """float64 -> the compute type (through float32, as a kernel's store does) -> float64."""
    return t.float().to(lp).double()


WRONG = ("mask_row_off", "last_key_out", "head_off", "no_rescale", "dk_no_scale")


def attn_emulate(q, k, v, d_o, mask, h, lp, keep=None, p=0.0, passes=False, wrong=None):
    """The chain in float32 with the kernels' rounding points: every contraction, exponential and sum is rounded to float32 once
    (computed in float64, so the result does not depend on a BLAS's summation order or on a vector exp), and P (after dropout), dS,
    O and the four outputs are rounded to `lp`.  passes=True: the dK / dV sums are rounded to `lp` after every 32 query rows, the
    multi-pass backward without an fp32 workspace.  Returns an AttnRef of float64 tensors holding `lp` values.

    wrong = one of WRONG gives a deliberately wrong variant (tests/test_attn_refs.py: the check must catch each):
      mask_row_off   a per-query mask is read one query row off
      last_key_out   the last key is left out of the softmax
      head_off       K is read with its head base off by one head
      no_rescale     two key tiles; the running sum is not rescaled when the second tile raises the row max
      dk_no_scale    dK without the 1 / sqrt(dk)"""
    assert wrong is None or wrong in WRONG
    q, k, v, d_o = (_split(t.double(), h) for t in (q, k, v, d_o))
    B, _, a, dk = q.shape
    m = k.shape[2]
    rs = float(np.float32(1.0) / np.sqrt(np.float32(dk)))
    if wrong == "mask_row_off" and mask is not None and mask.shape[1] > 1:
        mask = torch.roll(mask, 1, dims=1)
    ks = torch.roll(k, 1, dims=1) if wrong == "head_off" else k
    masked = _masked(mask, B, h, a, m)
    zero = torch.zeros((), dtype=torch.float64)
    S = torch.where(masked, torch.full((), -1e9, dtype=torch.float64), _f32(_f32(q @ ks.transpose(-1, -2)) * rs))
    if wrong == "last_key_out" and m > 1:
        S = S.clone()
        S[..., m - 1] = -math.inf
    mx = S.max(dim=-1, keepdim=True).values
    E = _f32(torch.exp(_f32(S - mx)))
    l = _f32(E.sum(dim=-1, keepdim=True))
    if wrong == "no_rescale" and m > 1:
        t = m // 2
        m1 = S[..., :t].max(dim=-1, keepdim=True).values
        l = _f32(torch.exp(S[..., :t] - m1).sum(dim=-1, keepdim=True) + E[..., t:].sum(dim=-1, keepdim=True))
    inv = _f32(1.0 / l)
    P = _f32(E * inv)
    c = _drop_scale(keep, p, torch.float64)
    Pd = _lp(P if c is None else _f32(P * c), lp)
    O = _lp(_f32(Pd @ v), lp)
    D = _f32((d_o * O).sum(dim=-1, keepdim=True))
    dP = _f32(d_o @ v.transpose(-1, -2))
    if c is not None:
        dP = _f32(dP * c)
    dS = _lp(torch.where(masked, zero, _f32(P * _f32(dP - D))), lp)
    dQ = _lp(_f32(_f32(dS @ ks) * rs), lp)
    rk = 1.0 if wrong == "dk_no_scale" else rs
    if passes:
        dK, dV = torch.zeros_like(k), torch.zeros_like(v)
        for q0 in range(0, a, 32):
            sl = slice(q0, min(q0 + 32, a))
            dK = _lp(_f32(dK + _f32(_f32(dS[:, :, sl].transpose(-1, -2) @ q[:, :, sl]) * rk)), lp)
            dV = _lp(_f32(dV + _f32(Pd[:, :, sl].transpose(-1, -2) @ d_o[:, :, sl])), lp)
    else:
        dK = _lp(_f32(_f32(dS.transpose(-1, -2) @ q) * rk), lp)
        dV = _lp(_f32(Pd.transpose(-1, -2) @ d_o), lp)
    return AttnRef(_merge(O), _merge(dQ), _merge(dK), _merge(dV), mx.squeeze(-1), inv.squeeze(-1))


# ------------------------------------------------------------------------------------------ the check
def ratio(got, ref, bnd, u):
    """(max |got - ref| / (u B) over B > 0, its flat index, number of elements with B == 0 and got != 0)."""
    got, ref = got.double(), ref.double()
    live = bnd > 0
    r = torch.where(live, (got - ref).abs() / (u * torch.where(live, bnd, torch.ones_like(bnd))), torch.zeros_like(bnd))
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))          # a NaN in `got` must not hide in max()
    worst = int(r.argmax())
    return float(r.reshape(-1)[worst]), worst, int(((got != 0) & ~live).sum())


def attn_check(got, ref, bnd, dtype, bars):
    """got: dict kind -> tensor packed [B, L, d].  Returns (ratios, failures): ratios[kind] = (ratio, (b, row, col) of the worst element),
    failures = one line per broken rule (ratio above its bar, a non-zero where B == 0, a non-finite value, relmax above the project's
    bar).  Both test files go through here."""
    ratios, failures = {}, []
    for kind in KINDS:
        g, r, b = got[kind].double(), getattr(ref, kind), bnd[kind]
        if not bool(torch.isfinite(g).all()):
            failures.append(f"{kind}: {int((~torch.isfinite(g)).sum())} non-finite elements")
        val, worst, nonzero = ratio(g, r, b, U[dtype])
        ratios[kind] = (val, tuple(int(i) for i in np.unravel_index(worst, tuple(g.shape))))
        if not val <= bars[kind]:
            failures.append(f"{kind}: ratio {val:.3g} > bar {bars[kind]:.3g} at {ratios[kind][1]}")
        if nonzero:
            failures.append(f"{kind}: {nonzero} non-zero elements where the bound is 0")
        # relmax (tests/util.py) divides by the largest reference entry.  With a single key dQ and dK are 0 analytically and the
        # float64 reference holds only its own cancellation noise (1e-16): there is nothing to be relative to, the ratio above
        # (against B, which does not cancel) is the whole check
        rmax = float(r.abs().max())
        rel = float((g - r).abs().max() / max(1e-6, rmax))
        tol = RELMAX[dtype] * (1 if kind == "O" else 2)
        if rmax > 1e-9 and not rel < tol:
            failures.append(f"{kind}: relmax {rel:.3g} >= {tol:.3g}")
    return ratios, failures


# ------------------------------------------------------------------------------------------ bars
def bar_of(r_emu_max):
    """max(4 r_emu, 4), rounded up to 1/100.  x 4: the kernels sum tile by tile with one online-softmax rescale per key tile, use the
    hardware exp and rsqrt and combine up to 8 waves, none of which attn_emulate does.  Floor 4: ratio == 1 is the first-order bound
    of a single rounding stage and the chain has about four."""
    return math.ceil(max(4.0 * r_emu_max, 4.0) * 100.0 - 1e-9) / 100.0


# Filled from tests/test_attn_refs.py::test_bars_are_the_measured_ones (which prints the table it measures).  "bf16_passes" holds for
# members whose backward rounds dK / dV to bf16 after every 32-row pass (per_pass_rounding); its O and dQ are the bf16 ones.
BARS = {
    "fp32": {"O": 4.0, "dQ": 4.0, "dK": 4.0, "dV": 4.0},
    "bf16": {"O": 11.51, "dQ": 4.0, "dK": 5.2, "dV": 14.38},
    "bf16_passes": {"O": 11.51, "dQ": 4.0, "dK": 5.2, "dV": 14.38},
}
