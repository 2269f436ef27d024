"""References for the persistent decode step (csrc/decode.hip, include/mtn_hip.h mtn_decode_step): plain torch on the CPU, no GPU imports.

  build_case  random tensors for a stage list, directly (no Model): bf16 weights in nn.Linear layout, fp32 biases, LayerNorm gains,
              lut, pe, hoisted k | v, masks, prefix caches, and per step {tokens, pos, anc}
  step_ref    the step in float64 on those (bf16-rounded) operands with no intermediate rounding, by the definitions of
              include/mtn_hip.h: LayerNorm with the unbiased std and eps added to the std, masked scores -1e9, prefix position t of
              hypothesis j read from cache slot anc[j][t], the newest k | v written to slot j at pos
  step_emul   the same walk in float32 with the kernel's rounding points: LayerNorm output, q, the q | k | v granules,
              probabilities, attention output, FFN hidden and out_lp rounded to bf16; x stays fp32
  run_case    every step of a case in turn (a step's new cache rows are stored in the cache's own type before the next one reads them)
  CASES       the shapes, shared by tests/test_decode_refs.py (CPU) and tests/test_decode_step_kernel_gpu.py
  CPU_EMUL_*  the worst |step_emul - step_ref| over CASES per kind of output, relative to the row's largest |ref|: the bf16
              rounding budget of the step.  tests/test_decode_refs.py re-measures them (the reference side only, never the kernel).

A step's result is a dict: x {stage: [W, d]} after every stage that writes x, qkv {stage: [W, 3d]}, att {stage: [W, d]} (the output
of every attention), hid {stage: [W, d_ff]}, out_lp [W, d], cache_rows {cache index: [W, 2d]}, and for the attentions q / scores / p
per (hypothesis, head).

Load-bearing inputs, so that an indexing mistake is an O(1) error or a NaN, never rounding noise:
  * bf16 NaN in every cache slot at a position t < pos that no anc[j][t] names, and in every cache row at positions >= pos (the row
    at pos is written by the step);
  * masked keys: NaN K rows (the score is replaced by -1e9 whatever it was) and V rows of magnitude 1e3 (their probability is
    exactly 0 unless the whole row is masked);
  * mask bytes beyond m (mask_stride > m) hold the opposite of the row's last real byte;
  * planted keys: for named (hypothesis, head) pairs the K row at an edge index (0, m - 1, 127, 128, 255, 256, pos) is a multiple of
    the reference q, scaled so that the key takes >= 0.9 of the reference probability.  build_case asserts that every planted pair
    reaches 0.9 in step_ref; a kernel that drops or misplaces that key is wrong by most of the row.
"""
import functools
import math

import torch

EMBED, SELF_QKV, SELF_ATT, OUT, CROSS, FFN1, FFN2, FINAL = range(8)       # include/mtn_hip.h MTN_DEC_*
X_WRITERS = (EMBED, OUT, FFN2)
BF16_ULP = 2.0 ** -8                  # spacing of bf16 in [1, 2): one ulp of v is at most BF16_ULP * |v|
MARGIN = 4.0                          # tests/test_row_kernels_gpu.py: fast-math intrinsics and a different summation order
PLANT_P = 0.9
EDGES = (256, 255, 128, 127, 0)       # besides m - 1 and pos

# Worst |step_emul - step_ref| / (row's largest |ref|) over CASES.  Measured with
#     python -c "from tests import decode_refs as R; print(R.measure_constants())"
CPU_EMUL_QKV = 4.73e-3
CPU_EMUL_ATT = 1.03e-2
CPU_EMUL_HID = 5.10e-3
CPU_EMUL_X = 3.63e-3
CPU_EMUL_OUT_LP = 4.96e-3
CPU_EMUL_CACHE = 4.31e-3
CONSTANTS = ("QKV", "ATT", "HID", "X", "OUT_LP", "CACHE")


def bound(kind, ref, bf16_out):
    """The elementwise bound of an output against step_ref: MARGIN x CPU_EMUL_<kind> x the row's largest |ref|, plus one bf16 ulp of the
    reference element where the output is stored as bf16."""
    b = MARGIN * globals()["CPU_EMUL_" + kind] * ref.abs().amax(-1, keepdim=True).expand_as(ref)
    return b + BF16_ULP * ref.abs() if bf16_out else b


# ------------------------------------------------------------------------------------------ the step
def _ln(x, a, b, eps):
    d = x.shape[-1]
    xc = x - x.sum(-1, keepdim=True) / d
    std = torch.sqrt((xc * xc).sum(-1, keepdim=True) / (d - 1))
    return a * xc / (std + eps) + b


def _step(case, stp, caches, emul):
    dt = torch.float32 if emul else torch.float64
    rb = (lambda t: t.to(torch.bfloat16).to(dt)) if emul else (lambda t: t)
    W, d, h = case["W"], case["d"], case["h"]
    dk = d // h
    pos, anc, tokens = stp["pos"], stp["anc"].long(), stp["tokens"]
    res = dict(x={}, qkv={}, att={}, hid={}, cache_rows={}, q={}, scores={}, p={})
    x = qkv = att = hid = None
    lnorm = lambda S, v: rb(_ln(v, S["ln_a"].to(dt), S["ln_b"].to(dt), S["ln_eps"]))
    lin = lambda S, v: v @ S["w"].to(dt).t() + S["bias"].to(dt)

    def attend(si, q, kv, mask):
        """q [W, d]; kv [W, m, 2d] (NaN allowed in masked K rows); mask [W, m] (0 = masked) or None -> [W, d]"""
        m = kv.shape[1]
        qh = q.reshape(W, h, dk)
        k, v = kv[..., :d].reshape(W, m, h, dk), kv[..., d:].reshape(W, m, h, dk)
        s = torch.einsum("jhc,jthc->jht", qh, k) / math.sqrt(dk)
        if mask is not None:
            s = torch.where((mask == 0).unsqueeze(1), torch.full_like(s, -1e9), s)
        p = rb(torch.softmax(s, dim=-1))
        res["q"][si], res["scores"][si], res["p"][si] = qh, s, p
        return rb(torch.einsum("jht,jthc->jhc", p, v).reshape(W, d))

    for si, S in enumerate(case["stages"]):
        kind = S["kind"]
        if kind == EMBED:
            x = case["lut"].to(dt)[tokens] * case["emb_scale"] + case["pe"].to(dt)[pos]
        elif kind == SELF_QKV:
            qkv = rb(lin(S, lnorm(S, x)))
            res["qkv"][si] = qkv
            res["cache_rows"][S["cache"]] = qkv[:, d:]
        elif kind == SELF_ATT:
            old = caches[S["cache"]][anc[:, :pos], torch.arange(pos)].to(dt)          # [W, pos, 2d]: slot anc[j][t] at position t
            att = attend(si, qkv[:, :d], torch.cat([old, qkv[:, d:].unsqueeze(1)], dim=1), None)
            res["att"][si] = att
        elif kind == CROSS:
            mask = None if S["mask"] is None else S["mask"][:, :S["m"]]
            att = attend(si, rb(lin(S, lnorm(S, x))), S["kv"].to(dt), mask)
            res["att"][si] = att
        elif kind == OUT:
            x = x + lin(S, att)
        elif kind == FFN1:
            hid = rb(torch.relu(lin(S, lnorm(S, x))))
            res["hid"][si] = hid
        elif kind == FFN2:
            x = x + lin(S, hid)
        elif kind == FINAL:
            res["out_lp"] = lnorm(S, x)
        if kind in X_WRITERS:
            res["x"][si] = x
    return res


def step_ref(case, stp, caches):
    return _step(case, stp, caches, emul=False)


def step_emul(case, stp, caches):
    return _step(case, stp, caches, emul=True)


def run_case(case, emul=False, caches=None):
    """Every step of the case -> (list of results, the caches afterwards).  The caches are copies in the case's own cache type."""
    caches = [c.clone() for c in (case["caches"] if caches is None else caches)]
    out = []
    for stp in case["steps"]:
        r = _step(case, stp, caches, emul)
        for ci, rows in r["cache_rows"].items():
            caches[ci][torch.arange(case["W"]), stp["pos"]] = rows.to(caches[ci].dtype)
        out.append(r)
    return out, caches


# ------------------------------------------------------------------------------------------ cases
def spec(cid, kind, d, h, W, L=8, pos=0, m=0, mask="none", d_ff=None, n_mid=None, seed=0):
    """kind: cross | self | ffn | whole.  mask (cross): none | ragged | hole | full | stride.  n_mid: the wide class's size the launch
    is to be given (None: the whole device)."""
    return dict(id=cid, kind=kind, d=d, h=h, W=W, L=L, pos=pos, m=m, mask=mask, d_ff=d_ff or 2 * d, n_mid=n_mid, seed=seed)


def _cases():
    out = []
    # cross-attention: every m at both head sizes; W and mask dealt so that each mask meets each W
    table = [(1, "none", 1), (1, "full", 9), (2, "ragged", 16), (2, "stride", 1), (127, "ragged", 9), (128, "full", 16), (128, "none", 1),
             (129, "stride", 9), (255, "hole", 16), (256, "ragged", 1), (256, "stride", 16), (257, "hole", 9), (257, "none", 16),
             (300, "full", 9), (300, "hole", 16), (300, "ragged", 16), (1024, "hole", 1), (1024, "stride", 16), (1024, "full", 9),
             (1024, "none", 16)]
    for d in (128, 256):
        for i, (m, mask, W) in enumerate(table):
            out.append(spec(f"cross_d{d}_m{m}_{mask}_w{W}", "cross", d, 4, W, m=m, mask=mask, seed=100 + i))
    Ws = (16, 1, 9)
    for d in (128, 256):
        for i, pos in enumerate((0, 1, 127, 128, 129, 255, 256, 257, 300)):
            out.append(spec(f"self_d{d}_pos{pos}_w{Ws[i % 3]}", "self", d, 4, Ws[i % 3], L=320, pos=pos, seed=200 + i))
        out.append(spec(f"self_d{d}_pos1023_w16", "self", d, 4, 16, L=1024, pos=1023, seed=210))
        out.append(spec(f"ffn_d{d}_w16", "ffn", d, 4, 16, seed=220))
        out.append(spec(f"ffn_d{d}_w9", "ffn", d, 4, 9, d_ff=3 * d + 32, seed=221))
    # slice plans of the small-M Linear: d 512, h 8, one row; q | k | v slices of 64, 48, 32, 16, 12 features, FFN-1 slices of 52, 36, 28, 12, 16
    for n_mid, dff in ((24, 1248), (32, 1152), (48, 1344), (96, 1152), (128, 2048)):
        out.append(spec(f"plan_self_nmid{n_mid}", "self", 512, 8, 1, L=8, pos=3, d_ff=dff, n_mid=n_mid, seed=300 + n_mid))
        out.append(spec(f"plan_ffn_nmid{n_mid}_dff{dff}", "ffn", 512, 8, 1, d_ff=dff, n_mid=n_mid, seed=400 + n_mid))
    # the row limit at d_ff = 4096: contraction steps beyond the prefetched ones (q | k | v slices of 48, FFN-1 slices of 64)
    out.append(spec("plan_self_d1024_w8", "self", 1024, 16, 8, L=8, pos=3, d_ff=4096, seed=500))
    out.append(spec("plan_ffn_d1024_w8", "ffn", 1024, 16, 8, d_ff=4096, seed=501))
    out.append(spec("whole_d128_w13", "whole", 128, 4, 13, L=16, pos=5, seed=600))
    out.append(spec("whole_d256_w16", "whole", 256, 4, 16, L=16, pos=5, seed=601))
    return out


CASES = _cases()
CASE_BY_ID = {c["id"]: c for c in CASES}


def make_mask(kind, W, m, g):
    """uint8 [W, mask_stride] (1 = keep) or None.  Hypothesis 0 keeps every key except in `hole`."""
    if kind == "none":
        return None
    stride = m + 5 if kind == "stride" else m
    t = torch.arange(m)
    if kind == "hole":        # keys masked inside the row, on both sides of key 256: hypothesis j loses t >= 256 with (t + j) % 3 == 2
        j = torch.arange(W).unsqueeze(1)
        keep = ~(((t.unsqueeze(0) >= 256) & ((t.unsqueeze(0) + j) % 3 == 2)) | ((t.unsqueeze(0) < 256) & ((t.unsqueeze(0) + 5 * j) % 11 == 5)))
        if m <= 256 and W > 1:
            keep[1:, m // 2] = False
    else:                     # ragged per hypothesis
        lens = torch.randint(max(1, m // 2), m + 1, (W,), generator=g)
        lens[0] = m
        keep = t.unsqueeze(0) < lens.unsqueeze(1)
        if kind == "full":
            keep[W - 1] = False               # one fully masked hypothesis: uniform over all m keys
    mask = torch.empty(W, stride, dtype=torch.uint8)
    mask[:, :m] = keep.to(torch.uint8)
    mask[:, m:] = 1 - mask[:, m - 1:m]        # padding bytes: the opposite of the last real byte
    return mask


def _bf(t):
    return t.to(torch.bfloat16)


def build_tensors(sp, wdtype=torch.bfloat16, fdtype=torch.float32):
    """The case without planted keys.  wdtype: the type of weights, k | v and caches (bf16 for the kernel; the oracle check builds float64)."""
    g = torch.Generator().manual_seed(sp["seed"])
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    W, d, h, L, dff, pos = sp["W"], sp["d"], sp["h"], sp["L"], sp["d_ff"], sp["pos"]
    V = 37
    nan = float("nan")
    case = dict(id=sp["id"], W=W, d=d, h=h, L=L, d_ff=dff, n_mid=sp["n_mid"], max_m=1, caches=[], planted=[],
                lut=(rn(V, d) / math.sqrt(d)).to(fdtype), pe=(0.5 * rn(L, d)).to(fdtype), emb_scale=float(torch.tensor(math.sqrt(d), dtype=fdtype)))
    ln = lambda: dict(ln_a=(1 + 0.1 * rn(d)).to(fdtype), ln_b=(0.1 * rn(d)).to(fdtype), ln_eps=1e-6)
    lin = lambda N, K: dict(N=N, K=K, w=(rn(N, K) / math.sqrt(K)).to(wdtype), bias=(0.1 * rn(N)).to(fdtype))
    st = [dict(kind=EMBED)]

    def self_att():
        case["caches"].append(rn(W, L, 2 * d).to(wdtype))
        ci = len(case["caches"]) - 1
        st.append(dict(kind=SELF_QKV, cache=ci, **lin(3 * d, d), **ln()))
        st.append(dict(kind=SELF_ATT, cache=ci))
        st.append(dict(kind=OUT, **lin(d, d)))

    def cross(m, mkind):
        mask = make_mask(mkind, W, m, g)
        kv = rn(W, m, 2 * d)
        if mask is not None:
            dead = mask[:, :m] == 0
            kv[..., :d][dead] = nan
            kv[..., d:][dead] = 1e3 * torch.sign(kv[..., d:][dead])
        st.append(dict(kind=CROSS, kv=kv.to(wdtype), m=m, mask=mask, mask_stride=m if mask is None else mask.shape[1], **lin(d, d), **ln()))
        st.append(dict(kind=OUT, **lin(d, d)))
        case["max_m"] = max(case["max_m"], m)

    def ffn():
        st.append(dict(kind=FFN1, **lin(dff, d), **ln()))
        st.append(dict(kind=FFN2, **lin(d, dff)))

    if sp["kind"] == "cross":
        cross(sp["m"], sp["mask"])
    elif sp["kind"] == "self":
        self_att()
    elif sp["kind"] == "ffn":
        ffn()
    else:
        for _ in range(2):
            self_att(); cross(300, "ragged"); cross(37, "stride"); ffn()
    st.append(dict(kind=FINAL, **ln()))
    case["stages"] = st
    # steps: random ancestors with anc[j][pos] = j; a whole case takes a second step whose rows descend from random parents
    anc = torch.randint(0, W, (W, L), generator=g, dtype=torch.int32)
    anc[:, pos] = torch.arange(W, dtype=torch.int32)
    steps = [dict(tokens=torch.randint(0, V, (W,), generator=g), pos=pos, anc=anc)]
    if sp["kind"] == "whole":
        parent = torch.randint(0, W, (W,), generator=g)
        anc2 = anc[parent].clone()
        anc2[:, pos + 1] = torch.arange(W, dtype=torch.int32)
        steps.append(dict(tokens=torch.randint(0, V, (W,), generator=g), pos=pos + 1, anc=anc2, parent=parent))
    case["steps"] = steps
    for c in case["caches"]:
        used = torch.zeros(W, L, dtype=torch.bool)
        used[anc[:, :pos].long(), torch.arange(pos)] = True
        c[~used] = nan
    return case


def _plant(case, si, j, hd, e):
    """Make key e the one (hypothesis j, head hd) of attention stage si looks at: its K row becomes c x the reference q."""
    d, dk = case["d"], case["d"] // case["h"]
    stp = case["steps"][0]
    r = step_ref(case, stp, case["caches"])
    q, s = r["q"][si][j, hd], r["scores"][si][j, hd].clone()
    s[e] = -float("inf")
    c = (math.log(PLANT_P / (1 - PLANT_P)) + float(torch.logsumexp(s, 0)) + 1.0) * math.sqrt(dk) / float(q @ q)
    S = case["stages"][si]
    cols = slice(hd * dk, (hd + 1) * dk)
    if S["kind"] == CROSS:
        S["kv"][j, e, cols] = (c * q).to(S["kv"].dtype)
    elif e < stp["pos"]:
        case["caches"][S["cache"]][int(stp["anc"][j, e]), e, cols] = (c * q).to(case["caches"][S["cache"]].dtype)
    else:                     # the newest key comes out of the projection: this head's k is made constant, W_k rows zero and b_k = c q
        P = case["stages"][si - 1]
        P["w"][d + hd * dk:d + (hd + 1) * dk] = 0
        P["bias"][d + hd * dk:d + (hd + 1) * dk] = (c * q).to(P["bias"].dtype)
    case["planted"].append((si, j, hd, e))


def planted_ok(case):
    """The builder's condition: every planted (stage, hypothesis, head, key) holds >= PLANT_P of the reference probability."""
    if not case["planted"]:
        return True, 1.0
    r = step_ref(case, case["steps"][0], case["caches"])
    worst = min(float(r["p"][si][j, hd, e]) for si, j, hd, e in case["planted"])
    return worst >= PLANT_P, worst


@functools.lru_cache(maxsize=None)
def build_case(cid):
    sp = CASE_BY_ID[cid]
    case = build_tensors(sp)
    if sp["kind"] in ("cross", "self") and sp["n_mid"] is None:
        si = 1 if sp["kind"] == "cross" else 2
        W, h = case["W"], case["h"]
        m = sp["m"] if sp["kind"] == "cross" else sp["pos"] + 1
        mask = case["stages"][si].get("mask")
        edges = [m - 1] + [e for e in EDGES if e < m - 1]          # (self: m - 1 is pos, planted first: it changes the other rows' scores)
        taken = set()
        for i, e in enumerate(edges):
            if m == 1:
                break                                                # a single key has probability 1 whatever it is
            for n in range(W * h):                                   # the first free pair, j and head both moving, whose key e is not masked
                j, hd = (3 * i + 1 + n) % W, (i + n // W) % h
                if (j, hd) not in taken and (mask is None or int(mask[j, e]) == 1):
                    taken.add((j, hd))
                    _plant(case, si, j, hd, e)
                    break
        ok, worst = planted_ok(case)
        assert ok, f"{cid}: a planted key holds only {worst:.3f} of its row"
    return case


# ------------------------------------------------------------------------------------------ the rounding budget
def _rel(got, ref):
    return float(((got.double() - ref).abs() / ref.abs().amax(-1, keepdim=True).clamp_min(1e-30)).max())


def case_budget(case):
    """max |step_emul - step_ref| / row max |ref| per kind of output, over the steps of one case"""
    refs, _ = run_case(case, emul=False)
    emus, _ = run_case(case, emul=True)
    out = dict.fromkeys(CONSTANTS, 0.0)
    for r, e in zip(refs, emus):
        for kind, key in (("QKV", "qkv"), ("ATT", "att"), ("HID", "hid"), ("X", "x")):
            for si in r[key]:
                out[kind] = max(out[kind], _rel(e[key][si], r[key][si]))
        out["OUT_LP"] = max(out["OUT_LP"], _rel(e["out_lp"], r["out_lp"]))
        for ci in r["cache_rows"]:
            out["CACHE"] = max(out["CACHE"], _rel(e["cache_rows"][ci], r["cache_rows"][ci]))
    return out


def measure_constants():
    out = dict.fromkeys(CONSTANTS, 0.0)
    for sp in CASES:
        b = case_budget(build_case(sp["id"]))
        out = {k: max(out[k], b[k]) for k in out}
    return out
