"""The unfused attention core (csrc/attention.hip, csrc/attn_mfma.h) through its C entry points mtn_attention_fwd_group /
mtn_attention_bwd_group, against the float64 reference and the componentwise bound of tests/attn_refs.py.

What the cases of attn_refs.CASES reach, by the host dispatch rules (forward key tiles of 64, backward key tiles of 32 and query
passes of 32; MFMA for one head size in {16, 32, 64, 128} with 8-element row strides, else the VALU kernels):
  dk128          MFMA DK = 128, 2 waves forward (2 tiles), 2 waves backward (3 tiles)
  dk128_long     MFMA DK = 128, 5 forward / 10 backward tiles in a small launch: 8 waves wanted.  bf16 takes them (backward 153,728 B of
                 LDS); fp32 takes 4, the largest count that fits 160 KB; 3 query passes; K | V column blocks of one buffer
  valu_dk8       VALU forward, 2 query blocks x 2 key tiles; VALU backward with a = 33 rounded up to 36 rows; per-query mask
  valu_dk48_a64  VALU backward at its 64-row limit
  valu_dk96      VALU, the largest LDS image of a head size the MFMA path does not take
  valu_stride    bf16, d_k = 64 but q / dq rows padded to d + 4: the VALU kernels by stride
  nw4            B h = 264 > 256 workgroups: 4 waves forward (5 tiles) and 4 waves backward (9 tiles)
  self_packed    q | k | v column blocks of one [rows, 3 d] buffer, causal mask broadcast over the batch (mask_sb = 0), 3 passes
  cross_perq     per-query mask with a batch stride, K | V packed, keys over a tile edge: the per-query branch of both MFMA kernels
  nows_null/_ws  bf16, 3 passes: dK / dV summed in the bf16 output buffers (kv_acc = NULL), and in the fp32 workspace
  edge_*         a in {1, 32, 33, 64, 65} x m in {1, 33}: pass and tile boundaries
  g3, g3_reversed  three members, one launch: grid.x = 6 with members of 4 and 2 workgroups, 8 waves forward with one member solo,
                 backward passes with 3, 2 and 1 members (member indices shift), kv_acc per member
  g4             four members, dropout on two of them with their own (p, salt)
  gmix           d_k = 64 and 32 in one group: the VALU kernels

Every output buffer (guard rows and pad columns included) is prefilled with NaN; afterwards every in-range element is finite and
everything else still holds the NaN bit for bit."""
import ctypes as C
import math

import pytest
import torch

from tests import attn_refs as A

pytestmark = pytest.mark.gpu

GUARD = 8                     # sentinel rows before and after every output (8 rows keep any row stride 16-byte aligned)
MTN_ERR_ARG = 1


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class _Out:
    """An output buffer [GUARD + rows + GUARD, ld] of NaN with named column blocks {name: (col, width)}; columns outside the blocks
    are pad."""

    def __init__(self, dev, tdt, rows, ld, blocks):
        self.full = torch.full((rows + 2 * GUARD, ld), float("nan"), dtype=tdt, device=dev)
        self.rows, self.ld, self.blocks = rows, ld, blocks
        self.bits = torch.int32 if tdt == torch.float32 else torch.int16
        self.sentinel = self.full[:1, :1].view(self.bits).clone()

    def ptr(self, name):
        return self.full.data_ptr() + (GUARD * self.ld + self.blocks[name][0]) * self.full.element_size()

    def untouched(self):
        return bool((self.full.view(self.bits) == self.sentinel).all())

    def check(self, what):
        """In-range elements finite, everything else the sentinel bit for bit."""
        inside = torch.zeros(self.full.shape, dtype=torch.bool, device=self.full.device)
        for col, width in self.blocks.values():
            inside[GUARD:GUARD + self.rows, col:col + width] = True
        same = self.full.view(self.bits) == self.sentinel
        assert bool(same[~inside].all()), f"{what}: {int((~same[~inside]).sum())} guard / pad elements were written"
        assert bool(torch.isfinite(self.full[inside]).all()), f"{what}: {int((~torch.isfinite(self.full[inside])).sum())} in-range elements not finite"

    def get(self, name, B):
        col, width = self.blocks[name]
        return self.full[GUARD:GUARD + self.rows, col:col + width].float().cpu().reshape(B, self.rows // B, width)


def build_group(dev, dtype, members):
    """members: list of (member description, inputs dict) -> (AttnArgs array, per-member state).  Nothing is launched."""
    from mtn_amd import lib as L, ops
    tdt = A.TORCH_DTYPE[dtype]
    arr = (L.AttnArgs * len(members))()
    state = []
    for i, (mem, x) in enumerate(members):
        B, h, a, m, dk, layout = (mem[n] for n in ("B", "h", "a", "m", "dk", "layout"))
        d = h * dk
        flat = lambda t: t.reshape(-1, d).to(dev, tdt)
        st = dict(keep=[])
        es = torch.empty((), dtype=tdt).element_size()
        args = arr[i]
        args.B, args.h, args.a, args.m, args.dk = B, h, a, m, dk
        if layout == "qkv3":                       # q | k | v and dq | dk | dv: column blocks of one [rows, 3 d] buffer
            assert a == m
            qkv = torch.cat([flat(x["q"]), flat(x["k"]), flat(x["v"])], dim=1).contiguous()
            st["keep"].append(qkv)
            args.q, args.k, args.v, args.ldq, args.ldkv = qkv.data_ptr(), qkv.data_ptr() + d * es, qkv.data_ptr() + 2 * d * es, 3 * d, 3 * d
            g = _Out(dev, tdt, B * a, 3 * d, dict(dQ=(0, d), dK=(d, d), dV=(2 * d, d)))
            st["outs"] = dict(dQ=g, dK=g, dV=g)
        else:
            ldq = d + 4 if layout == "padq" else d
            qb = torch.full((B * a, ldq), float("nan"), dtype=tdt, device=dev)
            qb[:, :d] = flat(x["q"])
            if layout == "kv2":                    # k | v of one [rows, 2 d] buffer
                kv = torch.cat([flat(x["k"]), flat(x["v"])], dim=1).contiguous()
                st["keep"] += [qb, kv]
                args.k, args.v, args.ldkv = kv.data_ptr(), kv.data_ptr() + d * es, 2 * d
                gkv = _Out(dev, tdt, B * m, 2 * d, dict(dK=(0, d), dV=(d, d)))
                st["outs"] = dict(dK=gkv, dV=gkv)
            else:
                kb, vb = flat(x["k"]).contiguous(), flat(x["v"]).contiguous()
                st["keep"] += [qb, kb, vb]
                args.k, args.v, args.ldkv = kb.data_ptr(), vb.data_ptr(), d
                st["outs"] = dict(dK=_Out(dev, tdt, B * m, d, dict(dK=(0, d))), dV=_Out(dev, tdt, B * m, d, dict(dV=(0, d))))
            args.q, args.ldq = qb.data_ptr(), ldq
            st["outs"]["dQ"] = _Out(dev, tdt, B * a, ldq, dict(dQ=(0, d)))
        st["outs"]["O"] = _Out(dev, tdt, B * a, d, dict(O=(0, d)))
        st["lse"] = _Out(dev, torch.float32, B * h * a, 2, dict(lse=(0, 2)))
        if x["mask"] is not None:
            mk = x["mask"].to(torch.uint8).contiguous().to(dev)
            st["keep"].append(mk)
            args.mask = mk.data_ptr()
            args.mask_sb = 0 if mk.size(0) == 1 else mk.size(1) * m
            args.mask_sq = 0 if mk.size(1) == 1 else m
        if mem["drop"]:
            seed = torch.full((1,), A.DROP_SEED, device=dev, dtype=torch.int64)
            st["keep"].append(seed)
            args.drop = ops._drop(mem["drop"][0], mem["drop"][1], seed)
        d_o = flat(x["d_o"]).contiguous()
        st["keep"].append(d_o)
        args.o, args.ldo, args.lse = st["outs"]["O"].ptr("O"), d, st["lse"].ptr("lse")
        args.d_o = d_o.data_ptr()
        args.dq, args.dk_out, args.dv_out = (st["outs"][n].ptr(n) for n in ("dQ", "dK", "dV"))
        ws = mem["kv_acc"] if mem["kv_acc"] is not None else (dtype == "bf16" and a > 32)
        if ws:
            st["ws"] = torch.full((2, B * m, d), float("nan"), device=dev, dtype=torch.float32)
            args.kv_acc = st["ws"].data_ptr()
        state.append(st)
    return arr, state


def all_untouched(state):
    return all(o.untouched() for st in state for o in list(st["outs"].values()) + [st["lse"]])


def run_group(dev, dtype, members):
    """One mtn_attention_fwd_group and one mtn_attention_bwd_group launch over `members`; checks the sentinels; returns per member
    dict(O, dQ, dK, dV: float32 CPU [B, L, d]; lse: [B, h, a, 2])."""
    from mtn_amd import lib as L
    lib = L.load()
    arr, state = build_group(dev, dtype, members)
    code = L.dtype_code(A.TORCH_DTYPE[dtype])
    L.check(lib.mtn_attention_fwd_group(code, len(members), arr, L.stream_ptr()))
    L.check(lib.mtn_attention_bwd_group(code, len(members), arr, L.stream_ptr()))
    torch.cuda.synchronize()
    res = []
    for i, ((mem, x), st) in enumerate(zip(members, state)):
        B, h, a, m = (mem[n] for n in ("B", "h", "a", "m"))
        for o in {id(o): o for o in st["outs"].values()}.values():
            o.check(f"member {i} {'|'.join(o.blocks)}")
        st["lse"].check(f"member {i} lse")
        r = {kind: st["outs"][kind].get(kind, B) for kind in A.KINDS}
        r["lse"] = st["lse"].full[GUARD:GUARD + B * h * a].cpu().reshape(B, h, a, 2)
        res.append(r)
    return res


def check_lse(lse, x, mem, ref):
    """Row max within the dot-product bound dk 2^-24 max_j(|q| |k|) / sqrt(dk) of the float64 one and 1 / row sum within relative
    (m + dk max_j(|q| |k|) / sqrt(dk) + 16) 2^-24 (bf16 products are exact in fp32); a fully masked row holds -1e9f exactly and
    1 / m within m 2^-24 relative."""
    B, h, a, m, dk = (mem[n] for n in ("B", "h", "a", "m", "dk"))
    u = 2.0 ** -24
    qh, kh = A._split(x["q"].double(), h).abs(), A._split(x["k"].double(), h).abs()
    aqk = (qh @ kh.transpose(-1, -2)).max(dim=-1).values / math.sqrt(dk)              # [B, h, a]
    full = A._masked(x["mask"], B, h, a, m).all(dim=-1)
    mx, inv = lse[..., 0].double(), lse[..., 1].double()
    live = ~full
    assert bool(((mx - ref.rowmax).abs()[live] <= (dk * u * aqk)[live]).all()), float(((mx - ref.rowmax).abs() / (dk * u * aqk))[live].max())
    rel = (inv - ref.invsum).abs() / ref.invsum
    assert bool((rel[live] <= ((m + dk * aqk + 16) * u)[live]).all()), float((rel / ((m + dk * aqk + 16) * u))[live].max())
    if bool(full.any()):
        assert bool((mx[full] == -1e9).all())
        assert bool(((inv[full] * m - 1.0).abs() <= m * u).all())


def check_member(tag, got, cid, idx, dtype):
    mem = A.CASE_BY_ID[cid]["members"][idx]
    x = A.inputs(cid, idx, dtype)
    ref, bnd = A.reference(cid, idx, dtype)
    bars = A.bars_for(mem, dtype)
    ratios, failures = A.attn_check(got, ref, bnd, dtype, bars)
    for kind in A.KINDS:
        print(f"{tag} member {idx} {kind}: ratio {ratios[kind][0]:.3f} (bar {bars[kind]:.2f}) worst at {ratios[kind][1]}")
    assert not failures, (tag, idx, failures)
    check_lse(got["lse"], x, mem, ref)


GPU_CASES = [(c["id"], dt) for c in A.CASES for dt in c["dtypes"]]


@pytest.mark.parametrize("cid,dtype", GPU_CASES, ids=[f"{c}-{dt}" for c, dt in GPU_CASES])
def test_attention_group(dev, cid, dtype):
    case = A.CASE_BY_ID[cid]
    members = [(mem, A.inputs(cid, i, dtype)) for i, mem in enumerate(case["members"])]
    res = run_group(dev, dtype, members)
    for i, got in enumerate(res):
        check_member(f"{cid} {dtype}", got, cid, i, dtype)


def test_exact_zeros(dev):
    """The structural zeros, stated directly (attn_check asks for them through B == 0): dK / dV rows of a key masked for every query;
    dQ rows and all dK of a fully masked sample, whose dV is not 0."""
    for cid, dtype in (("cross_perq", "bf16"), ("cross_perq", "fp32"), ("dk128", "bf16"), ("valu_dk48_a64", "fp32")):
        mem = A.CASE_BY_ID[cid]["members"][0]
        got = run_group(dev, dtype, [(mem, A.inputs(cid, 0, dtype))])[0]
        B, a, m = mem["B"], mem["a"], mem["m"]
        if mem["mask"] == "perq":
            assert bool((got["dK"][:, m - 1] == 0).all()) and bool((got["dV"][0, m - 1] == 0).all())
            assert bool((got["dQ"][B - 1, a // 2] == 0).all()) and bool((got["dQ"][0] != 0).any())
        else:
            assert bool((got["dQ"][B - 1] == 0).all()) and bool((got["dK"][B - 1] == 0).all())
            assert bool((got["dV"][B - 1] != 0).all())


def test_argument_checks(dev):
    """Every refused call returns MTN_ERR_ARG with a message and writes nothing; a valid call afterwards succeeds."""
    from mtn_amd import lib as L
    lib = L.load()
    fwd, bwd = lib.mtn_attention_fwd_group, lib.mtn_attention_bwd_group

    def group(dtype, B, h, a, m, dk, kv_acc=None):
        mem = A.M(B, h, a, m, dk, "none", kv_acc=kv_acc)
        g = torch.Generator().manual_seed(a * 1000 + m * 10 + dk)
        d = h * dk
        x = dict(q=torch.randn(B, a, d, generator=g), k=torch.randn(B, m, d, generator=g), v=torch.randn(B, m, d, generator=g),
                 d_o=torch.randn(B, a, d, generator=g), mask=None, keep=None, p=0.0)
        return build_group(dev, dtype, [(mem, x)])

    def refused(fn, code, count, arr, state, what):
        rc = fn(code, count, arr, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == MTN_ERR_ARG, (what, rc)
        assert lib.mtn_last_error().decode(), what
        assert all_untouched(state), what

    for dtype in ("fp32", "bf16"):
        code = L.dtype_code(A.TORCH_DTYPE[dtype])
        arr, state = group(dtype, 2, 2, 20, 33, 16)
        d = 32
        for fn in (fwd, bwd):
            refused(fn, code, 0, arr, state, "count 0")
            refused(fn, code, 5, arr, state, "count 5")
            for bad in (6, 132):
                arr[0].dk = bad
                refused(fn, code, 1, arr, state, f"dk {bad}")
            arr[0].dk = 16
            arr[0].ldq = d + 2
            refused(fn, code, 1, arr, state, "ldq = d + 2")
            arr[0].ldq = d
            o = arr[0].o
            arr[0].o = None
            refused(fn, code, 1, arr, state, "NULL o")
            arr[0].o = o
        lse = arr[0].lse
        arr[0].lse = None
        refused(bwd, code, 1, arr, state, "backward with NULL lse")
        arr[0].lse = lse
        arr2, state2 = group(dtype, 1, 2, 40, 8, 16, kv_acc=True)
        arr2[0].kv_acc += 4
        refused(bwd, code, 1, arr2, state2, "kv_acc misaligned by 4 bytes")
        arr3, state3 = group(dtype, 1, 2, 65, 8, 24)
        refused(bwd, code, 1, arr3, state3, "VALU backward with 65 query rows")
        L.check(fwd(code, 1, arr, L.stream_ptr()))
        L.check(bwd(code, 1, arr, L.stream_ptr()))
        torch.cuda.synchronize()
        for o in state[0]["outs"].values():
            o.check("valid call after the refusals")
