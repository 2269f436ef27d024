"""The persistent decode step (csrc/decode.hip) through its C entry point mtn_decode_step, against the float64 step of
tests/decode_refs.py, on stage lists built straight from tensors (no Model).

Short stage lists put one sublayer under direct observation through the granule buffers, which persist after the launch:
  cross  [EMBED, CROSS, OUT, FINAL]            og = the attention output, xg = x after the output projection
  self   [EMBED, SELF_QKV, SELF_ATT, OUT, FINAL]   qg = q | k | v, og, xg, and the cache row (j, pos)
  ffn    [EMBED, FFN1, FFN2, FINAL]            hg = the hidden row, xg
They respect the kernel's hand-off rules (read in csrc/decode.hip): OUT and FFN2 poll the tag of stage si - 1, which is the attention
/ FFN1 before them; SELF_ATT polls the q | k | v granules with the tag of stage si - 1, the SELF_QKV before it; every x reader
(SELF_QKV, FFN1, CROSS, FINAL) walks back to the latest class-0 stage (EMBED, OUT, FFN2), and an x writer adds to ITS columns, which
it kept in LDS from the class-0 stage before — EMBED here.  FINAL sits on the units, of which there are W h >= W.

What the cases of decode_refs.CASES reach:
  cross_*  m in {1, 2, 127, 128, 129, 255, 256, 257, 300, 1024} at dk 32 and 64: the score loop's second to fourth pass (keys >= 256:
           K rows and mask bytes reloaded), the PV loop's loads from memory (u >= 4: keys >= 256 at dk 32, >= 128 at dk 64); masks none /
           ragged per hypothesis / holes on both sides of key 256 / one fully masked hypothesis / mask_stride > m; W in {1, 9, 16}
  self_*   pos in {0, 1, 127, 128, 129, 255, 256, 257, 300} with L = 320 and pos = 1023 with L = 1024, random ancestors
  plan_*   d 512, h 8, one row, the grid cut so that n_mid is 24 / 32 / 48 / 96 / 128: q | k | v slices of 64 / 48 / 32 / 16 / 12 features
           (T = 4, 3, 2, 1, 1) and FFN-1 slices of 52 / 36 / 28 / 12 / 16; d 1024, d_ff 4096, 8 rows: contraction steps beyond the
           prefetched ones
  whole_*  2 layers x (self, cross over 300 keys, cross over 37 keys with a padded mask, FFN), W in {13, 16}, two launches on the same
           buffers with new tokens, the next position and ancestors re-ordered as a beam step does

Every granule buffer starts as all ones (data NaN, a tag no launch produces), out_lp as NaN, and the caches hold NaN wherever the step
must not read (decode_refs).  After a launch: the granules of the last producer of each buffer carry tag
((sync[0] before + 1) << 8) | (stage + 1) and the others are untouched; cache row (j, pos) is the reference k | v and every other cache
element, two guard slots included, is bit-identical; sync[0] advanced by one, sync[1] and sync[2] are 0; NaN in an output fails.

Bounds.  Each output is held to step_ref within MARGIN x CPU_EMUL_<kind> x (the row's largest |ref|), plus one bf16 ulp (2^-8 |ref|) of
the reference element where the output is stored as bf16.  CPU_EMUL_* (tests/decode_refs.py) is the worst distance of step_emul — the
float32 walk with the kernel's bf16 rounding points — from step_ref over these same cases, measured on the CPU and re-measured by
tests/test_decode_refs.py; MARGIN = 4 is what tests/test_row_kernels_gpu.py grants for fast-math intrinsics and another summation
order.  No number here comes from a run of the kernel:
  q | k | v (qg)       4 x 4.73e-3 = 1.89e-2 of the row maximum, + 1 ulp
  attention out (og)   4 x 1.03e-2 = 4.12e-2, + 1 ulp       (a planted key holds >= 0.9 of its row: losing it costs ~0.9 of the head's output)
  FFN hidden (hg)      4 x 5.10e-3 = 2.04e-2, + 1 ulp
  x (xg, fp32)         4 x 3.63e-3 = 1.45e-2
  out_lp               4 x 4.96e-3 = 1.98e-2, + 1 ulp
  cache row (j, pos)   4 x 4.31e-3 = 1.72e-2, + 1 ulp

A poll that times out sets sync[1]: the test that sees it fails, and so does every later test of this module, without launching."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import decode_refs as R

pytestmark = pytest.mark.gpu

MTN_ERR_ARG = 1
_TIMED_OUT = []


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _no_launch_after_a_timeout():
    if _TIMED_OUT:
        pytest.fail(f"a poll of the decode step timed out in {_TIMED_OUT[0]}: nothing more is launched from this module")


def _ones(dev, *shape):
    return torch.full(shape, -1, dtype=torch.int64, device=dev)


class Step:
    """Device state of one case: the stage array, the granule buffers, the caches between two guard slots, the step block."""

    def __init__(self, case, dev, sync0=0):
        from mtn_amd import lib as L
        self.L, self.case, self.dev = L, case, dev
        W, d, dff, Lm = case["W"], case["d"], case["d_ff"], case["L"]
        self.keep = []
        up = lambda t: self.keep.append(t.contiguous().to(dev)) or self.keep[-1]
        self.caches = []
        for c in case["caches"]:                 # slot -1 and slot W are guards
            full = torch.full((W + 2, Lm, 2 * d), float("nan"), dtype=torch.bfloat16, device=dev)
            full[1:W + 1] = c.to(dev)
            self.caches.append(full)
        arr = (L.DecodeStage * len(case["stages"]))()
        for s_, S in zip(arr, case["stages"]):
            s_.kind = S["kind"]
            for name in ("w", "bias", "ln_a", "ln_b", "kv", "mask"):
                if S.get(name) is not None:
                    setattr(s_, name, up(S[name]).data_ptr())
            for name in ("N", "K", "m", "mask_stride", "ln_eps"):
                if name in S:
                    setattr(s_, name, S[name])
            if "cache" in S:
                s_.cache = self.caches[S["cache"]][1:].data_ptr()
        self.stages = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.xg, self.qg, self.og, self.hg = _ones(dev, W, d), _ones(dev, W, 3 * d // 2), _ones(dev, W, d // 2), _ones(dev, W, dff // 2)
        self.out_lp = torch.full((W + 2, d), float("nan"), dtype=torch.bfloat16, device=dev)        # rows 0 and W + 1 are guards
        self.sync = torch.tensor([sync0, 0, 0, 0], dtype=torch.int32, device=dev)
        self.tokens = torch.zeros(W, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.anc = torch.zeros(W, Lm, dtype=torch.int32, device=dev)
        self.lut, self.pe = up(case["lut"]), up(case["pe"])
        a = L.DecodeArgs()
        a.W, a.d, a.h, a.L, a.n_stages, a.d_ff, a.max_m = W, d, case["h"], Lm, len(case["stages"]), dff, case["max_m"]
        a.xg, a.qg, a.og, a.hg, a.out_lp = self.xg.data_ptr(), self.qg.data_ptr(), self.og.data_ptr(), self.hg.data_ptr(), self.out_lp[1:].data_ptr()
        a.tokens, a.lut, a.emb_scale, a.pe = self.tokens.data_ptr(), self.lut.data_ptr(), case["emb_scale"], self.pe.data_ptr()
        a.pos, a.anc, a.sync, a.dbg = self.pos.data_ptr(), self.anc.data_ptr(), self.sync.data_ptr(), None
        self.args = a
        n_cu = int(torch.cuda.get_device_properties(dev).multi_processor_count)
        self.grid = min(256, n_cu) if case["n_mid"] is None or case["n_mid"] >= 128 else W * case["h"] + d // 16 + case["n_mid"]
        assert self.grid <= n_cu, f"this device has {n_cu} compute units, the plan under test needs {self.grid}"

    def set_step(self, stp):
        self.tokens.copy_(stp["tokens"])
        self.pos.fill_(stp["pos"])
        self.anc.copy_(stp["anc"])

    def buffers(self):
        return [self.xg, self.qg, self.og, self.hg, self.out_lp, self.sync] + self.caches

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.clone().view(torch.uint8) for b in self.buffers()]

    def call(self, args=None, grid=None, stages=True):
        rc = self.L.load().mtn_decode_step(C.byref(self.args if args is None else args), self.stages.data_ptr() if stages else None,
                                           self.grid if grid is None else grid, self.L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def launch(self, what):
        rc = self.call()
        assert rc == 0, f"{what}: mtn_decode_step returned {rc}: {self.L.load().mtn_last_error().decode()}"
        sync = self.sync.cpu().tolist()
        if sync[1] != 0:
            _TIMED_OUT.append(what)
            pytest.fail(f"{what}: a poll timed out (sync = {sync}): the step's results are invalid")
        return sync


def _granules(buf):
    """int64 [W, n] -> (data uint32 [W, n], tag uint32 [W, n])"""
    a = buf.cpu().numpy().view(np.uint32).reshape(buf.shape[0], buf.shape[1], 2)
    return a[..., 0], a[..., 1]


def _f32(data):
    return torch.from_numpy(data.copy().view(np.float32)).double()


def _bf16_pairs(data):
    lo, hi = (data << 16).view(np.float32), (data & np.uint32(0xffff0000)).view(np.float32)
    return torch.from_numpy(np.stack([lo, hi], axis=-1).reshape(data.shape[0], -1)).double()


def hold(what, kind, got, ref, bf16_out):
    """got within the bound of ref, elementwise; prints the worst |got - ref| / bound before it asserts."""
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements are not finite"
    err, bnd = (got - ref).abs(), R.bound(kind, ref, bf16_out)
    ratio = err / bnd
    i = int(ratio.argmax())
    r, c = divmod(i, ref.shape[1])
    print(f"{what}: worst |got - ref| / bound = {float(ratio.max()):.3f} at row {r} column {c} (got {float(got[r, c]):.6g}, ref {float(ref[r, c]):.6g}, "
          f"bound {float(bnd[r, c]):.3g}; row max |ref| {float(ref[r].abs().max()):.4g})")
    assert float(ratio.max()) <= 1.0, f"{what}: |got - ref| = {float(err[r, c]):.4g} > bound {float(bnd[r, c]):.4g} at row {r} column {c}"


def check_step(S, ref, gen, before, what):
    """Everything a launch leaves behind, against step_ref's result `ref`.  before: S.snapshot() taken in front of the launch."""
    case = S.case
    W, d = case["W"], case["d"]
    kinds = [st["kind"] for st in case["stages"]]
    last = lambda ks: max([i for i, k in enumerate(kinds) if k in ks], default=None)
    for name, buf, ks, key, kind, dec in (("xg", S.xg, R.X_WRITERS, "x", "X", _f32), ("qg", S.qg, (R.SELF_QKV,), "qkv", "QKV", _bf16_pairs),
                                          ("og", S.og, (R.SELF_ATT, R.CROSS), "att", "ATT", _bf16_pairs), ("hg", S.hg, (R.FFN1,), "hid", "HID", _bf16_pairs)):
        data, tag = _granules(buf)
        si = last(ks)
        if si is None:
            assert bool((data == 0xffffffff).all() and (tag == 0xffffffff).all()), f"{what}: {name} has no producer in this list and was written"
            continue
        want = (gen << 8) | (si + 1)
        assert bool((tag == want).all()), f"{what}: {int((tag != want).sum())} granules of {name} do not carry tag {want:#x} (e.g. {int(tag[tag != want][0]):#x})"
        hold(f"{what} {name} (stage {si})", kind, dec(data), ref[key][si], name != "xg")
    out = S.out_lp.cpu()
    assert bool(torch.isnan(out[0]).all() and torch.isnan(out[W + 1]).all()), f"{what}: a guard row of out_lp was written"
    hold(f"{what} out_lp", "OUT_LP", out[1:W + 1].double(), ref["out_lp"], True)
    pos = int(S.pos.cpu())
    for ci, full in enumerate(S.caches):
        now, was = full.cpu(), before[5 + 1 + ci].view(torch.bfloat16).view(full.shape).cpu()
        hold(f"{what} cache {ci} row (j, {pos})", "CACHE", now[1:W + 1, pos].double(), ref["cache_rows"][ci], True)
        same = now.view(torch.int16) == was.view(torch.int16)
        same[1:W + 1, pos] = True
        assert bool(same.all()), f"{what}: {int((~same).sum())} elements of cache {ci} outside row (j, {pos}) changed"


def run_case(cid, dev, sync0=0):
    case = R.build_case(cid)
    refs, _ = R.run_case(case)
    S = Step(case, dev, sync0)
    for n, (stp, ref) in enumerate(zip(case["steps"], refs)):
        S.set_step(stp)
        before = S.snapshot()
        sync = S.launch(f"{cid} launch {n}")
        assert sync[:3] == [sync0 + n + 1, 0, 0], f"{cid} launch {n}: sync = {sync}, expected generation {sync0 + n + 1} and no time-out"
        check_step(S, ref, sync0 + n + 1, before, f"{cid} launch {n}")
    return S


def _ids(prefix):
    return [c["id"] for c in R.CASES if c["id"].startswith(prefix)]


@pytest.mark.parametrize("cid", _ids("cross_"))
def test_cross_attention(cid, dev):
    run_case(cid, dev)


@pytest.mark.parametrize("cid", _ids("self_"))
def test_self_attention(cid, dev):
    run_case(cid, dev, sync0=2)


@pytest.mark.parametrize("cid", _ids("ffn_"))
def test_feed_forward(cid, dev):
    run_case(cid, dev)


@pytest.mark.parametrize("cid", _ids("plan_"))
def test_slice_plans(cid, dev):
    run_case(cid, dev)


@pytest.mark.parametrize("cid", _ids("whole_"))
def test_whole_step_twice_on_the_same_buffers(cid, dev):
    """Nothing is re-zeroed between the launches: the second one's outputs match its own reference, so no granule of the first
    launch was taken for one of the second."""
    run_case(cid, dev, sync0=40)


REFUSALS = [
    ("W17", dict(W=17)), ("d384", dict(d=384, d_ff=768)), ("head16", dict(h=8)), ("L1025", dict(L=1025)), ("max_m0", dict(max_m=0)),
    ("max_m1025", dict(max_m=1025)), ("dff_below_d", dict(d_ff=96)), ("dff_mod32", dict(d_ff=400)), ("dff4128", dict(d_ff=4128)),
    ("Wd_over_8192", dict(W=16, d=1024, h=16, d_ff=1024)), ("W16_dff4096", dict(W=16, d=512, h=8, d_ff=4096)),
    ("n_stages161", dict(n_stages=161)), ("grid_small", dict(grid=9 * 4 + 128 // 16 + 15)), ("null_xg", dict(xg=None)),
    ("null_out_lp", dict(out_lp=None)), ("null_sync", dict(sync=None)), ("null_stages", dict(stages=False)),
]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, change, dev):
    """Host-side argument checks: an error code, nothing launched, every buffer and sync untouched."""
    S = Step(R.build_case("ffn_d128_w9"), dev, sync0=5)
    S.set_step(S.case["steps"][0])
    a = type(S.args).from_buffer_copy(S.args)
    change = dict(change)
    grid, stages = change.pop("grid", None), change.pop("stages", True)
    for k, v in change.items():
        setattr(a, k, v)
    before = S.snapshot()
    rc = S.call(a, grid, stages)
    assert rc == MTN_ERR_ARG, f"{name}: mtn_decode_step returned {rc}"
    assert all(torch.equal(x, y) for x, y in zip(before, S.snapshot())), f"{name}: a refused call wrote to a buffer"
    assert S.launch(f"{name}: the unchanged arguments")[:3] == [6, 0, 0]
