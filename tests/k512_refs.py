"""Host references for the direct tests of the K = 512 projection kernels (csrc/gemm_k512.hip, csrc/gemm_k512_tile.h:
y = x W^T + b, bf16 in, bf16 out; tests/test_k512_kernel_gpu.py); validated without a GPU by tests/test_k512_refs.py.  Plain helpers,
no fixtures, no GPU imports.

make_case   one problem (M, N, lda, ldb, ldc, bias on / off): bf16 x [M, lda] and W [N, ldb] whose rows carry the scale ramps
            linspace(0.5, 1.5) (a row or column swap is an O(1) error), whose columns >= 512 hold bf16 NaN (a kernel that reads past
            K is visibly wrong), and a float32 bias drawn from N(0, 1), or none.
ref64       x[:, :512].double() @ W[:, :512].double().T + bias.double().
bound64     the DERIVED elementwise bound on |out - ref|:

                (1 + 2^-8) * [ 2^-8 |ref| + (K + 1) 2^-23 (sum_k |x_k| |w_k| + |bias|) ]

            Products of two bf16 values (8-bit significands) are exact in float32.  The float32 result s (K products and the bias, K + 1
            additions in any order and grouping, each addition within 2^-23 of its own result — the unit of a truncating adder, twice
            that of a rounding one — and no partial result above sum |x_k| |w_k| + |bias|) satisfies, to first order,
            |s - ref| <= E = (K + 1) 2^-23 (sum |x_k| |w_k| + |bias|).  One round-to-nearest bf16 rounding (fh_pack2 rounds to nearest
            even; 8 significant bits) moves s by at most half a unit in the last place, 2^-8 |s|, and |s| <= |ref| + E:
            |out - ref| <= 2^-8 (|ref| + E) + E <= (1 + 2^-8) (2^-8 |ref| + E).  No margin factor on top.
emulate     the float32 arithmetic of the kernels, in their order: one accumulator per output element, sixteen steps of 32 products
            in ascending k (one MFMA each), the bias added in float32, one rounding to bf16.  Its switches are the MUTATIONS that
            tests/test_k512_refs.py requires the bound to reject.
violations  elements of an output outside the bound (or not finite), and the worst |out - ref| / bound.

CASES       the problem lists of the stand-alone wide-tile launches, QUEUE_SHAPE the one-tile problem of the queue tests, FORMS the
            problem set just above the 512-tile minimum of mtn_gemm; shared with the GPU file."""
from types import SimpleNamespace

import torch

K = 512
STEP = 32                              # contraction depth of one MFMA (16 x 16 x 32)
BF16 = torch.bfloat16

# (M, N, lda, ldb, ldc, bias).  ldc = 2 N: the output is the SECOND column block of a [rows, 2 N] buffer.
# One list = one mtn_kv_project call with n_now = count - 1: the last problem waits for mtn_riders_flush.
CASES = {
    # one row tile, partial and full: M = 1, 16, 127, 128; one and two column tiles
    "one_row_tile": [(1, 256, 512, 512, 256, True), (16, 256, 520, 528, 264, False), (127, 512, 1024, 512, 512, True),
                     (128, 256, 512, 528, 512, True), (128, 512, 520, 512, 520, False)],
    # two and three row tiles (the last one of 1 row, of 1 row, full), up to three column tiles: tn = t / tiles_m with tiles_m = 2, 3
    "row_tiles": [(129, 512, 520, 528, 1024, True), (257, 768, 512, 512, 768, False), (384, 512, 1024, 528, 520, True),
                  (257, 256, 1024, 512, 256, True)],
    # three full row tiles x three column tiles behind a one-tile problem, everything padded, null bias; the waiting problem has two row tiles
    "nine_tiles": [(16, 256, 512, 512, 256, True), (384, 768, 520, 528, 776, False), (129, 768, 1024, 528, 1536, True)],
}
QUEUE_SHAPE = (8, 256, 512, 512, 256, True)
# 128 x 128 tiles: 32*8 + 8*6 + 1*2 + 16*8 + 13*6 + 1*2 = 514, wide tiles 257.  mtn_gemm hands a launch to these kernels from 512 on; with
# exactly 512 the wide form would have 256 workgroups, the persistent form's fixed grid, and the census (one name for the three forms,
# told apart by their workgroup counts) could not say which of the two ran: the second problem below 8 rows makes the counts 257, 514, 256.
# M = 1000 is no multiple of 64 (the persistent form's row unit); M = 5 and 3 leave most XCDs without a unit of those problems; N = 1024,
# 768, 256 make a persistent workgroup change its column tile between units.
FORMS = [(4096, 1024, 512, 512, 1024, True), (1000, 768, 640, 528, 768, True), (5, 256, 512, 512, 256, True),
         (2048, 1024, 512, 512, 1032, False), (1664, 768, 512, 512, 768, True), (3, 256, 520, 512, 264, False)]
PERSISTENT_GRID = 256                  # workgroups of the persistent form, whatever the problems


def tiles(shapes, tile_n):
    """Workgroups of a tile-per-workgroup launch over `shapes`: 128-row tiles x tile_n-column tiles."""
    return sum(((s[0] + 127) // 128) * ((s[1] + tile_n - 1) // tile_n) for s in shapes)


def make_case(shape, seed):
    M, N, lda, ldb, ldc, has_bias = shape
    assert lda >= K and ldb >= K and N % 8 == 0
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.full((M, lda), float("nan"), dtype=BF16)
    w = torch.full((N, ldb), float("nan"), dtype=BF16)
    x[:, :K] = (torch.randn(M, K, generator=g) * torch.linspace(0.5, 1.5, M).unsqueeze(1)).to(BF16)
    w[:, :K] = (torch.randn(N, K, generator=g) * (K ** -0.5) * torch.linspace(0.5, 1.5, N).unsqueeze(1)).to(BF16)
    bias = torch.randn(N, generator=g) if has_bias else None
    return SimpleNamespace(shape=shape, M=M, N=N, lda=lda, ldb=ldb, ldc=ldc, x=x, w=w, bias=bias)


def ref64(c):
    ref = c.x[:, :K].double() @ c.w[:, :K].double().t()
    return ref if c.bias is None else ref + c.bias.double()


def bound64(c, ref):
    mag = c.x[:, :K].double().abs() @ c.w[:, :K].double().abs().t()
    if c.bias is not None:
        mag = mag + c.bias.double().abs()
    return (1 + 2.0 ** -8) * (2.0 ** -8 * ref.abs() + (K + 1) * 2.0 ** -23 * mag)


def with_refs(c):
    c.ref = ref64(c)
    c.bound = bound64(c, c.ref)
    return c


def emulate(c, drop_last_step=False, drop_product=None, drop_bias=False, truncate=False):
    """-> bf16 [M, N].  drop_product = k: the product x_k w_k is missing from every output element."""
    x, w = c.x[:, :K].float(), c.w[:, :K].float()
    if drop_product is not None:
        x = x.clone()
        x[:, drop_product] = 0.0
    acc = torch.zeros(c.M, c.N, dtype=torch.float32)
    for s in range(K // STEP - (1 if drop_last_step else 0)):
        acc = acc + x[:, s * STEP:(s + 1) * STEP] @ w[:, s * STEP:(s + 1) * STEP].t()
    if c.bias is not None and not drop_bias:
        acc = acc + c.bias
    if truncate:
        return (acc.view(torch.int32) & -65536).view(torch.float32).to(BF16)       # exact: the low 16 bits are zero
    return acc.to(BF16)                                                            # round to nearest even


def violations(out, ref, bound):
    """-> (elements outside the bound or not finite, worst |out - ref| / bound over the finite ones)."""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = (out - ref).abs()
    bad = ~torch.isfinite(out) | (err > bound)
    ratio = torch.where(torch.isfinite(out), err / bound, torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max())


def assert_within(out, c, what):
    n, worst = violations(out, c.ref, c.bound)
    assert n == 0, f"{what} {c.shape}: {n} of {c.ref.numel()} elements outside the bound, worst |out - ref| / bound = {worst:.3g}"
    return worst
