"""The large-batch token-axis kernels at every matmul precision through the C-ABI.  One body each for the forward / input-gradient
kernel and the weight gradient (csrc/token_linear_common.h: token_linear_body, token_dw_body), entered with the fp32 products
(csrc/token_linear.hip: token_linear_kernel, token_dw_kernel — HIGHEST, what every default run uses) or the bf16 products
(csrc/token_linear_bf16.hip: token_linear_bf16_kernel at nasrec_gemm_desc_t.precision = MEDIUM, token_dw_bf16_kernel at HIGH / MEDIUM),
held to the arithmetic contract of DESIGN.md "Matmul precision":

    HIGHEST |C - sum_k a b| <= (Kt + 8) u S,                   S = sum_k |a| |b|
    MEDIUM  |C - sum_k â b̂| <= (Kt + 8) u S,                  S = sum_k |â| |b̂|
    HIGH    |C - sum_k a b| <= (2^-16 + (3 Kt + 8) u) S,       S = sum_k |a| |b|

(HIGHEST: an fp32 FMA chain of Kt terms with unit roundoff 2^-24 stays within Kt 2^-23 S; the + 8 is the allowance for the epilogue
and the second pass, as at MEDIUM)

with â = bf16(a) (round to nearest even), u = 2^-23, Kt the total k of the product, everything on the right in fp64; an fp32 term t
the epilogue adds (bias, the accumulation target) widens the bound by 8 u |t|.  Exact-integer products (|W| <= 2, |x| <= 3, integer
bias; dW: |dz|, |x| <= 2, every sum < 2^24) need no tolerance and catch any fragment, k-permutation, padding, tail or row-block error.

Shapes: B = 1024 (the routes' minimum) and 1031 (a ragged last workgroup); M over every row-block count and its edges; K segments
with ragged k-steps and ragged 32-k chunks, [32] and [33] (a chunk exactly full / one k over), and the > 64 KB LDS image at M = 64.
Weight gradient: 45 x 73 (3 x 5 blocks of 16) and 72 x 73 (5 x 5 blocks: the instantiation at the register limit).

The forward / input-gradient kernel has no HIGH body: measured, it was slower than the fp32 kernel on one of the launches of
DESIGN.md's table, so HIGH keeps the fp32 products there and its cases left with the kernel (further cases of the fp32 kernels, at a
flat tolerance, are in tests/test_gemm_fast_gpu.py); test_high_keeps_the_fp32_body_of_the_forward_kernel pins that."""
import ctypes as C

import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import plan as P

pytestmark = pytest.mark.gpu

PRECISIONS = [L.PRECISION_HIGHEST, L.PRECISION_HIGH, L.PRECISION_MEDIUM]  # token_dw_kernel; token_dw_bf16_kernel
LINEAR_PRECISIONS = [L.PRECISION_HIGHEST, L.PRECISION_MEDIUM]             # token_linear_kernel; token_linear_bf16_kernel
U = 2.0 ** -23
K3 = [26, 72, 9]
KBIG = [72, 72, 72, 72, 21]  # at M = 64: 99 KB of staged weights (> the default dynamic-LDS limit)


def _coef(prec, Kt):
    return 2.0 ** -16 + (3 * Kt + 8) * U if prec == L.PRECISION_HIGH else (Kt + 8) * U


def _seen(prec, t):
    """the operand as the product sees it, in fp64: bf16-rounded for MEDIUM, itself for HIGH and HIGHEST"""
    return t.bfloat16().double() if prec == L.PRECISION_MEDIUM else t.double()


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).contiguous()


def _ints(lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, device="cuda").float().contiguous()


def _launch(lib, d):
    L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()


def _within(got, want, bound, what):
    """elementwise |got - want| <= bound (fp64); prints the figure before it asserts"""
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max err %.3e, max err / bound %.3f" % (what, float(err.max()), ratio))
    assert torch.isfinite(got).all(), what
    assert bool((err <= bound).all()), "%s: max err / bound = %.3f" % (what, ratio)


def _tok_desc(am, segs, zmode, prec, **kw):
    d = L.GemmDesc()
    d.kind = L.OP_GEMM
    d.amode, d.bmode, d.cmode, d.nseg, d.zmode = am, L.AM_TOKR, L.CM_TOKJ, len(segs), zmode
    d.dims_in_use = kw.get("dims", -1)
    d.act = kw.get("act", 0)
    d.beta = kw.get("beta", 0)
    d.bias_on_rows, d.mask_on_rows = 1, 1
    d.splitk = 1
    for k in ("bias", "save_z"):
        if kw.get(k) is not None:
            setattr(d, k, kw[k].data_ptr())
    for q, sd in enumerate(segs):
        for k, v in sd.items():
            setattr(d.seg[q], k, v)
        d.seg[q].Mvalid = sd["M"]
    d.precision = prec
    name = "token_linear_bf16_kernel" if prec == L.PRECISION_MEDIUM else "token_linear_kernel"
    assert P.gemm_kernel_name(d) == name, "the case must be sized for the token-axis kernel"
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# forward: out[b, n', e] = act(sum_n W[n', n] x[b, n, e] + bias[n']); inputs and outputs are token sub-ranges of larger slabs
# ---------------------------------------------------------------------------------------------------------------------------------
def _forward(lib, prec, B, nout, Ks, act, dims, beta, integers, save_z=False):
    """-> out, out0, z (or None), W, bias, x (the K-concatenated input, [B, sum Ks, 16]), and a re-launch closure"""
    Ntot = sum(Ks)
    if integers:
        W, bias = _ints(-2, 2, nout, Ntot), _ints(-3, 3, nout)
        slabs = [_ints(-3, 3, B, k + 5, 16) for k in Ks]
        out = _ints(-3, 3, B, nout + 3, 16)
    else:
        W, bias = _rand(nout, Ntot, scale=0.2), _rand(nout)
        slabs = [_rand(B, k + 5, 16) for k in Ks]  # the segment is rows 2 .. 2+k of a larger slab
        out = _rand(B, nout + 3, 16)
    out0 = out.clone()
    z = torch.zeros_like(out) if save_z else None
    segs, koff = [], 0
    for slab, k in zip(slabs, Ks):
        segs.append(dict(A=W.data_ptr() + 4 * koff, B=slab.data_ptr() + 4 * 2 * 16, C=out.data_ptr() + 4 * 16, M=nout, N=B * 16, K=k, lda=Ntot,
                         ldb=slab.stride(0), ldc=out.stride(0)))
        koff += k
    d = _tok_desc(L.AM_KC, segs, 0, prec, bias=bias, act=act, dims=dims, beta=beta)
    if save_z:
        d.save_z = z.data_ptr() + 4 * 16
    _launch(lib, d)
    x = torch.cat([slab[:, 2:2 + k] for slab, k in zip(slabs, Ks)], 1)

    def again():
        out.copy_(out0)
        _launch(lib, d)
        return out.clone()
    return out, out0, z, W, bias, x, again, (slabs, segs)


def _forward_reference(prec, W, bias, x):
    """-> (pre-activation of the product as the contract states it, its bound), both fp64"""
    Ws, xs = _seen(prec, W), _seen(prec, x)
    zz = torch.einsum("on,bne->boe", Ws, xs) + bias.double()[None, :, None]
    S = torch.einsum("on,bne->boe", Ws.abs(), xs.abs())
    return zz, _coef(prec, W.shape[1]) * S + 8 * U * bias.double().abs()[None, :, None]


# every row-block count and its edges on the ragged three-segment K; a chunk exactly full and one k over; the large LDS image
FWD_SHAPES = [(1024, 7, K3), (1031, 16, K3), (1024, 17, K3), (1031, 48, K3), (1024, 49, K3), (1031, 80, K3),
              (1024, 45, [32]), (1031, 45, [33]), (1031, 64, KBIG)]


@pytest.mark.parametrize("prec", LINEAR_PRECISIONS)
@pytest.mark.parametrize("B,nout,Ks", FWD_SHAPES)
def test_forward_integer_products_are_exact(lib, prec, B, nout, Ks):
    torch.manual_seed(21)
    out, out0, _, W, bias, x, _, _keep = _forward(lib, prec, B, nout, Ks, L.ACT_RELU, -1, 0, integers=True)
    want = (torch.einsum("on,bne->boe", W.double(), x.double()) + bias.double()[None, :, None]).clamp_min(0)
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(out[:, 1:1 + nout].double(), want), "max diff %g" % float((out[:, 1:1 + nout].double() - want).abs().max())
    assert torch.equal(out[:, 0], out0[:, 0]) and torch.equal(out[:, 1 + nout:], out0[:, 1 + nout:]), "rows outside the target were written"


@pytest.mark.parametrize("prec", LINEAR_PRECISIONS)
@pytest.mark.parametrize("B,nout,Ks", FWD_SHAPES)
def test_forward_within_the_derived_bound(lib, prec, B, nout, Ks):
    torch.manual_seed(22)
    out, out0, _, W, bias, x, _, _keep = _forward(lib, prec, B, nout, Ks, L.ACT_NONE, -1, 0, integers=False)
    want, bound = _forward_reference(prec, W, bias, x)
    _within(out[:, 1:1 + nout], want, bound, "forward M=%d K=%s prec=%d" % (nout, Ks, prec))
    assert torch.equal(out[:, 0], out0[:, 0]) and torch.equal(out[:, 1 + nout:], out0[:, 1 + nout:]), "rows outside the target were written"


@pytest.mark.parametrize("prec", LINEAR_PRECISIONS)
@pytest.mark.parametrize("integers", [False, True])
def test_forward_prefix_mask_relu_and_accumulation(lib, prec, integers):
    """dims 30 of 45 rows live, ReLU, beta = 1: the masked rows keep exactly what the target held"""
    torch.manual_seed(23)
    B, nout, dims = 1031, 45, 30
    out, out0, _, W, bias, x, _, _keep = _forward(lib, prec, B, nout, K3, L.ACT_RELU, dims, 1, integers=integers)
    if integers:
        want = (torch.einsum("on,bne->boe", W.double(), x.double()) + bias.double()[None, :, None]).clamp_min(0)
        want[:, dims:] = 0
        assert torch.equal(out[:, 1:1 + nout].double(), want + out0[:, 1:1 + nout].double())
    else:
        zz, bound = _forward_reference(prec, W, bias, x)
        want = zz.clamp_min(0)  # (ReLU is 1-Lipschitz: the bound of z holds for it)
        want[:, dims:] = 0
        t = out0[:, 1:1 + nout].double()
        _within(out[:, 1:1 + nout], want + t, bound + 8 * U * t.abs(), "forward mask+relu+beta prec=%d" % prec)
    assert torch.equal(out[:, 1 + dims:1 + nout], out0[:, 1 + dims:1 + nout]), "a masked row adds exactly zero"
    assert torch.equal(out[:, 0], out0[:, 0]) and torch.equal(out[:, 1 + nout:], out0[:, 1 + nout:]), "rows outside the target were written"


@pytest.mark.parametrize("prec", LINEAR_PRECISIONS)
def test_forward_silu_with_saved_preactivation(lib, prec):
    torch.manual_seed(24)
    B, nout = 1024, 80
    out, out0, z, W, bias, x, _, _keep = _forward(lib, prec, B, nout, K3, L.ACT_SILU, -1, 1, integers=False, save_z=True)
    zz, bound = _forward_reference(prec, W, bias, x)
    _within(z[:, 1:1 + nout], zz, bound, "save_z prec=%d" % prec)
    t = out0[:, 1:1 + nout].double()
    want = zz * torch.sigmoid(zz) + t
    # |SiLU'| <= 1.1 carries the bound of z to the output; the device's own sigmoid is held as tests/test_gemm_fast_gpu.py::_close holds it
    tol = 2e-5 * max(1.0, float(want.abs().max()))
    _within(out[:, 1:1 + nout], want, 1.1 * bound + 8 * U * t.abs() + tol, "silu output prec=%d" % prec)
    assert torch.equal(z[:, 0], torch.zeros_like(z[:, 0])) and torch.equal(z[:, 1 + nout:], torch.zeros_like(z[:, 1 + nout:]))
    assert torch.equal(out[:, 0], out0[:, 0]) and torch.equal(out[:, 1 + nout:], out0[:, 1 + nout:]), "rows outside the target were written"


def test_medium_rounds_its_operands_to_nearest_even(lib):
    """randn data, K = 107: MEDIUM is held to its bound against the product of the ROUNDED operands.  The test's own discrimination is
    asserted first: the fp32 product of the unrounded operands, and the product of truncated operands, both lie outside that bound."""
    torch.manual_seed(25)
    B, nout = 1024, 45
    out, _, _, W, bias, x, _, _keep = _forward(lib, L.PRECISION_MEDIUM, B, nout, K3, L.ACT_NONE, -1, 0, integers=False)
    want, bound = _forward_reference(L.PRECISION_MEDIUM, W, bias, x)
    exact = torch.einsum("on,bne->boe", W.double(), x.double()) + bias.double()[None, :, None]

    def trunc(t):
        return (t.view(torch.int32) & -65536).view(torch.float32).double()
    chopped = torch.einsum("on,bne->boe", trunc(W), trunc(x)) + bias.double()[None, :, None]
    for name, other in (("unrounded", exact), ("truncated", chopped)):
        outside = float(((other - want).abs() > bound).double().mean())
        print("%s product: %.1f %% of the elements outside the MEDIUM bound" % (name, 100 * outside))
        assert outside > 0.5, "the bound must separate the rounded-operand product from the %s one" % name
    _within(out[:, 1:1 + nout], want, bound, "medium vs rounded operands")


def test_high_keeps_the_fp32_body_of_the_forward_kernel(lib):
    """HIGH is a permission the forward / input-gradient kernel does not take up: same kernel, same bits as HIGHEST"""
    torch.manual_seed(26)
    B, nout = 1024, 45
    W, bias, x, out = _rand(nout, 107, scale=0.2), _rand(nout), _rand(B, 107, 16), {}
    for prec in (L.PRECISION_HIGHEST, L.PRECISION_HIGH):
        out[prec] = torch.zeros(B, nout, 16, device="cuda")
        d = L.GemmDesc()
        d.kind, d.amode, d.bmode, d.cmode, d.nseg, d.dims_in_use, d.splitk = L.OP_GEMM, L.AM_KC, L.AM_TOKR, L.CM_TOKJ, 1, -1, 1
        d.bias, d.bias_on_rows, d.mask_on_rows, d.precision = bias.data_ptr(), 1, 1, prec
        for k, v in dict(A=W.data_ptr(), B=x.data_ptr(), C=out[prec].data_ptr(), M=nout, N=B * 16, K=107, lda=107, ldb=107 * 16, ldc=nout * 16,
                         Mvalid=nout).items():
            setattr(d.seg[0], k, v)
        assert P.gemm_kernel_name(d) == "token_linear_kernel"
        _launch(lib, d)
    assert torch.equal(out[L.PRECISION_HIGHEST], out[L.PRECISION_HIGH])


@pytest.mark.parametrize("prec", LINEAR_PRECISIONS)
def test_forward_is_deterministic(lib, prec):
    torch.manual_seed(27)
    out, _, _, _, _, _, again, _keep = _forward(lib, prec, 1031, 64, KBIG, L.ACT_NONE, -1, 0, integers=False)
    first = out.clone()
    assert torch.equal(first, again())


# ---------------------------------------------------------------------------------------------------------------------------------
# input gradient: dx_s[b, n, e] = sum_n' W[n', koff_s + n] dz[b, n', e], a batch of independent problems
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", LINEAR_PRECISIONS)
@pytest.mark.parametrize("integers", [False, True])
def test_input_gradient_batch(lib, prec, integers):
    """the prefix mask as a shorter K (50 of 64), accumulation into a gradient that already holds a contribution"""
    torch.manual_seed(28)
    B, nout, kd, Ks = 1024, 64, 50, [72, 72, 66]
    Ntot = sum(Ks)
    if integers:
        W, dz = _ints(-2, 2, nout, Ntot), _ints(-3, 3, B, nout, 16)
    else:
        W, dz = _rand(nout, Ntot, scale=0.2), _rand(B, nout, 16)
    segs, checks, koff = [], [], 0
    for q, k in enumerate(Ks):
        dx = _ints(-3, 3, B, k + 2, 16) if integers else _rand(B, k + 2, 16)
        dx0 = dx.clone()
        acc = q == 1
        segs.append(dict(A=W.data_ptr() + 4 * koff, B=dz.data_ptr(), C=dx.data_ptr(), M=k, N=B * 16, K=kd, lda=Ntot, ldb=dz.stride(0),
                         ldc=dx.stride(0), accumulate=int(acc)))
        Ws, gs = _seen(prec, W[:kd, koff:koff + k]), _seen(prec, dz[:, :kd])
        want = torch.einsum("on,boe->bne", Ws, gs)
        t = dx0[:, :k].double() if acc else torch.zeros_like(want)
        bound = _coef(prec, kd) * torch.einsum("on,boe->bne", Ws.abs(), gs.abs()) + 8 * U * t.abs()
        checks.append((dx, want + t, bound, dx0, k))
        koff += k
    _launch(lib, _tok_desc(L.AM_RC, segs, 1, prec))
    for q, (dx, want, bound, dx0, k) in enumerate(checks):
        if integers:
            assert torch.equal(dx[:, :k].double(), want)
        else:
            _within(dx[:, :k], want, bound, "input gradient problem %d prec=%d" % (q, prec))
        assert torch.equal(dx[:, k:], dx0[:, k:])


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradient: dW[n', n] = sum_{b,e} dz[b, n', e] x[b, n, e], S workgroups per problem -> S slabs -> the fixed-order second pass
# ---------------------------------------------------------------------------------------------------------------------------------
def _dw(lib, prec, B, S, nout, kd, widths, integers):
    Ntot = sum(widths)
    if integers:
        dz, dW = _ints(-2, 2, B, nout + 2, 16), _ints(-3, 3, nout, Ntot)
    else:
        dz, dW = _rand(B, nout + 2, 16, scale=0.3), _rand(nout, Ntot)
    db = torch.zeros(nout, device="cuda")
    dW0 = dW.clone()
    g = _seen(prec, dz[:, 1:1 + nout]).clone()
    g[:, kd:] = 0  # Mvalid: the rows beyond the prefix are zero
    segs, checks, slabs, koff = [], [], [], 0
    for q, w in enumerate(widths):
        slab = _ints(-2, 2, B, w + 4, 16) if integers else _rand(B, w + 4, 16)
        slabs.append(slab)
        ones, acc = int(q == 0), int(q == len(widths) - 1)
        segs.append(dict(A=dz.data_ptr() + 4 * 16, B=slab.data_ptr() + 4 * 3 * 16, C=dW.data_ptr() + 4 * koff, M=nout, N=w + ones, K=B * 16,
                         lda=dz.stride(0), ldb=slab.stride(0), ldc=Ntot, Mvalid=kd, accumulate=acc, ones_col=ones, rowsum=db.data_ptr() if ones else None))
        xs = _seen(prec, slab[:, 3:3 + w])
        want = torch.einsum("boe,bne->on", g, xs)
        t = dW0[:, koff:koff + w].double() if acc else torch.zeros_like(want)
        bound = _coef(prec, B * 16) * torch.einsum("boe,bne->on", g.abs(), xs.abs()) + 8 * U * t.abs()
        checks.append((koff, w, want + t, bound))
        koff += w
    d = L.GemmDesc()
    d.kind = L.OP_GEMM
    d.amode, d.bmode, d.cmode, d.nseg, d.zmode, d.dims_in_use = L.AM_TOKK, L.AM_TOKK, L.CM_PLAIN, len(segs), 1, -1
    for q, sd in enumerate(segs):
        for k, v in sd.items():
            setattr(d.seg[q], k, v)
    ws = torch.full((S * nout * (max(widths) + 1) * len(segs),), float("nan"), device="cuda")
    d.splitk, d.workspace = S, ws.data_ptr()
    d.precision = prec
    name = "token_dw_kernel" if prec == L.PRECISION_HIGHEST else "token_dw_bf16_kernel"
    assert P.gemm_route(d)[0] == L.GEMM_ROUTE_TOKEN_DW and P.gemm_kernel_name(d) == name
    _launch(lib, d)

    def again():
        dW.copy_(dW0)
        db.zero_()
        ws.fill_(float("nan"))
        _launch(lib, d)
        return dW.clone(), db.clone()
    return dW, db, checks, g.sum((0, 2)), _coef(prec, B * 16) * g.abs().sum((0, 2)), again, (dz, slabs)


# (B, S, nout, kd, widths).  45 x (72 + ones column): 3 x 5 blocks — the smallest launch the family takes, then the shapes of the fp32
# test; 72 x (72 + ones column): 5 x 5 blocks (integer sums <= 1024 * 16 * 4)
DW45 = (45, 40, [72, 26, 9, 72])
DW_SHAPES = [pytest.param(1024, 4, *DW45, id="1024-4"), pytest.param(1280, 8, *DW45, id="1280-8"), pytest.param(1280, 37, *DW45, id="1280-37"),
             pytest.param(1024, 4, 72, 64, [72, 72], id="1024-4-5x5")]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("B,S,nout,kd,widths", DW_SHAPES)
def test_weight_gradient_integer_products_are_exact(lib, prec, B, S, nout, kd, widths):
    torch.manual_seed(29)
    dW, db, checks, db_want, _, _, _keep = _dw(lib, prec, B, S, nout, kd, widths, integers=True)
    for koff, w, want, _ in checks:
        assert float(want.abs().max()) < 2 ** 24
        assert torch.equal(dW[:, koff:koff + w].double(), want), "columns %d..%d" % (koff, koff + w)
    assert torch.equal(db.double(), db_want)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("B,S,nout,kd,widths", DW_SHAPES)
def test_weight_gradient_within_the_derived_bound(lib, prec, B, S, nout, kd, widths):
    torch.manual_seed(30)
    dW, db, checks, db_want, db_bound, again, _keep = _dw(lib, prec, B, S, nout, kd, widths, integers=False)
    for koff, w, want, bound in checks:
        _within(dW[:, koff:koff + w], want, bound, "dW columns %d..%d B=%d S=%d prec=%d" % (koff, koff + w, B, S, prec))
    _within(db, db_want, db_bound, "bias gradient (ones column) B=%d S=%d prec=%d" % (B, S, prec))
    first = (dW.clone(), db.clone())
    second = again()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), "two launches of one descriptor differ"
