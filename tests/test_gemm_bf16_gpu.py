"""The bf16 body of the throughput-regime GEMM (csrc/gemm_fast_bf16.hip: nasrec_gemm_desc_t.precision = HIGH / MEDIUM) through the
C-ABI, held to the arithmetic contract of DESIGN.md "Matmul precision":

    MEDIUM  |C_ij - sum_k â_ik b̂_jk| <= (Kt + 8) u S_ij,                  S_ij = sum_k |â_ik| |b̂_jk|
    HIGH    |C_ij - sum_k a_ik b_jk| <= (2^-16 + (3 Kt + 8) u) S_ij,       S_ij = sum_k |a_ik| |b_jk|

with â = bf16(a) (round to nearest even), u = 2^-23, Kt the total k of the product, everything on the right in fp64.  Where an
epilogue adds an fp32 term t (bias, the accumulation target) the addition is one of the "+ 8" roundings, on a value of magnitude
<= S + |t|: the bound grows by 8 u |t|.  Exact-integer products need no tolerance at all and catch any fragment, transposition, tail or
k-permutation error; every case runs on the three schedules (one pass, split-K slabs, balanced pieces + fix-up).

Geometry: M = 2048, N = 1035 = 16 x 9 tiles of 128 x 128 — the fewest the throughput rule takes, with an 11-wide last tile column."""
import ctypes as C

import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import plan as P

pytestmark = pytest.mark.gpu

SCHEDULES = [1, 2, L.SPLITK_BALANCED]
PRECISIONS = [L.PRECISION_HIGH, L.PRECISION_MEDIUM]
BINDINGS = [(L.AM_KC, L.AM_KC), (L.AM_KC, L.AM_RC), (L.AM_RC, L.AM_RC)]
U = 2.0 ** -23
M, N = 2048, 1035


def _coef(prec, Kt):
    return (Kt + 8) * U if prec == L.PRECISION_MEDIUM else 2.0 ** -16 + (3 * Kt + 8) * U


def _seen(prec, t):
    """the operand as the product sees it, in fp64: bf16-rounded for MEDIUM, itself for HIGH"""
    return t.bfloat16().double() if prec == L.PRECISION_MEDIUM else t.double()


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def sk_ws():
    return torch.empty(L.SK_WORKSPACE_FLOATS, dtype=torch.float32, device="cuda")


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).contiguous()


def _desc(am, bm, segs, zmode, splitk, sk_ws, keep, prec, **kw):
    d = L.GemmDesc()
    d.kind = L.OP_GEMM
    d.amode, d.bmode, d.cmode, d.nseg, d.zmode = am, bm, L.CM_PLAIN, len(segs), zmode
    d.dims_in_use = kw.get("dims", -1)
    d.act = kw.get("act", 0)
    d.beta = kw.get("beta", 0)
    for k in ("bias", "save_z", "save_act", "rowsum_out"):
        if kw.get(k) is not None:
            setattr(d, k, kw[k].data_ptr())
    for q, (ptr, off, width, ld) in enumerate(kw.get("mul", [])):
        d.mul_ptr[q], d.mul_off[q], d.mul_width[q], d.mul_ld[q] = ptr, off, width, ld
    d.mul_nseg = len(kw.get("mul", []))
    for q, sd in enumerate(segs):
        for k, v in sd.items():
            setattr(d.seg[q], k, v)
        if "Mvalid" not in sd:
            d.seg[q].Mvalid = sd["M"]
    d.splitk = splitk
    if splitk == L.SPLITK_BALANCED:
        d.workspace = sk_ws.data_ptr()
    elif splitk > 1:
        nprob = len(segs) if zmode else 1
        ws = torch.empty(splitk * max(s["M"] for s in segs) * max(s["N"] for s in segs) * nprob, device="cuda")
        keep.append(ws)
        d.workspace = ws.data_ptr()
    if prec is not None:
        d.precision = prec
    want = "gemm_fast_bf16_kernel" if prec else "gemm_fast_kernel"
    assert P.gemm_kernel_name(d) == want, "the case must be sized for the throughput kernel"
    return d


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


def _operand(mode, rows, k, values):
    """a [rows x k] operand in the memory layout of `mode`, with a row stride that is no multiple of 4 floats -> (storage view, ld,
    [rows, k] logical view)"""
    def pad(n):
        return n + 1 if (n + 1) % 4 else n + 2

    if mode == L.AM_KC:
        t = torch.zeros(rows, pad(k), device="cuda")[:, :k]
        t.copy_(values)
        return t, t.stride(0), t
    t = torch.zeros(k, pad(rows), device="cuda")[:, :rows]
    t.copy_(values.t())
    return t, t.stride(0), t.t()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exact integers
# ---------------------------------------------------------------------------------------------------------------------------------
_INT_CASES = {}


def _int_case(am, bm, prec):
    """operands and the exact product, built once per (binding, precision) and left unchanged"""
    key = (am, bm, prec)
    if key not in _INT_CASES:
        g = torch.Generator(device="cuda").manual_seed(11 + am * 7 + bm * 3 + prec)
        amax = 2047 if prec == L.PRECISION_HIGH else 127  # 12 significant bits: HIGH's lo plane carries the low 4; 7 bits: exact in bf16
        Ks = [13, 200, 75]
        ops, want = [], torch.zeros(M, N, dtype=torch.float64, device="cuda")
        for k in Ks:
            a = torch.randint(-amax, amax + 1, (M, k), device="cuda", generator=g).float()
            b = torch.randint(-4, 5, (N, k), device="cuda", generator=g).float()
            A, lda, _ = _operand(am, M, k, a)
            B, ldb, _ = _operand(bm, N, k, b)
            ops.append((A, lda, B, ldb, k))
            want += a.double() @ b.double().t()  # (integers, every partial sum < 2^24 < 2^53: the fp64 product IS the int64 product)
        assert float(want.abs().max()) < 2 ** 24
        _INT_CASES[key] = (ops, want.to(torch.int64))
    return _INT_CASES[key]


@pytest.mark.parametrize("splitk", SCHEDULES)
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("am,bm", BINDINGS)
def test_integer_products_are_exact_on_every_binding(lib, sk_ws, am, bm, prec, splitk):
    ops, want = _int_case(am, bm, prec)
    out = torch.full((M, N), float("nan"), device="cuda")
    keep = []
    segs = [dict(A=A.data_ptr(), B=B.data_ptr(), C=out.data_ptr(), M=M, N=N, K=k, lda=lda, ldb=ldb, ldc=N) for A, lda, B, ldb, k in ops]
    _launch(lib, _desc(am, bm, segs, 0, splitk, sk_ws, keep, prec))
    assert torch.isfinite(out).all()
    bad = int((out.to(torch.int64) != want).sum()) + int((out != out.round()).sum())
    assert bad == 0, "%d of %d elements differ from the integer product" % (bad, M * N)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. rounding mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", SCHEDULES)
def test_medium_rounds_operands_to_nearest_even(lib, sk_ws, splitk):
    K = 64
    x = torch.full((M, K), 1.0 + 3 * 2.0 ** -9, device="cuda")  # between 1 and 1 + 2^-7, nearer the latter: RNE -> 1.0078125, truncation -> 1
    W = torch.ones(N, K, device="cuda")
    out = torch.full((M, N), float("nan"), device="cuda")
    keep = []
    _launch(lib, _desc(L.AM_KC, L.AM_KC, [dict(A=x.data_ptr(), B=W.data_ptr(), C=out.data_ptr(), M=M, N=N, K=K, lda=K, ldb=K, ldc=N)], 0, splitk,
                       sk_ws, keep, L.PRECISION_MEDIUM))
    assert bool((out == 64 * 1.0078125).all()), "got %r .. %r" % (float(out.min()), float(out.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. analytic bounds on randn data at shallow K
# ---------------------------------------------------------------------------------------------------------------------------------
_FWD = {}


def _fwd_case():
    if not _FWD:
        torch.manual_seed(21)
        Ks = [13, 96, 51]
        _FWD.update(Ks=Ks, xs=[_rand(M, k + 3)[:, :k] for k in Ks], Ws=[_rand(N, k, scale=0.3) for k in Ks], bias=_rand(N), R1=_rand(M, 700),
                    R2=_rand(M, 200))
        R = torch.zeros(M, N, dtype=torch.float64, device="cuda")
        R[:, :700] = _FWD["R1"].double()
        R[:, 800:1000] = _FWD["R2"].double()
        _FWD["R"] = R
    return _FWD


@pytest.mark.parametrize("splitk", SCHEDULES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_forward_product_with_the_gated_epilogue_meets_the_bound(lib, sk_ws, prec, splitk):
    c = _fwd_case()
    Ks, xs, Ws, bias, R = c["Ks"], c["xs"], c["Ws"], c["bias"], c["R"]
    ldc, dims = N + 5, 1000
    out, z, a = (torch.full((M, ldc), 7.0, device="cuda") for _ in range(3))
    keep = []
    segs = [dict(A=x.data_ptr(), B=W.data_ptr(), C=out.data_ptr(), M=M, N=N, K=k, lda=x.stride(0), ldb=k, ldc=ldc) for x, W, k in zip(xs, Ws, Ks)]
    d = _desc(L.AM_KC, L.AM_KC, segs, 0, splitk, sk_ws, keep, prec, bias=bias, act=L.ACT_SIGMOID, dims=dims, save_z=z, save_act=a,
              mul=[(c["R1"].data_ptr(), 0, 700, 700), (c["R2"].data_ptr(), 800, 200, 200)])
    _launch(lib, d)
    zz = sum(_seen(prec, x) @ _seen(prec, W).t() for x, W in zip(xs, Ws)) + bias.double()
    S = sum(_seen(prec, x).abs() @ _seen(prec, W).abs().t() for x, W in zip(xs, Ws))
    bz = _coef(prec, sum(Ks)) * S + 8 * U * bias.double().abs()
    _within(z[:, :N], zz, bz, "save_z")
    sig = torch.sigmoid(zz)
    _within(a[:, :N], sig, bz / 4 + 2e-5, "save_act")  # |sigmoid'| <= 1/4
    want = sig * R
    want[:, dims:] = 0
    _within(out[:, :N], want, R.abs() * bz / 4 + 2e-5 * want.abs().clamp_min(1.0), "out")
    assert bool((out[:, dims:N] == 0).all()), "columns beyond dims_in_use must be written as 0"
    for t in (out, z, a):
        assert bool((t[:, N:] == 7.0).all()), "columns beyond N were written"


@pytest.mark.parametrize("splitk", SCHEDULES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_input_gradient_batch_meets_the_bound(lib, sk_ws, prec, splitk):
    torch.manual_seed(22)
    K = 150
    keep, segs, checks = [], [], []
    for nin, acc in [(1035, True), (1024, False)]:  # (in features, accumulate: the whole-tile launches start their accumulators from dx)
        dy, W, dx = _rand(M, K), _rand(K, nin, scale=0.3), _rand(M, nin)
        dx0 = dx.double().clone() if acc else torch.zeros(M, nin, dtype=torch.float64, device="cuda")
        segs.append(dict(A=dy.data_ptr(), B=W.data_ptr(), C=dx.data_ptr(), M=M, N=nin, K=K, lda=K, ldb=nin, ldc=nin, accumulate=int(acc)))
        keep.append((dy, W))
        checks.append((dx, dx0 + _seen(prec, dy) @ _seen(prec, W), _coef(prec, K) * (_seen(prec, dy).abs() @ _seen(prec, W).abs()) + 8 * U * dx0.abs()))
    _launch(lib, _desc(L.AM_KC, L.AM_RC, segs, 1, splitk, sk_ws, keep, prec))
    for q, (got, want, bound) in enumerate(checks):
        _within(got, want, bound, "dx[%d]" % q)


@pytest.mark.parametrize("splitk", SCHEDULES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_weight_gradient_batch_with_bias_column_row_mask_and_accumulation_meets_the_bound(lib, sk_ws, prec, splitk):
    torch.manual_seed(23)
    B = 157
    shapes = [(1024, 1034, 1024, 0, 1), (512, 1024, 400, 1, 0), (128, 1024, 128, 0, 0), (1024, 1024, 1024, 1, 1)]  # nout, nin, Mvalid, acc, ones
    keep, segs, checks = [], [], []
    for nout, nin, mv, acc, ones in shapes:
        dy, x, dW, db = _rand(B, nout, scale=0.3), _rand(B, nin), _rand(nout, nin), torch.full((nout,), float("nan"), device="cuda")
        dW0 = dW.double().clone() if acc else torch.zeros(nout, nin, dtype=torch.float64, device="cuda")
        segs.append(dict(A=dy.data_ptr(), B=x.data_ptr(), C=dW.data_ptr(), M=nout, N=nin + ones, K=B, lda=nout, ldb=nin, ldc=nin, Mvalid=mv,
                         accumulate=acc, ones_col=ones, rowsum=db.data_ptr() if ones else None))
        keep.append((dy, x))
        dz = _seen(prec, dy).clone()
        dz[:, mv:] = 0
        xx = _seen(prec, x)
        cf = _coef(prec, B)
        checks.append((dW, dW0 + dz.t() @ xx, cf * (dz.abs().t() @ xx.abs()) + 8 * U * dW0.abs(), db if ones else None, dz.sum(0), cf * dz.abs().sum(0)))
    _launch(lib, _desc(L.AM_RC, L.AM_RC, segs, 1, splitk, sk_ws, keep, prec))
    for q, (dW, want_w, bound_w, db, want_b, bound_b) in enumerate(checks):
        _within(dW, want_w, bound_w, "dW[%d]" % q)
        if db is not None:
            _within(db, want_b, bound_b, "db[%d]" % q)  # (the virtual column is exactly 1.0 in bf16, its lo plane 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. HIGH is far closer to the unrounded product than MEDIUM
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", SCHEDULES)
def test_high_is_at_least_16x_closer_than_medium(lib, sk_ws, splitk):
    torch.manual_seed(24)
    K = 1024
    x, W = _rand(M, K), _rand(N, K, scale=0.05)
    want = x.double() @ W.double().t()
    err = {}
    for prec in PRECISIONS:
        out = torch.full((M, N), float("nan"), device="cuda")
        keep = []
        _launch(lib, _desc(L.AM_KC, L.AM_KC, [dict(A=x.data_ptr(), B=W.data_ptr(), C=out.data_ptr(), M=M, N=N, K=K, lda=K, ldb=K, ldc=N)], 0, splitk,
                           sk_ws, keep, prec))
        assert torch.isfinite(out).all()
        err[prec] = float((out.double() - want).abs().max())
    print("max err against the fp64 product of the unrounded operands: high %.3e, medium %.3e, ratio %.1f"
          % (err[L.PRECISION_HIGH], err[L.PRECISION_MEDIUM], err[L.PRECISION_MEDIUM] / err[L.PRECISION_HIGH]))
    assert err[L.PRECISION_HIGH] <= err[L.PRECISION_MEDIUM] / 16


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. determinism of the balanced schedule, 6. precision = 0 is the fp32 kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("n", [1035, 4200, 8300])
def test_balanced_schedule_is_deterministic_below_between_and_above_the_rounds(lib, sk_ws, prec, n):
    """16 x 9 = 144 tiles (every tile shared), 16 x 33 = 528 (all shared, shares cross tile boundaries), 16 x 65 = 1040 (528 shared +
    512 whole): two launches give the same bits, and they meet the bound"""
    torch.manual_seed(25)
    K = 64
    x, W = _rand(M, K), _rand(n, K, scale=0.3)
    outs, keep = [], []
    for _ in range(2):
        y = torch.full((M, n), float("nan"), device="cuda")
        sk_ws.fill_(float("nan"))
        _launch(lib, _desc(L.AM_KC, L.AM_KC, [dict(A=x.data_ptr(), B=W.data_ptr(), C=y.data_ptr(), M=M, N=n, K=K, lda=K, ldb=K, ldc=n)], 0,
                           L.SPLITK_BALANCED, sk_ws, keep, prec))
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    xx, ww = _seen(prec, x), _seen(prec, W)
    _within(outs[0], xx @ ww.t(), _coef(prec, K) * (xx.abs() @ ww.abs().t()), "y")


@pytest.mark.parametrize("splitk", SCHEDULES)
def test_precision_highest_written_explicitly_is_the_untouched_descriptor(lib, sk_ws, splitk):
    torch.manual_seed(26)
    K = 200
    x, W = _rand(M, K), _rand(N, K, scale=0.3)
    outs, keep = [], []
    for prec in (None, L.PRECISION_HIGHEST):
        y = torch.full((M, N), float("nan"), device="cuda")
        _launch(lib, _desc(L.AM_KC, L.AM_KC, [dict(A=x.data_ptr(), B=W.data_ptr(), C=y.data_ptr(), M=M, N=N, K=K, lda=K, ldb=K, ldc=N)], 0, splitk,
                           sk_ws, keep, prec))
        outs.append(y)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
