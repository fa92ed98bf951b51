"""The operator kernels that never run as worklist items — activation backward, bias-gradient row sums, memset, the int64 constant
table, scale, column reductions of more than 16 destinations — stand-alone against plain fp64 math (exact equality where the operator
only moves or rounds once), at the descriptor forms the plan compiler emits (tests/op_forms.py; tests/test_op_forms_cpu.py holds the
STANDALONE table below, together with tests/wl_cases.py, against the harvest) and at the shapes where an elementwise or reducing
kernel goes wrong: sizes that are no multiple of the workgroup, strides wider than the data and different per operand, guard columns
and a tail behind every output (NaN where the operator must overwrite, a finite sentinel where it must not write, NaN in the guard
columns of the inputs: read, they poison the result).

Two launches share a test where the planner makes them share a buffer: the Transformer backward writes its per-sample
parameter-gradient partials into ONE [B, nodes * 1696] buffer (partial_ld > 0) that one NASREC_OP_REDUCE_ROWS with 12 destinations
per node sums (plan.py _flush_mha_reduce).

Tolerances: wl_cases.close at 2e-5, the figure the same operators have in tests/test_ops_gpu.py.  The activation backward has no
established figure: its floor is the error of torch's fp32 evaluation of the same formula against fp64 on the case's own inputs
(computable without a GPU), and the kernel is allowed 8 x that floor — the multiple tests/test_operating_point_parity_gpu.py uses —
as a maximum absolute error.  (See test_activation_backward for the figures.)"""
import ctypes as C

import pytest
import torch

import wl_cases as W
from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu
NAN, SENTINEL = W.NAN, W.SENTINEL


class Standalone:
    """descs: the launches, in order; outs: name -> device tensor (in full); check(outs)"""

    def __init__(self, ctx, descs, outs, check):
        self.ctx, self.descs, self.outs, self.check = ctx, list(descs), outs, check


STANDALONE = []


def _add(name, fn):
    STANDALONE.append((name, lambda device, fn=fn, name=name: fn(W.Ctx(device, W.hash_name(name) & 0xffff))))


# ---- activation backward: dz = dy * act'(z) * [i < dims] ----------------------------------------------------------------------------------
ACT_NAME = {L.ACT_RELU: "relu", L.ACT_SILU: "silu", L.ACT_SIGMOID: "sigmoid"}
ACT_FLOOR_MULTIPLE = 8.0


def act_grad(z, dy, act):
    """the formula of csrc/interact.hip act_bwd_kernel in the dtype of its arguments"""
    if act == L.ACT_RELU:
        return torch.where(z > 0, dy, torch.zeros_like(dy))
    s = 1.0 / (1.0 + torch.exp(-z))
    return dy * s * (1.0 + z * (1.0 - s)) if act == L.ACT_SILU else dy * s * (1.0 - s)


def _act_bwd(ctx, mode, act, dims, rows, D, pads):
    """KC: rows = R, element (r, i) at r * ld + i.  TOKR: rows = B samples of D tokens, element (b, i, e) at b * ld + 16 i + e, R = 16 B.
    pads: extra floats of the row strides of dy, z, dz"""
    width = D if mode == L.AM_KC else D * 16
    z, dy = 2.0 * ctx.randn(rows, width), ctx.randn(rows, width)
    z.view(-1)[:8] = torch.tensor([30.0, -30.0, 100.0, -100.0, 0.0, -0.0, 88.0, -88.0])  # (__expf saturates both ways)
    z.view(-1)[-4:] = torch.tensor([100.0, -100.0, 30.0, -30.0])

    def padded(t, pad):
        h = torch.full((rows, width + pad), NAN)
        h[:, :width] = t
        return ctx.dev(h)
    gdy, gz = padded(dy, pads[0]), padded(z, pads[1])
    dzh, inside = W._tailed(rows, width + pads[2], width, NAN)
    dz = ctx.dev(dzh)
    a = L.ActBwdDesc()
    a.kind, a.mode, a.R, a.D = L.OP_ACT_BWD, mode, (rows if mode == L.AM_KC else rows * 16), D
    a.ld_dy, a.ld_z, a.ld_dz, a.act, a.dims_in_use = width + pads[0], width + pads[1], width + pads[2], act, dims
    a.dy, a.z, a.dz = gdy.data_ptr(), gz.data_ptr(), dz.data_ptr()
    keep = torch.ones(width, dtype=torch.bool)
    if dims >= 0:
        keep = (torch.arange(width) if mode == L.AM_KC else torch.arange(width) // 16) < dims
    ref = act_grad(z.double(), dy.double(), act) * keep.double()
    floor = float((act_grad(z, dy, act).double() * keep.double() - ref).abs().max())

    def check(got):
        g = got["dz"].cpu()
        v = g[inside].view(rows, width)
        assert bool(torch.isfinite(v).all()), "a saturated exponential left a NaN or an infinity"
        err = float((v.double() - ref).abs().max())
        print("act_bwd %s: fp32 floor %.3e, kernel %.3e" % (ACT_NAME[act], floor, err))
        assert err <= ACT_FLOOR_MULTIPLE * floor, "max err %.3e against %g x the fp32 floor %.3e" % (err, ACT_FLOOR_MULTIPLE, floor)
        assert bool((v[:, ~keep] == 0).all()), "columns behind dims_in_use are not zero"
        assert torch.equal(g[~inside], dzh[~inside]), "guard columns or the tail behind dz were written"
    return Standalone(ctx, [a], {"dz": dz}, check)


_ACT_SHAPES = {L.AM_KC: ("kc", 37, 45, 20), L.AM_TOKR: ("tokr", 5, 7, 3)}  # (R * D = 1665 and 16 B * D = 560: no multiple of 256)
for _mode, (_mn, _rows, _D, _mid) in _ACT_SHAPES.items():
    for _act in (L.ACT_RELU, L.ACT_SILU, L.ACT_SIGMOID):
        for _dims in (-1, 0, _mid):
            _add("act_bwd_%s_%s_dims%d" % (_mn, ACT_NAME[_act], _dims),
                 (lambda a: lambda c: _act_bwd(c, a[0], a[1], a[2], a[3], a[4], (5, 16, 32)))((_mode, _act, _dims, _rows, _D)))
# the planner's strides (plan.py linear_dense / linear_tokens, SiLU): z and dz buffers of the operator's own, dy the node's output —
# its own buffer or a token range of a block's slab; dims_in_use = the full width
_add("act_bwd_kc_silu_dims45_tight", lambda c: _act_bwd(c, L.AM_KC, L.ACT_SILU, 45, 37, 45, (0, 0, 0)))
_add("act_bwd_tokr_silu_dims7_tight", lambda c: _act_bwd(c, L.AM_TOKR, L.ACT_SILU, 7, 5, 7, (0, 0, 0)))
_add("act_bwd_tokr_silu_dims7_dy_in_slab", lambda c: _act_bwd(c, L.AM_TOKR, L.ACT_SILU, 7, 5, 7, (128, 0, 0)))
ACT_CASES = [n for n, _ in STANDALONE]


# ---- bias-gradient row sums: out[r] = sum_k P(r, k) [aux(r, k) > 0], rows >= rvalid are zero ------------------------------------------------
def _rowsum(ctx, mode, R, K, rvalid, extra):
    if mode == L.AM_RC:  # P(r, k) at k * ld + r
        shape, ld = (K, R + extra), R + extra
    else:  # TOKK: P(r, k = 16 b + e) at b * ld + 16 r + e
        shape, ld = (K // 16, R + extra, 16), (R + extra) * 16
    p, aux = ctx.randn(*shape), ctx.randn(*shape)
    if mode == L.AM_RC:
        logical = lambda t: t[:, :R].t()
        p[:, R:], aux[:, R:] = NAN, NAN
    else:
        logical = lambda t: t[:, :R].permute(1, 0, 2).reshape(R, K)
        p[:, R:], aux[:, R:] = NAN, NAN
    outh = torch.cat([torch.full((R,), NAN), torch.full((W.TAIL,), SENTINEL)])
    out = ctx.dev(outh)
    r = L.RowsumDesc()
    r.kind, r.mode, r.R, r.K, r.ld, r.rvalid = L.OP_ROWSUM, mode, R, K, ld, rvalid
    r.p, r.aux, r.out = ctx.dev(p).data_ptr(), ctx.dev(aux).data_ptr(), out.data_ptr()

    def check(got):
        g = got["out"].cpu()
        ref = (logical(p).double() * (logical(aux) > 0).double()).sum(1)
        ref[rvalid:] = 0
        W.close(g[:R], ref)
        assert bool((g[rvalid:R] == 0).all()) and torch.equal(g[R:], outh[R:])
    return Standalone(ctx, [r], {"out": out}, check)


_add("rowsum_rc_r45_k37_rvalid30_aux", lambda c: _rowsum(c, L.AM_RC, 45, 37, 30, 3))
_add("rowsum_tokk_r7_k592_rvalid5_aux", lambda c: _rowsum(c, L.AM_TOKK, 7, 37 * 16, 5, 3))


# ---- memset, the int64 constant table, scale: exact ------------------------------------------------------------------------------------------
def _memset_flat(ctx, n, lead):
    """n floats `lead` floats into a buffer (lead = 4: 16-byte aligned, the kernel; lead = 1: the runtime's memset)"""
    h = ctx.randn(lead + n + W.TAIL)
    t = ctx.dev(h)
    m = L.MemsetDesc()
    m.kind, m.bytes, m.ptr = L.OP_MEMSET, 4 * n, t.data_ptr() + 4 * lead

    def check(got):
        ref = h.clone()
        ref[lead:lead + n] = 0
        assert torch.equal(got["x"].cpu(), ref)
    return Standalone(ctx, [m], {"x": t}, check)


def _memset_chunks(ctx):
    """chunk table [offset, count, ...] over one arena (plan.path_chunks: 16-byte aligned offsets): counts that are no multiple of 4,
    one chunk longer than a workgroup's first pass, an empty chunk"""
    table = [4, 5, 16, 1030, 1052, 0, 1060, 3, 2048, 256]
    h = ctx.randn(2400)
    t = ctx.dev(h)
    tab = ctx.dev(torch.tensor(table, dtype=torch.int64))
    m = L.MemsetDesc()
    m.kind, m.bytes, m.ptr, m.chunks, m.nchunks = L.OP_MEMSET, 4 * 2400, t.data_ptr(), tab.data_ptr(), len(table) // 2

    def check(got):
        ref = h.clone()
        for o, n in zip(table[::2], table[1::2]):
            ref[o:o + n] = 0
        assert torch.equal(got["x"].cpu(), ref)
    return Standalone(ctx, [m], {"x": t}, check)


_add("memset_flat_98304", lambda c: _memset_flat(c, 98304, 4))  # (a batch-256 gradient slab)
_add("memset_flat_1003_tail", lambda c: _memset_flat(c, 1003, 4))
_add("memset_flat_2101251_strided", lambda c: _memset_flat(c, 2048 * 256 * 4 + 4096 + 3, 4))  # (more than 2048 workgroups' first pass)
_add("memset_flat_2359296_strided", lambda c: _memset_flat(c, 2359296, 4))  # (a batch-2048 gradient slab: [2048, 72, 16])
_add("memset_flat_1003_unaligned", lambda c: _memset_flat(c, 1003, 1))
_add("memset_chunked", _memset_chunks)


def _const_i64(ctx, n):
    vals = [(1 << 40) + 977 * i - (i % 3) * (1 << 33) for i in range(n)]
    h = torch.full((n + 4,), -7, dtype=torch.int64)
    t = ctx.dev(h)
    d = L.ConstI64Desc()
    d.kind, d.n, d.dst = L.OP_CONST_I64, n, t.data_ptr() + 16
    d.vals[:n] = vals

    def check(got):
        ref = h.clone()
        ref[2:2 + n] = torch.tensor(vals, dtype=torch.int64)
        assert torch.equal(got["dst"].cpu(), ref)
    return Standalone(ctx, [d], {"dst": t}, check)


_add("const_i64_n5", lambda c: _const_i64(c, 5))
_add("const_i64_n300", lambda c: _const_i64(c, 300))
_add("const_i64_n448", lambda c: _const_i64(c, L.CONST_I64_MAX))


def _scale(ctx, n, in_place):
    x = ctx.randn(n + W.TAIL)
    gx = ctx.dev(x)
    yh = x.clone() if in_place else torch.cat([torch.full((n,), NAN), torch.full((W.TAIL,), SENTINEL)])
    gy = gx if in_place else ctx.dev(yh)
    d = L.ScaleDesc()
    d.kind, d.n, d.s, d.x, d.y = L.OP_SCALE, n, 0.3, gx.data_ptr(), gy.data_ptr()

    def check(got):
        ref = yh.clone()
        ref[:n] = x[:n] * torch.tensor(0.3, dtype=torch.float32)  # (one fp32 product: exact)
        assert torch.equal(got["y"].cpu(), ref)
    return Standalone(ctx, [d], {"y": gy}, check)


_add("scale_n1003", lambda c: _scale(c, 1003, False))
_add("scale_n1003_in_place", lambda c: _scale(c, 1003, True))
_add("scale_n600001_strided", lambda c: _scale(c, 600001, False))


# ---- column reductions of more than 16 destinations: the compact item form holds 16, so these keep a launch of their own -------------------
def _wide_reduce(ctx, R, lens, pad, null=(), skip=None):
    b = W._reduce(ctx, R, sum(lens) + (skip[1] if skip else 0), lens, pad=pad, null=null, skip=skip)
    return Standalone(ctx, [b.desc], b.outs, b.check)


_add("reduce_r256_c72_24dst_tight", lambda c: _wide_reduce(c, 256, [3] * 24, 0))  # (the planner's: two Transformer nodes, ld == C)
_add("reduce_r300_c150_48dst_wide_null_gap", lambda c: _wide_reduce(c, 300, [3] * 48, 5, null=(7,), skip=(20, 6)))
WIDE_REDUCES = ["reduce_r256_c72_24dst_tight", "reduce_r300_c150_48dst_wide_null_gap"]


def _mha_shared_partials(ctx):
    """two Transformer backward launches (N = 16 and N = 7) write their per-sample parameter-gradient partials into one
    [B, 2 * 1696 + 3] buffer (partial_ld = 3395, the second node at column 1696); one NASREC_OP_REDUCE_ROWS with 24 destinations sums
    both.  The 3 trailing columns keep their sentinel; the sums are the fp64 parameter gradients of both nodes."""
    B, ld = 5, 2 * L.MHA_PARAMS + 3
    nodes = [W._mha(W.Ctx(ctx.device, 11), 16, -1, B, True, os=(0, 8), shared=(ld, 0)),
             W._mha(W.Ctx(ctx.device, 12), 7, -1, B, True, xs=(2, 1), os=(1, 4), shared=(ld, L.MHA_PARAMS))]
    parth = torch.full((B, ld), SENTINEL)
    parth[:, :2 * L.MHA_PARAMS] = NAN
    part = ctx.dev(parth)
    r = L.ReduceRowsDesc()
    r.kind, r.R, r.C, r.ld, r.in_, r.ndst = L.OP_REDUCE_ROWS, B, 2 * L.MHA_PARAMS, ld, part.data_ptr(), 24
    outs, grads, descs = {"part": part}, [], []
    for j, nb in enumerate(nodes):
        ctx.keep.append(nb.ctx)
        nb.desc.dparams_partial = part.data_ptr() + 4 * j * L.MHA_PARAMS
        off = 0
        for q, shp in enumerate(W.MHA_SHAPES):
            n = int(torch.Size(shp).numel())
            t = ctx.dev(torch.cat([torch.full((n,), NAN), torch.full((2,), SENTINEL)]))
            r.dst[12 * j + q], r.dst_off[12 * j + q], r.dst_len[12 * j + q] = t.data_ptr(), j * L.MHA_PARAMS + off, n
            grads.append((j, off, n, t))
            off += n
        outs["dx%d" % j] = nb.outs["dx"]
        descs += list(nb.setup) + [nb.desc]
    descs.append(r)

    def check(got):
        g = got["part"].cpu()
        assert torch.equal(g[:, 2 * L.MHA_PARAMS:], parth[:, 2 * L.MHA_PARAMS:]), "the trailing columns of the shared buffer were written"
        assert not bool(torch.isnan(g[:, :2 * L.MHA_PARAMS]).any()), "a column of the shared buffer was left unwritten"
        for j, nb in enumerate(nodes):
            # the node's own check sums a [B, partial_ld] buffer of partials over its rows: hand it the reduction's sums as row 0
            sums = torch.full((B, ld), SENTINEL)
            sums[:, j * L.MHA_PARAMS:(j + 1) * L.MHA_PARAMS] = 0
            for k, off, n, t in grads:
                if k == j:
                    v = t.cpu()
                    assert bool((v[n:] == SENTINEL).all())
                    sums[0, j * L.MHA_PARAMS + off:j * L.MHA_PARAMS + off + n] = v[:n]
            nb.check({"dx": got["dx%d" % j], "part": sums})
    return Standalone(ctx, descs, outs, check)


_add("mha_bwd_two_nodes_share_partials_reduced_by_24dst", _mha_shared_partials)


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return L.load()


def _launch(lib, b):
    init = {k: v.clone() for k, v in b.outs.items()}
    for d in b.descs:
        L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in b.outs.items()}
    assert any(not torch.equal(init[k], got[k]) for k in got), "a launch that leaves every buffer as it was compares nothing"
    return got


@pytest.mark.parametrize("name,fn", [(n, f) for n, f in STANDALONE if n in ACT_CASES], ids=ACT_CASES)
def test_activation_backward(lib, name, fn):
    """dz = dy * act'(z) * [i < dims_in_use] in both modes, for ReLU, SiLU and sigmoid, at z = +-30, +-88, +-100 among the inputs: finite,
    zero behind the mask, within 8 x the error of torch's fp32 evaluation of the same formula against fp64 on the same inputs.
    Figures measured on an MI355X when the test was added (max absolute error over a case, the range over the cases; the test prints
    both per case): ReLU floor 0, kernel 0 (a select); SiLU floor 2.1e-7 .. 7.4e-7, kernel 1.3e-7 .. 7.4e-7; sigmoid floor 9.7e-8 ..
    1.5e-7, kernel 9.7e-8 .. 1.6e-7; the largest kernel / floor ratio of a case is 1.73 (SiLU: 5.66e-7 against 3.27e-7), against the
    8 allowed.  With dims_in_use = 0 both are 0."""
    b = fn("cuda")
    b.check(_launch(lib, b))


@pytest.mark.parametrize("name,fn", [(n, f) for n, f in STANDALONE if n not in ACT_CASES], ids=[n for n, _ in STANDALONE if n not in ACT_CASES])
def test_stand_alone_operator_against_fp64(lib, name, fn):
    b = fn("cuda")
    b.check(_launch(lib, b))

