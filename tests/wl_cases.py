"""The case table of the worklist items (csrc/worklist_body.h, csrc/worklist.hip): for every item kind the worklist and persistent kernels
have a body for, a list of named cases.  A case is a function that builds, from a seed, the operator's descriptor (the SAME descriptor runs
as the stand-alone launch and as an item), its inputs, its output buffers — guard rows and columns included, pre-filled with a finite
sentinel, or with NaN where the operator must overwrite everything — and a check of those outputs against plain fp64 math.  Every case
names the body it was written to reach (`body`; body_of() reads the same name off an item's geometry), so that a case that silently ran
on another body is noticed.  tests/test_worklist_items_gpu.py runs the cases on the GPU; tests/test_worklist_geometry_cpu.py builds them
on the host (the geometry pass never dereferences a pointer) and holds the launcher's geometry query, which schedule.item_bytes decides
by, against the dry pass of the persistent launch and against body_of().

Plain Python: nothing here touches a GPU at import, and a case built with device="cpu" touches none at all."""
import math

import torch

from nasrec_amd import _lib as L

SENTINEL = 7.0
NAN = float("nan")
WL_TOKS, WL_T32x32, WL_T64x16, WL_T16x64 = 0, 1, 2, 3  # csrc/worklist_body.h
TILE_NAME = {WL_T32x32: "T32x32", WL_T64x16: "T64x16", WL_T16x64: "T16x64"}
BIND_NAME = {0: "KC.KC", 1: "KC.RC", 2: "RC.RC"}  # (RC stands for TOKR too, KC for TOKK: which axis of the operand is contiguous)
WL_LDS_FLOATS = 7840
TRI_LD = 20


def close(a, b, tol=2e-5):
    """the comparison of tests/test_ops_gpu.py: max error against tol * max(1, scale of the reference)"""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * scale, "max err %.3e (scale %.3e)" % (err, scale)  # (a NaN left in `a` fails too)


def body_of(kind, part, geom):
    """the body ps_run_item / wl_run pick for an item of this kind, part and geometry"""
    if kind != L.OP_GEMM:
        return {L.OP_MHA_FWD: "mha_fwd", L.OP_MHA_BWD: "mha_bwd", L.OP_FM_FWD: "fm_fwd", L.OP_FM_BWD: "fm_bwd", L.OP_DOT_TRI_FWD: "dot_tri_fwd",
                L.OP_DOT_TRI_BWD: "dot_tri_bwd", L.OP_COPY_SEGS: "copy_segs", L.OP_GATE_BWD: "gate_bwd", L.OP_REDUCE_ROWS: "reduce_rows",
                L.OP_DEDUP_IDS: "dedup_ids", L.OP_FINAL_FWD: "final_fwd", L.OP_FINAL_FUSED: "final_fused", L.OP_FINAL_BWD: "final_bwd"}[kind]
    if part == L.WL_EPI:
        return "second_pass"
    cfg = geom[2]
    tile, bind, aux = cfg & 3, (cfg >> 2) & 3, (cfg >> 4) & 1
    if tile == WL_TOKS:
        if bind == 3:
            return "dense_small_dx" if geom[1] == 0 else "dense_small.NB%d" % (geom[1] >> 16)
        return "token_fwd" if bind == 1 else "token_dx"
    return "%s.%s.%s" % (TILE_NAME[tile], BIND_NAME[bind], "mask" if aux else "plain")


# what nasrec_worklist_item_geometry calls a body (NASREC_WL_BODY_*): the names above without tile shape, binding and batch count, which
# stay private to csrc/; "kind" = the one body of a kind that is no GEMM
BODY_ENUM_NAME = {L.WL_BODY_KIND: "kind", L.WL_BODY_TILE: "tile", L.WL_BODY_SECOND_PASS: "second_pass", L.WL_BODY_DENSE_SMALL: "dense_small",
                  L.WL_BODY_DENSE_SMALL_DX: "dense_small_dx", L.WL_BODY_TOKEN_FWD: "token_fwd", L.WL_BODY_TOKEN_DX: "token_dx"}


def body_enum_name(kind, part, geom):
    """body_of at the granularity of the public enum"""
    if kind != L.OP_GEMM:
        return "kind"
    head = body_of(kind, part, geom).split(".")[0]
    return "tile" if head in TILE_NAME.values() else head


class Ctx:
    """tensors of one case: generated on the host from the case's seed, moved to `device`, kept alive"""

    def __init__(self, device, seed):
        self.device = device
        self.g = torch.Generator().manual_seed(seed)
        self.keep = []

    def dev(self, t):
        d = t.to(self.device).contiguous()
        if d.data_ptr() == t.data_ptr():
            d = t.clone()
        self.keep.append(d)
        return d

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g) * scale

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g)


class Built:
    """one built case.  desc: the descriptor; parts: the item launches it takes — (WL_WHOLE,), or (WL_MAIN, WL_EPI) for a split-K product
    (the stand-alone launch of the descriptor runs both passes); outs: every buffer the operator writes (name -> device tensor, in full); check(outs): the fp64
    comparison of the stand-alone launch; setup: descriptors launched once, stand-alone, before anything else (the Transformer forward that
    saves the state its backward consumes)"""

    def __init__(self, ctx, desc, outs, check, parts=(L.WL_WHOLE,), setup=()):
        self.ctx, self.desc, self.outs, self.check, self.parts, self.setup = ctx, desc, outs, check, tuple(parts), tuple(setup)
        self.init = None


class Case:
    def __init__(self, kind, name, body, fn, force=False, gemm=False):
        self.kind, self.name, self.body, self.fn, self.force, self.gemm = kind, name, body, fn, force, gemm

    def build(self, device, seed=0):
        b = self.fn(Ctx(device, seed * 1000003 + (hash_name(self.name) & 0xffff)))
        if self.force:
            b.desc._wl_force = True  # (schedule._gemm_wanted would keep it out by its routing policy; the launcher's geometry accepts it)
        return b


def hash_name(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) & 0x7fffffff
    return h


# ======================================================================================================================================
# GEMM: C(i, j) = epilogue(sum_k A(i, k) B(j, k)) (include/nasrec_hip.h)
# ======================================================================================================================================
class Operand:
    """an operand with logical shape [R, K] bound as `mode`; `lead` floats in front and `extra` beyond the rows make the pointer odd and the
    leading dimension wider than the data"""

    def __init__(self, ctx, mode, R, K, extra=0, lead=0, scale=1.0, mask=False):
        self.mode, self.R, self.K = mode, R, K
        if mode == L.AM_KC:
            shape, self.ld = (R, K + extra), K + extra
        elif mode == L.AM_RC:
            shape, self.ld = (K, R + extra), R + extra
        elif mode == L.AM_TOKR:  # rows j = 16 b + e, k = token: t[b, k, e]
            assert R % 16 == 0
            shape, self.ld = (R // 16, K + extra, 16), (K + extra) * 16
        else:  # AM_TOKK: k = 16 b + e, rows = token: t[b, r, e]
            assert K % 16 == 0
            shape, self.ld = (K // 16, R + extra, 16), (R + extra) * 16
        n = 1
        for s in shape:
            n *= s
        self.shape = shape
        self.host = ctx.randn(lead + n, scale=scale)
        self.t = ctx.dev(self.host)
        self.ptr = self.t.data_ptr() + 4 * lead
        self.view = self.host[lead:].view(*shape)
        self.mask = Operand(ctx, mode, R, K, extra, lead) if mask else None

    def logical(self):
        v, R, K = self.view, self.R, self.K
        if self.mode == L.AM_KC:
            m = v[:, :K]
        elif self.mode == L.AM_RC:
            m = v[:, :R].t()
        elif self.mode == L.AM_TOKR:
            m = v[:, :K, :].permute(0, 2, 1).reshape(R, K)
        else:
            m = v[:, :R, :].permute(1, 0, 2).reshape(R, K)
        m = m.double()
        if self.mask is not None:
            m = m * (self.mask.logical_raw() > 0).double()
        return m

    def logical_raw(self):
        keep, self.mask = self.mask, None
        try:
            return self.logical()
        finally:
            self.mask = keep


class Output:
    """C of one problem, [M, N] bound as `cmode`, inside a larger buffer (guard rows and columns keep the sentinel); `acc`: the operator
    adds to what the buffer holds"""

    def __init__(self, ctx, cmode, M, N, acc, guard=3):
        self.cmode, self.M, self.N = cmode, M, N
        if cmode == L.CM_PLAIN:
            self.ld = N + guard
            host = torch.full((M + 2, self.ld), SENTINEL)
            region = torch.zeros(M + 2, self.ld, dtype=torch.bool)
            region[:M, :N] = True
        else:  # CM_TOKJ: C(i, j = 16 b + e) = t[b, i, e]
            assert N % 16 == 0
            self.ld = (M + guard) * 16
            host = torch.full((N // 16, M + guard, 16), SENTINEL)
            region = torch.zeros(N // 16, M + guard, 16, dtype=torch.bool)
            region[:, :M, :] = True
        host[region] = ctx.randn(int(region.sum())) if acc else NAN
        self.host, self.region, self.acc = host, region, acc
        self.t = ctx.dev(host)
        self.ptr = self.t.data_ptr()

    def logical(self, t):
        if self.cmode == L.CM_PLAIN:
            return t[:self.M, :self.N]
        return t[:, :self.M, :].permute(1, 0, 2).reshape(self.M, self.N)

    def check(self, got, ref, tol=2e-5):
        got = got.cpu()
        close(self.logical(got), ref + (self.logical(self.host).double() if self.acc else 0.0), tol)
        assert torch.equal(got[~self.region], self.host[~self.region]), "guard rows / columns were written"


def _epilogue(acc, bias, bias_on_rows, act, dims, mask_on_rows):
    z = acc
    if bias is not None:
        z = z + (bias.double()[:, None] if bias_on_rows else bias.double()[None, :])
    if act == L.ACT_RELU:
        z = z.clamp_min(0)
    if dims >= 0:
        z = z.clone()
        if mask_on_rows:
            z[dims:, :] = 0
        else:
            z[:, dims:] = 0
    return z


def gemm_case(ctx, am, bm, cm, probs, zmode, splitk=1, bias=False, bias_on_rows=0, act=L.ACT_NONE, dims=-1, mask_on_rows=0, beta=0):
    """probs: one dict per z-problem (zmode) or ONE dict whose `K` is a list of k-segments (zmode 0).  Keys: M, N, K, and optionally
    Mvalid, acc, ones, amask, bmask, dead (A = NULL: the segment / problem counts as zeros), extra_a, extra_b, lead_a, lead_b."""
    d = L.GemmDesc()
    d.kind, d.amode, d.bmode, d.cmode, d.zmode, d.act, d.dims_in_use, d.splitk = L.OP_GEMM, am, bm, cm, zmode, act, dims, splitk
    d.bias_on_rows, d.mask_on_rows, d.beta = bias_on_rows, mask_on_rows, beta
    outs, checks = {}, []
    segs = []
    if zmode:
        for p in probs:
            segs.append((p, p["K"], True))
    else:
        assert len(probs) == 1
        for q, K in enumerate(probs[0]["K"]):
            segs.append((probs[0], K, q == 0))
    d.nseg = len(segs)
    Mmax = max(p["M"] for p in probs)
    Nmax = max(p["N"] for p in probs)
    bvec = None
    if bias:
        bvec = ctx.randn(Mmax if bias_on_rows else Nmax)
        d.bias = ctx.dev(bvec).data_ptr()
    accs, cur = [], None
    for q, (p, K, new) in enumerate(segs):
        M, N = p["M"], p["N"]
        ones = p.get("ones", 0)
        dead = p.get("dead", False) if zmode else (q in p.get("dead_segs", ()))
        mv = p.get("Mvalid", M)
        A = Operand(ctx, am, M, K, p.get("extra_a", 0) if zmode else p.get("extra_a", {}).get(q, 0), p.get("lead_a", 0), 0.5, p.get("amask", False))
        Bop = Operand(ctx, bm, N - ones, K, p.get("extra_b", 0), p.get("lead_b", 0) if zmode else p.get("lead_b", {}).get(q, 0), 0.5, p.get("bmask", False))
        s = d.seg[q]
        s.A, s.B = (None if dead else A.ptr), Bop.ptr
        s.M, s.N, s.K, s.lda, s.ldb, s.Mvalid, s.ones_col = M, N, K, A.ld, Bop.ld, mv, ones
        if A.mask is not None and not dead:
            s.Aaux = A.mask.ptr
        if Bop.mask is not None and not dead:
            s.Baux = Bop.mask.ptr
        if new:
            acc_c = bool(p.get("acc", 0)) if zmode else bool(beta)
            cur = dict(out=Output(ctx, cm, M, N - ones, acc_c), acc=torch.zeros(M, N - ones, dtype=torch.float64), rs=torch.zeros(M, dtype=torch.float64),
                       ones=ones, M=M, q=q, rowsum=None)
            accs.append(cur)
            outs["C%d" % q] = cur["out"].t
            if ones:
                rs = ctx.dev(torch.cat([torch.full((M,), NAN), torch.full((2,), SENTINEL)]))
                cur["rowsum"] = rs
                outs["rowsum%d" % q] = rs
                s.rowsum = rs.data_ptr()
            s.accumulate = 1 if (zmode and p.get("acc", 0)) else 0
        s.C, s.ldc = cur["out"].ptr, cur["out"].ld
        if not zmode:
            s.accumulate = 0
        cur.setdefault("terms", []).append((A, Bop, mv, dead))
    if splitk > 1:
        ws = ctx.dev(torch.full((splitk * Mmax * Nmax * (len(probs) if zmode else 1),), 3.0))
        d.workspace = ws.data_ptr()
        outs["workspace"] = ws

    def check(got):
        for c in accs:
            acc, rs = c["acc"].clone(), c["rs"].clone()
            for A, Bop, mv, dead in c["terms"]:
                if dead:
                    continue
                a = A.logical().clone()
                a[mv:, :] = 0
                acc += a @ Bop.logical().t()
                rs += a.sum(1)
            bq = None
            if bvec is not None:
                bq = bvec[:c["M"]] if bias_on_rows else bvec[:acc.shape[1]]
            c["out"].check(got["C%d" % c["q"]], _epilogue(acc, bq, bias_on_rows, act, dims, mask_on_rows))
            if c["ones"]:
                r = got["rowsum%d" % c["q"]].cpu()
                close(r[:c["M"]], rs)
                assert bool((r[c["M"]:] == SENTINEL).all()), "row sums written behind the last row"

    return Built(ctx, d, outs, check, parts=(L.WL_MAIN, L.WL_EPI) if splitk > 1 else (L.WL_WHOLE,))


# ---- wl_dense_small: x W^T, binding KC / KC / plain, not zmode, no mask operands, unsplit -------------------------------------------
def _dense_fwd(ctx, M, N, Ks, dead=(), extra=None, bias=True, act=L.ACT_RELU, dims=-1, beta=0, lead_w=0):
    """k-segments of ONE weight matrix W [N, sum Ks] (so that segment q's pointer is W + 4 * (K_0 + .. + K_{q-1}): not 16-byte aligned
    behind an odd width) against separate inputs x_q [M, K_q (+ extra)]"""
    extra = extra or {}
    Kt = sum(Ks)
    d = L.GemmDesc()
    d.kind, d.amode, d.bmode, d.cmode, d.zmode, d.act, d.dims_in_use, d.splitk, d.beta = L.OP_GEMM, L.AM_KC, L.AM_KC, L.CM_PLAIN, 0, act, dims, 1, beta
    d.nseg = len(Ks)
    Wflat = ctx.randn(lead_w + N * Kt, scale=0.1)  # (lead_w floats in front: the weights themselves start off a 16-byte boundary)
    Wh = Wflat[lead_w:].view(N, Kt)
    Wptr = ctx.dev(Wflat).data_ptr() + 4 * lead_w
    bvec = ctx.randn(N) if bias else None
    if bias:
        d.bias = ctx.dev(bvec).data_ptr()
    out = Output(ctx, L.CM_PLAIN, M, N, bool(beta))
    xs, off = [], 0
    for q, K in enumerate(Ks):
        e = extra.get(q, 0)
        xh = ctx.randn(M, K + e)
        x = ctx.dev(xh)
        s = d.seg[q]
        s.A, s.B, s.C = (None if q in dead else x.data_ptr()), Wptr + 4 * off, out.ptr
        s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.Mvalid = M, N, K, K + e, Kt, out.ld, M
        xs.append(torch.zeros(M, K, dtype=torch.float64) if q in dead else xh[:, :K].double())
        off += K

    def check(got):
        acc = torch.cat(xs, 1) @ Wh.double().t()
        out.check(got["C"], _epilogue(acc, bvec, 0, act, dims, 0))

    return Built(ctx, d, {"C": out.t}, check)


# ---- wl_dense_small_dx: dy W per problem, binding KC / RC / plain, zmode ----------------------------------------------------------------
def _dense_dx(ctx, probs, mask):
    """probs: (M, N, K, accumulate, dead).  dy [M, Kw] (+ its saved activation as the ReLU mask) is shared; W_q [K, N_q] are column ranges
    of one weight matrix"""
    ps = [dict(M=M, N=N, K=K, acc=acc, dead=dead, amask=mask and not dead, extra_a=5, extra_b=2) for M, N, K, acc, dead in probs]
    return gemm_case(ctx, L.AM_KC, L.AM_RC, L.CM_PLAIN, ps, 1)


# ======================================================================================================================================
# the other kinds
# ======================================================================================================================================
MHA_SHAPES = [(48, 16), (48,), (16, 16), (16,), (16,), (16,), (16, 16), (16,), (16, 16), (16,), (16,), (16,)]


def _mha_ref(x, p, dims):
    """modules.py:664-686 in fp64"""
    Win, bin_, Wout, bout, l1w, l1b, W1, c1, W2, c2, l2w, l2b = p
    B, N, E = x.shape
    qkv = x @ Win.t() + bin_
    q, k, v = [t.reshape(B, N, 8, 2).permute(0, 2, 1, 3) for t in (qkv[..., :16], qkv[..., 16:32], qkv[..., 32:])]
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(2), -1) @ v
    a = a.permute(0, 2, 1, 3).reshape(B, N, E) @ Wout.t() + bout
    h = torch.nn.functional.layer_norm(a + x, (16,), l1w, l1b, 1e-5)
    f = torch.relu(h @ W1.t() + c1) @ W2.t() + c2
    out = torch.nn.functional.layer_norm(h + f, (16,), l2w, l2b, 1e-5)
    if dims >= 0:
        out = out * (torch.arange(N) < dims).double()[None, :, None]
    return out


def _slab(ctx, B, N, lead, tail, fill):
    """a token range [B, N, 16] that starts `lead` tokens into a slab of lead + N + tail tokens -> (host slab, host view, device slab,
    device pointer of the view, batch stride, mask of the view inside the slab).  fill: "randn", NAN or SENTINEL for the view; the slab's
    other tokens hold random values ("randn": an input) or the sentinel (an output)"""
    Nt = lead + N + tail
    inside = torch.zeros(B, Nt, 16, dtype=torch.bool)
    inside[:, lead:lead + N] = True
    if fill == "randn":
        host = ctx.randn(B, Nt, 16)
    else:
        host = torch.full((B, Nt, 16), SENTINEL)
        host[inside] = fill
    dev = ctx.dev(host)
    return host, host[:, lead:lead + N], dev, dev.data_ptr() + 4 * lead * 16, Nt * 16, inside


def _view_check(got, host, inside, ref, tol, what):
    """the view of an output slab against fp64, the slab's other tokens bit for bit what they were"""
    got = got.cpu()
    B = host.shape[0]
    close(got[inside].view(B, -1, 16), ref, tol)
    assert torch.equal(got[~inside], host[~inside]), "%s: slab tokens outside the view were written" % what


def _mha(ctx, N, dims, B, backward, saved=True, xs=(0, 0), os=(0, 0), shared=None):
    """xs / os: (tokens in front of, tokens behind) the view inside the slab of x / dx and of out / dout — the plan compiler hands the
    Transformer a token range of a block's slab as its output (ldo > N * 16); shared: (partial_ld, first column) of this node's
    parameter-gradient partials inside a buffer it shares with other nodes (plan.py _flush_mha_reduce), None: a buffer of its own"""
    p = [ctx.randn(*s, scale=(0.3 if len(s) == 2 else 0.1)) for s in MHA_SHAPES]
    p[4] = 0.17 + 0.02 * ctx.randn(16)
    p[10] = 0.17 + 0.02 * ctx.randn(16)
    xslab, x, gxs, xptr, ldx, _ = _slab(ctx, B, N, xs[0], xs[1], "randn")
    if dims >= 0:
        x[:, dims:] = 0  # supernet mode zeroes masked tokens before attention (modules.py:653-662)
        gxs.copy_(xslab)
    x = x.clone()
    gp = [ctx.dev(t) for t in p]
    oslab, _, out, optr, ldo, oin = _slab(ctx, B, N, os[0], os[1], NAN)
    state = ctx.dev(torch.full((B * N * L.MHA_SAVED,), 0.5))
    f = L.MhaDesc()
    f.kind, f.B, f.N, f.ldx, f.ldo, f.dims_in_use = L.OP_MHA_FWD, B, N, ldx, ldo, dims
    f.x, f.out = xptr, optr
    f.saved = state.data_ptr() if (saved or backward) else None
    for q in range(12):
        f.params[q] = gp[q].data_ptr()

    def reference():
        pd = [t.double().requires_grad_(True) for t in p]
        xd = x.double().requires_grad_(True)
        return pd, xd, _mha_ref(xd, pd, dims)

    if not backward:
        def check(got):
            _view_check(got["out"], oslab, oin, reference()[2].detach(), 1e-5, "out")
        outs = {"out": out}
        if saved:
            outs["saved"] = state
        return Built(ctx, f, outs, check)
    _, dout, _, doptr, _, _ = _slab(ctx, B, N, os[0], os[1], "randn")
    dout = dout.clone()
    dxslab, _, dx, dxptr, _, dxin = _slab(ctx, B, N, xs[0], xs[1], NAN)
    pld, pcol = shared if shared is not None else (L.MHA_PARAMS, 0)
    phost = torch.full((B, pld), SENTINEL)
    phost[:, pcol:pcol + L.MHA_PARAMS] = NAN
    part = ctx.dev(phost)
    e = L.MhaDesc()
    e.kind, e.B, e.N, e.ldx, e.ldo, e.dims_in_use = L.OP_MHA_BWD, B, N, ldx, ldo, dims
    e.x, e.dout, e.dx, e.dparams_partial, e.saved = xptr, doptr, dxptr, part.data_ptr() + 4 * pcol, state.data_ptr()
    if shared is not None:
        e.partial_ld = pld
    for q in range(12):
        e.params[q] = gp[q].data_ptr()

    def check_bwd(got):
        pd, xd, ref = reference()
        ref.backward(dout.double())
        _view_check(got["dx"], dxslab, dxin, xd.grad, 2e-5, "dx")
        g = got["part"].cpu()
        keep = torch.ones(pld, dtype=torch.bool)
        keep[pcol:pcol + L.MHA_PARAMS] = False
        assert torch.equal(g[:, keep], phost[:, keep]), "columns of the shared partial buffer outside this node's were written"
        sums, off = g[:, pcol:pcol + L.MHA_PARAMS].double().sum(0), 0
        for q, s in enumerate(MHA_SHAPES):
            n = pd[q].numel()
            close(sums[off:off + n], pd[q].grad.reshape(-1), 2e-5)
            off += n

    return Built(ctx, e, {"dx": dx, "part": part}, check_bwd, setup=(f,))


TAIL = 3  # floats of sentinel behind a buffer whose strides leave no room for guard columns


def _tailed(B, ld, width, fill):
    """a [B, ld] buffer with TAIL floats behind its last row, as one flat tensor -> (flat, mask of the [B, width] view): the view holds
    `fill` (a tensor, NAN), every guard column and the tail the sentinel"""
    flat = torch.full((B * ld + TAIL,), SENTINEL)
    inside = torch.zeros(B * ld + TAIL, dtype=torch.bool)
    inside[:B * ld].view(B, ld)[:, :width] = True
    flat[inside] = fill if not torch.is_tensor(fill) else fill.reshape(-1)
    return flat, inside


def _fm(ctx, B, N, acc, backward, extra=8, ld_ix=20, add=False):
    """extra: tokens of the slab behind the N the operator reads (0: ldx == N * 16); ld_ix = 16: the interaction lives in a buffer of
    its own; add: out = add + FM term in one pass (plan.py op_fm: the node sum of a fixed sub-network without LayerNorm)"""
    Ntot = N + extra
    slab = ctx.randn(B, Ntot, 16)
    gx = ctx.dev(slab)
    x = slab[:, :N]
    d = L.FmDesc()
    d.B, d.N, d.ldx, d.ld_ix, d.accumulate, d.x = B, N, Ntot * 16, ld_ix, acc, gx.data_ptr()
    xd = x.double().requires_grad_(True)

    def fm(xd):
        return xd.sum(1) ** 2 - (xd ** 2).sum(1)

    if not backward:
        base, inside = _tailed(B, ld_ix, 16, ctx.randn(B, 16) if acc else NAN)
        ix = ctx.dev(base)
        d.kind, d.ix = L.OP_FM_FWD, ix.data_ptr()
        addend = None
        if add:  # (same row stride as ix; its guard columns are NaN: read, they would poison the result)
            ah, ain = _tailed(B, ld_ix, 16, 1.0 + ctx.rand(B, 16))
            ah[~ain] = NAN
            addend = ah[ain].view(B, 16).double()
            d.add = ctx.dev(ah).data_ptr()

        def check(got):
            g = got["ix"].cpu()
            ref = fm(x.double()) + (base[inside].view(B, 16).double() if acc else 0.0) + (addend if add else 0.0)
            close(g[inside].view(B, 16), ref)
            assert torch.equal(g[~inside], base[~inside]), "guard columns or the tail behind ix were written"
        return Built(ctx, d, {"ix": ix}, check)
    dixh, dixin = _tailed(B, ld_ix, 16, ctx.randn(B, 16))
    dixh[~dixin] = NAN
    dix = dixh[dixin].view(B, 16)
    init, inside = _tailed(B, Ntot * 16, N * 16, ctx.randn(B, N * 16) if acc else NAN)
    gdix, dx = ctx.dev(dixh), ctx.dev(init)
    d.kind, d.dix, d.dx = L.OP_FM_BWD, gdix.data_ptr(), dx.data_ptr()

    def check_bwd(got):
        g = got["dx"].cpu()
        fm(xd).backward(dix.double())
        close(g[inside].view(B, N, 16), xd.grad + (init[inside].view(B, N, 16).double() if acc else 0.0))
        assert torch.equal(g[~inside], init[~inside]), "tokens behind the view or the tail behind dx were written"
    return Built(ctx, d, {"dx": dx}, check_bwd)


def _dot_tri(ctx, k1, B, backward, pad=3):
    """pad = 0: ld_out == k1 (k1 - 1) / 2 exactly, as the plan compiler emits it (rows start off 16-byte boundaries)"""
    T = ctx.randn(B, k1, 16)
    P = k1 * (k1 - 1) // 2
    gT = ctx.dev(T)
    d = L.DotTriDesc()
    d.B, d.k1, d.ld_out, d.T = B, k1, P + pad, gT.data_ptr()
    li, lj = torch.tril_indices(k1, k1, offset=-1)

    def tri(Td):
        return (Td @ Td.transpose(1, 2))[:, li, lj]

    if not backward:
        init, inside = _tailed(B, P + pad, P, NAN)
        out = ctx.dev(init)
        d.kind, d.out = L.OP_DOT_TRI_FWD, out.data_ptr()

        def check(got):
            g = got["out"].cpu()
            close(g[inside].view(B, P), tri(T.double()))
            assert torch.equal(g[~inside], init[~inside]), "columns beyond the triangle or the tail behind the last row were written"
        return Built(ctx, d, {"out": out}, check)
    douth, doin = _tailed(B, P + pad, P, ctx.randn(B, P))
    douth[~doin] = NAN  # (gradient columns beyond the triangle and behind the last row are nobody's: read, they poison dT)
    dout = douth[doin].view(B, P)
    dTh, dTin = _tailed(B, k1 * 16, k1 * 16, NAN)
    gdo, dT = ctx.dev(douth), ctx.dev(dTh)
    d.kind, d.dout, d.dT = L.OP_DOT_TRI_BWD, gdo.data_ptr(), dT.data_ptr()

    def check_bwd(got):
        Td = T.double().requires_grad_(True)
        tri(Td).backward(dout.double())
        g = got["dT"].cpu()
        close(g[dTin].view(B, k1, 16), Td.grad)
        assert torch.equal(g[~dTin], dTh[~dTin]), "the tail behind dT was written"
    return Built(ctx, d, {"dT": dT}, check_bwd)


def _copy(ctx, B, reverse, big=False):
    c = L.CopySegsDesc()
    if big:  # B * W >= 65535 * 256 elements: a launch of >= 65535 workgroups, whose item table no longer fits 16 bits per entry
        W = 4096
        a = ctx.randn(B, W)
        ga, dst = ctx.dev(a), ctx.dev(torch.full((B, W), NAN))
        c.kind, c.B, c.nseg, c.ld_dst, c.dst = L.OP_COPY_SEGS, B, 1, W, dst.data_ptr()
        c.seg[0], c.width[0], c.ld[0], c.off[0] = ga.data_ptr(), W, W, 0

        def check_big(got):
            assert torch.equal(got["dst"], ga)
        return Built(ctx, c, {"dst": dst}, check_big)
    a, b2 = ctx.randn(B, 5), ctx.randn(B, 9, 16)
    W = 5 + 7 + 9 * 16  # (a gap of 7 columns between the segments, 3 guard columns behind them)
    c.kind, c.B, c.nseg, c.ld_dst, c.accumulate, c.reverse = L.OP_COPY_SEGS, B, 2, W + 3, 0, int(reverse)
    ga, gb = ctx.dev(a), ctx.dev(b2)
    dsth = ctx.randn(B, W + 3) if reverse else torch.full((B, W + 3), SENTINEL)
    dst = ctx.dev(dsth)
    c.dst = dst.data_ptr()
    c.seg[0], c.width[0], c.ld[0], c.off[0] = ga.data_ptr(), 5, 5, 0
    c.seg[1], c.width[1], c.ld[1], c.off[1] = gb.data_ptr(), 9 * 16, 9 * 16, 12
    if not reverse:
        def check(got):
            ref = dsth.clone()
            ref[:, :5] = a
            ref[:, 12:W] = b2.reshape(B, -1)
            assert torch.equal(got["dst"].cpu(), ref)
        return Built(ctx, c, {"dst": dst}, check)
    c.seg_accumulate[0], c.seg_accumulate[1] = 1, 0

    def check_rev(got):
        assert torch.equal(got["a"].cpu(), a + dsth[:, :5]) and torch.equal(got["b"].cpu(), dsth[:, 12:W].reshape(B, 9, 16))
    return Built(ctx, c, {"a": ga, "b": gb}, check_rev)


def _copy_fwd(ctx, B, segs, accumulate, pad=3):
    """forward copy of segments (offset, width, extra columns of the source's stride, NULL?) into dst [B, W + pad], W = the end of the
    last segment.  A NULL segment counts as zeros (plan.py zero_fill); accumulate: dst += instead of dst ="""
    W = max(o + w for o, w, _, _ in segs)
    c = L.CopySegsDesc()
    c.kind, c.B, c.nseg, c.ld_dst, c.accumulate, c.reverse = L.OP_COPY_SEGS, B, len(segs), W + pad, int(accumulate), 0
    covered = torch.zeros(B * (W + pad) + TAIL, dtype=torch.bool)
    for o, w, _, _ in segs:
        covered[:B * (W + pad)].view(B, W + pad)[:, o:o + w] = True
    dsth = torch.full((B * (W + pad) + TAIL,), SENTINEL)
    dsth[covered] = ctx.randn(int(covered.sum())) if accumulate else NAN
    dst = ctx.dev(dsth)
    c.dst = dst.data_ptr()
    ref = dsth.clone()
    if not accumulate:
        ref[covered] = 0.0
    rv = ref[:B * (W + pad)].view(B, W + pad)
    for q, (o, w, extra, null) in enumerate(segs):
        src = ctx.randn(B, w + extra)
        c.seg[q], c.width[q], c.ld[q], c.off[q] = (None if null else ctx.dev(src).data_ptr()), w, (1 if null else w + extra), o
        if not null:
            rv[:, o:o + w] += src[:, :w]

    def check(got):
        assert torch.equal(got["dst"].cpu(), ref)  # (one fp32 addition per element: exact)
    return Built(ctx, c, {"dst": dst}, check)


def _copy_rev(ctx, B, W, acc):
    """the reverse of a one-segment copy without a gap: seg (+)= dst[:, :W]"""
    c = L.CopySegsDesc()
    c.kind, c.B, c.nseg, c.ld_dst, c.reverse = L.OP_COPY_SEGS, B, 1, W, 1
    dsth = ctx.randn(B, W)
    init, inside = _tailed(B, W + 2, W, ctx.randn(B, W) if acc else NAN)
    seg = ctx.dev(init)
    c.dst = ctx.dev(dsth).data_ptr()
    c.seg[0], c.width[0], c.ld[0], c.off[0], c.seg_accumulate[0] = seg.data_ptr(), W, W + 2, 0, int(acc)

    def check(got):
        ref = init.clone()
        ref[inside] = (init[inside] if acc else 0.0) + dsth.reshape(-1)
        assert torch.equal(got["seg"].cpu(), ref)
    return Built(ctx, c, {"seg": seg}, check)


def _gate(ctx, B, D, rsegs, pads=(0, 0, 0)):
    """rsegs: (offset, width, dr_accumulate[, dR wanted = True[, R given = True]]) of the segments of R; columns outside every segment,
    and the columns of a segment whose R is NULL, have R = 0.  pads: extra columns of the row strides of dout, g and dz"""
    dout, gate = ctx.randn(B, D), ctx.rand(B, D)

    def padded(t, pad):  # (an input: the guard columns are NaN — read, they would poison the result)
        h = torch.full((B, D + pad), NAN)
        h[:, :D] = t
        return ctx.dev(h)
    gd, gg = padded(dout, pads[0]), padded(gate, pads[1])
    dzh, dzin = _tailed(B, D + pads[2], D, NAN)
    dz = ctx.dev(dzh)
    e = L.GateBwdDesc()
    e.kind, e.B, e.D, e.ld_dout, e.ld_g, e.ld_dz = L.OP_GATE_BWD, B, D, D + pads[0], D + pads[1], D + pads[2]
    e.dout, e.g, e.dz, e.nseg = gd.data_ptr(), gg.data_ptr(), dz.data_ptr(), len(rsegs)
    outs, rs = {"dz": dz}, []
    Rp = torch.zeros(B, D, dtype=torch.float64)
    for q, seg in enumerate(rsegs):
        off, w, acc = seg[:3]
        want_dr, have_r = (seg[3] if len(seg) > 3 else True), (seg[4] if len(seg) > 4 else True)
        R = ctx.randn(B, w + 2)
        init = torch.full((B, w + 2), SENTINEL)
        init[:, :w] = ctx.randn(B, w) if acc else NAN
        gR, dR = ctx.dev(R), ctx.dev(init)
        e.r_ptr[q], e.dr_ptr[q] = (gR.data_ptr() if have_r else None), (dR.data_ptr() if want_dr else None)
        e.r_off[q], e.r_width[q], e.r_ld[q], e.dr_accumulate[q] = off, w, w + 2, acc
        if have_r:
            Rp[:, off:off + w] = R[:, :w].double()
        if want_dr:
            outs["dR%d" % q] = dR
            rs.append((q, off, w, acc, init))

    def check(got):
        g = got["dz"].cpu()
        close(g[dzin].view(B, D), dout.double() * Rp * gate.double() * (1 - gate.double()))
        assert torch.equal(g[~dzin], dzh[~dzin]), "guard columns or the tail behind dz were written"
        for q, off, w, acc, init in rs:
            g = got["dR%d" % q].cpu()
            close(g[:, :w], (dout.double() * gate.double())[:, off:off + w] + (init[:, :w].double() if acc else 0.0))
            assert torch.equal(g[:, w:], init[:, w:])
    return Built(ctx, e, outs, check)


def _reduce(ctx, R, Cn, lens, first=0, pad=3, null=(), skip=None):
    """column sums of [R, Cn] scattered to destinations of the given lengths, laid end to end from column `first`.  pad: columns of
    the row stride beyond Cn; null: destinations whose pointer is NULL (their sums are dropped); skip: (destination index, columns)
    — a range of columns in front of that destination that belongs to nobody"""
    x = ctx.randn(R, Cn + pad)
    gx = ctx.dev(x)
    r = L.ReduceRowsDesc()
    r.kind, r.R, r.C, r.ld, r.ndst, r.in_ = L.OP_REDUCE_ROWS, R, Cn, Cn + pad, len(lens), gx.data_ptr()
    outs, dsts, off = {}, [], first
    for q, n in enumerate(lens):
        if skip is not None and q == skip[0]:
            off += skip[1]
        init = torch.cat([torch.full((n,), NAN), torch.full((2,), SENTINEL)])
        t = ctx.dev(init)
        r.dst[q], r.dst_off[q], r.dst_len[q] = (None if q in null else t.data_ptr()), off, n
        if q not in null:
            outs["dst%d" % q] = t
            dsts.append((q, off, n))
        off += n
    assert off <= Cn

    def check(got):
        sums = x[:, :Cn].double().sum(0)
        for q, o, n in dsts:
            g = got["dst%d" % q].cpu()
            close(g[:n], sums[o:o + n])
            assert bool((g[n:] == SENTINEL).all())
    return Built(ctx, r, outs, check)


def _dedup(ctx, B, Fs=5):
    """the id patterns of tests/test_dedup_split_gpu.py, one per field: one id everywhere, no duplicates, a table of 3 rows, a table of 50
    rows, every id exactly twice half a batch apart"""
    cols = [torch.full((B,), 12345, dtype=torch.int64), torch.randperm(10 ** 6, generator=ctx.g)[:B], torch.randint(0, 3, (B,), generator=ctx.g),
            torch.randint(0, 50, (B,), generator=ctx.g)]
    half = torch.randperm(10 ** 6, generator=ctx.g)[:(B + 1) // 2]
    cols.append(torch.cat([half, half])[:B])
    idx = torch.stack(cols[:Fs], 1).contiguous()
    cap = 256
    init = dict(leader=torch.full((B * Fs,), 9, dtype=torch.int32), order=torch.full((Fs * cap,), -7, dtype=torch.int32),
                lists=torch.full((Fs * cap,), -7, dtype=torch.int32), counts=torch.full((Fs * 2,), -7, dtype=torch.int32))
    gi = ctx.dev(idx)
    outs = {k: ctx.dev(v) for k, v in init.items()}
    d = L.DedupIdsDesc()
    d.kind, d.B, d.Fs, d.cap, d.idx = L.OP_DEDUP_IDS, B, Fs, cap, gi.data_ptr()
    d.leader, d.order, d.lists, d.counts = (outs[k].data_ptr() for k in ("leader", "order", "lists", "counts"))

    def check(got):
        want = {k: v.clone() for k, v in init.items()}
        lead = want["leader"].view(B, Fs)
        for f in range(Fs):
            members = {}
            for b in range(B):
                members.setdefault(int(idx[b, f]), []).append(b)
            start = nrun = 0
            lead[:, f] = 0
            for b in range(B):  # (leaders in ascending sample order: the body's block scan)
                m = members[int(idx[b, f])]
                if m[0] != b:
                    continue
                lead[b, f] = 2 if len(m) > 1 else 1
                if len(m) > 1:
                    e = (start | (len(m) << 16) | 0x80000000) & 0xffffffff
                    want["lists"][f * cap + nrun] = e - (1 << 32) if e >= (1 << 31) else e
                    want["order"][f * cap + start:f * cap + start + len(m)] = torch.tensor(m, dtype=torch.int32)
                    start += len(m)
                    nrun += 1
            want["counts"][2 * f], want["counts"][2 * f + 1] = nrun, 0
        for k in want:
            assert torch.equal(got[k].cpu(), want[k]), k
    return Built(ctx, d, outs, check)


def _final(ctx, B, kind, accs=(0, 1)):
    """two feature segments (dense D = 300, sparse 7 x 16) in front of the final logit.  FINAL_FWD: logits; FINAL_FUSED: logits and the
    feature gradients; FINAL_BWD with the fused loss: loss, d logits, feature gradients, d w and d bias (batch slices at B >= 1024)"""
    D, N = 300, 7
    K = D + N * 16
    dl, sl = ctx.randn(B, D), ctx.randn(B, N, 16)
    w, bias = ctx.randn(1, K, scale=0.05), ctx.randn(1)
    y = (ctx.rand(B) < 0.25).float()
    g = {k: ctx.dev(v) for k, v in dict(dl=dl, sl=sl, w=w, bias=bias, y=y).items()}
    feats = torch.cat([dl, sl.reshape(B, -1)], 1).double()
    z = feats @ w.double().t()[:, 0] + bias.double()
    f = L.FinalDesc()
    f.kind, f.B, f.nseg = kind, B, 2
    f.w, f.bias = g["w"].data_ptr(), g["bias"].data_ptr()
    f.seg[0], f.width[0], f.ld[0], f.off[0] = g["dl"].data_ptr(), D, D, 0
    f.seg[1], f.width[1], f.ld[1], f.off[1] = g["sl"].data_ptr(), N * 16, N * 16, D
    if kind == L.OP_FINAL_FWD:
        logits = ctx.dev(torch.full((B,), NAN))
        f.logits = logits.data_ptr()

        def check_fwd(got):
            close(got["logits"], z)
        return Built(ctx, f, {"logits": logits}, check_fwd)
    inits = [torch.randn(B, D, generator=ctx.g) if accs[0] else torch.full((B, D), NAN),
             torch.randn(B, N * 16, generator=ctx.g) if accs[1] else torch.full((B, N * 16), NAN)]
    dsegs = [ctx.dev(t) for t in inits]
    loss, dlog = ctx.dev(torch.full((1,), SENTINEL)), ctx.dev(torch.full((B,), SENTINEL))
    f.y, f.loss, f.dlogits_out, f.grad_scale = g["y"].data_ptr(), loss.data_ptr(), dlog.data_ptr(), 1.0 / B
    for q in range(2):
        f.dseg[q], f.dseg_accumulate[q] = dsegs[q].data_ptr(), accs[q]
    outs = {"dseg0": dsegs[0], "dseg1": dsegs[1], "loss": loss, "dlogits": dlog}

    def check_dsegs(got, zz):
        ref = ((torch.sigmoid(zz) - y.double()) / B)[:, None] * w.double()
        close(got["dseg0"], ref[:, :D] + (inits[0].double() if accs[0] else 0.0), 1e-5)
        close(got["dseg1"], ref[:, D:] + (inits[1].double() if accs[1] else 0.0), 1e-5)

    if kind == L.OP_FINAL_FUSED:
        logits = ctx.dev(torch.full((B,), NAN))
        f.logits = logits.data_ptr()
        outs["logits"] = logits

        def check_fused(got):
            close(got["logits"], z)
            check_dsegs(got, z)
        return Built(ctx, f, outs, check_fused)
    lg = (z + 0.01 * torch.randn(B, generator=ctx.g).double()).float()  # (FINAL_BWD reads the logits an earlier launch left)
    f.logits = ctx.dev(lg).data_ptr()
    nsplit = 4 if B >= 1024 else 0
    if nsplit:
        part = ctx.dev(torch.full((nsplit * (K + 1),), NAN))
        f.nsplit, f.dw = nsplit, part.data_ptr()
        outs["part"] = part
    else:
        dw, db = ctx.dev(torch.full((K,), NAN)), ctx.dev(torch.full((1,), NAN))
        f.dw, f.dbias = dw.data_ptr(), db.data_ptr()
        outs["dw"], outs["dbias"] = dw, db

    def check_bwd(got):
        zz = lg.double()
        dlr = (torch.sigmoid(zz) - y.double()) / B
        close(got["dlogits"], dlr, 1e-6)
        close(got["loss"], torch.nn.functional.binary_cross_entropy_with_logits(zz, y.double()).reshape(1), 1e-6)
        check_dsegs(got, zz)
        if nsplit:
            sums = got["part"].view(nsplit, K + 1).double().sum(0).cpu()
            dwg, dbg = sums[:K], sums[K:]
        else:
            dwg, dbg = got["dw"], got["dbias"]
        close(dwg, (dlr[:, None] * feats).sum(0), 1e-5)
        close(dbg, dlr.sum().reshape(1), 1e-5)
    return Built(ctx, f, outs, check_bwd)


# ======================================================================================================================================
# the table
# ======================================================================================================================================
CASES = []


def _add(kind, name, body, fn, force=False, gemm=False):
    CASES.append(Case(kind, name, body, fn, force, gemm))


def _g(name, body, fn, force=False):
    _add("gemm", name, body, fn, force, True)


KC, RC, TOKR, TOKK, PLAIN, TOKJ = L.AM_KC, L.AM_RC, L.AM_TOKR, L.AM_TOKK, L.CM_PLAIN, L.CM_TOKJ

# wl_dense_small
_g("dense_70x77_k13_dead7_45_bias_relu", "dense_small.NB1", lambda c: _dense_fwd(c, 70, 77, [13, 7, 45], dead=(1,), extra={2: 5}))
_g("dense_70x77_k13_dead7_45_dims40_beta", "dense_small.NB1", lambda c: _dense_fwd(c, 70, 77, [13, 7, 45], dead=(1,), extra={2: 5}, dims=40, beta=1, lead_w=1))
_g("dense_3x13_k16", "dense_small.NB1", lambda c: _dense_fwd(c, 3, 13, [16], act=L.ACT_NONE))
_g("dense_17x36_k128_eight_steps", "dense_small.NB1", lambda c: _dense_fwd(c, 17, 36, [128]))
_g("dense_33x16_k100_60_two_batches", "dense_small.NB2", lambda c: _dense_fwd(c, 33, 16, [100, 60], bias=False))
_g("dense_33x16_k260_leaves_the_body", "T64x16.KC.KC.plain", lambda c: _dense_fwd(c, 33, 16, [100, 60, 100]))  # 7 + 4 + 7 = 18 steps > 16
# wl_dense_small_dx
_DX = [(70, 21, 33, 1, False), (70, 100, 128, 0, False), (70, 30, 40, 0, True)]
_g("dense_dx_three_problems", "dense_small_dx", lambda c: _dense_dx(c, _DX, False))
_g("dense_dx_three_problems_relu_mask", "dense_small_dx", lambda c: _dense_dx(c, _DX, True))
_g("dense_dx_k129_leaves_the_body", "T64x16.KC.RC.plain", lambda c: _dense_dx(c, [(70, 21, 129, 1, False), (70, 30, 40, 0, True)], False))
# the token-axis bodies (their shapes: the tests of their own in tests/test_worklist_items_gpu.py) once more for the mixed and persistent forms
_g("token_fwd_17x64_tok5_16_33", "token_fwd",
   lambda c: gemm_case(c, KC, TOKR, TOKJ, [dict(M=40, N=17 * 16, K=[5, 16, 33], extra_b=3)], 0, bias=True, bias_on_rows=1, act=L.ACT_RELU))
_g("token_dx_5x48_tok72_32", "token_dx",
   lambda c: gemm_case(c, RC, TOKR, TOKJ, [dict(M=72, N=5 * 16, K=48, acc=1, bmask=True, extra_a=32), dict(M=32, N=5 * 16, K=48, acc=0, bmask=True, extra_a=72)], 1))


# the general tiles: 3 tiles x 3 binding pairs x {plain, mask operand}
def _batch32(c, am, bm, mask, K):
    """>= 128 workgroups of a 64 x 64 tiling over the problems of one zmode launch: six 300 x 300 products and two ragged ones"""
    tok = am == TOKK
    ones = 1 if am != KC or tok else 0  # (the weight-gradient bindings carry their bias gradient as a virtual column of ones)
    ps = [dict(M=300, N=300 + ones, K=K, acc=q % 2, ones=ones, Mvalid=300 - 7 * (q % 3), amask=mask, extra_a=q % 2, extra_b=3) for q in range(6)]
    ps += [dict(M=13, N=14 + ones, K=K, acc=1, ones=ones, amask=mask), dict(M=200, N=129 + ones, K=K, acc=0, ones=ones, Mvalid=111, amask=mask)]
    return gemm_case(c, am, bm, PLAIN, ps, 1)


for _mask in (False, True):
    _m = "mask" if _mask else "plain"
    _g("t32_kckc_%s_k45" % _m, "T32x32.KC.KC.%s" % _m, (lambda mk: lambda c: _batch32(c, KC, KC, mk, 45))(_mask))
    _g("t32_kcrc_%s_k65" % _m, "T32x32.KC.RC.%s" % _m, (lambda mk: lambda c: _batch32(c, KC, RC, mk, 65))(_mask))
    _g("t32_rcrc_%s_k64" % _m, "T32x32.RC.RC.%s" % _m, (lambda mk: lambda c: _batch32(c, RC, RC, mk, 64))(_mask))
    # 64 x 16 strips: N = 16 B columns against M = 8 .. 64 rows pad least as 64-row strips when M is close to 64
    _g("t64x16_kckc_%s_k4096" % _m, "T64x16.KC.KC.%s" % _m, (lambda mk: lambda c: gemm_case(
        c, TOKK, TOKK, PLAIN, [dict(M=64, N=27 + 1, K=4096, ones=1, Mvalid=40, amask=mk), dict(M=48, N=73 + 1, K=4096, ones=1, acc=1, amask=mk)], 1))(_mask), force=True)
    _g("t64x16_kcrc_%s_tok45" % _m, "T64x16.KC.RC.%s" % _m, (lambda mk: lambda c: gemm_case(
        c, KC, TOKR, TOKJ, [dict(M=64, N=9 * 16, K=[26, 45], Mvalid=50, bmask=mk, extra_b=3)], 0, bias=True, bias_on_rows=1, act=L.ACT_RELU, dims=24,
        mask_on_rows=1))(_mask))
    _g("t64x16_rcrc_%s_k65" % _m, "T64x16.RC.RC.%s" % _m, (lambda mk: lambda c: gemm_case(
        c, RC, TOKR, TOKJ, [dict(M=64, N=9 * 16, K=[48, 65], bmask=mk, extra_a={0: 5, 1: 0})], 0))(_mask))
    # 16 x 64 strips: few rows against many columns
    _g("t16x64_kckc_%s_k300" % _m, "T16x64.KC.KC.%s" % _m, (lambda mk: lambda c: gemm_case(
        c, KC, KC, PLAIN, [dict(M=8, N=200, K=300, acc=1, Mvalid=5, amask=mk, extra_a=1), dict(M=13, N=64, K=45, acc=0, amask=mk)], 1))(_mask))
    _g("t16x64_kcrc_%s_k129" % _m, "T16x64.KC.RC.%s" % _m, (lambda mk: lambda c: gemm_case(
        c, KC, RC, PLAIN, [dict(M=10, N=130, K=129, acc=0, amask=mk, extra_a=3), dict(M=16, N=100, K=64, acc=1, Mvalid=9, amask=mk)], 1))(_mask))
    _g("t16x64_rcrc_%s_tok_k_concat" % _m, "T16x64.RC.RC.%s" % _m, (lambda mk: lambda c: gemm_case(
        c, RC, TOKR, TOKJ, [dict(M=10, N=16 * 16, K=[48, 45, 64], bmask=mk, extra_a={0: 0, 1: 7, 2: 2}, extra_b=3)], 0))(_mask))
# a tie of the padding rule (pad64x16 == pad16x64): the launcher's rule Nmax >= Mmax decides
_g("tie_80x16_16x80_wide", "T64x16.RC.RC.plain", lambda c: gemm_case(c, RC, RC, PLAIN, [dict(M=80, N=16, K=70, Mvalid=60), dict(M=16, N=80, K=33, acc=1)], 1))
_g("tie_128x64_tall", "T16x64.RC.RC.plain", lambda c: gemm_case(c, RC, RC, PLAIN, [dict(M=128, N=64, K=33, acc=1), dict(M=13, N=14, K=33)], 1))
# split-K: WL_MAIN then WL_EPI
_g("splitk3_plain_70x77_k13_dead7_781", "second_pass", lambda c: gemm_case(
    c, KC, KC, PLAIN, [dict(M=70, N=77, K=[13, 7, 781], dead_segs=(1,), extra_a={2: 5})], 0, splitk=3, bias=True, act=L.ACT_RELU, dims=40, beta=1))
_g("splitk4_plain_70x77_k13_dead7_781", "second_pass", lambda c: gemm_case(
    c, KC, KC, PLAIN, [dict(M=70, N=77, K=[13, 7, 781], dead_segs=(1,), extra_a={2: 5})], 0, splitk=4, bias=True, act=L.ACT_RELU, dims=40, beta=1))
_g("splitk3_tokj_40x144_tok26_45", "second_pass", lambda c: gemm_case(
    c, KC, TOKR, TOKJ, [dict(M=40, N=9 * 16, K=[26, 45], extra_b=3)], 0, splitk=3, bias=True, bias_on_rows=1, act=L.ACT_RELU, dims=24, mask_on_rows=1))
_g("splitk4_tokj_40x144_tok26_45", "second_pass", lambda c: gemm_case(
    c, KC, TOKR, TOKJ, [dict(M=40, N=9 * 16, K=[26, 45], extra_b=3)], 0, splitk=4, bias=True, bias_on_rows=1, act=L.ACT_RELU, dims=24, mask_on_rows=1))
_ZSK = [dict(M=192, N=195 + 1, K=96, ones=1, Mvalid=150, acc=0, amask=True), dict(M=64, N=37 + 1, K=96, ones=1, Mvalid=64, acc=1, amask=True),
        dict(M=13, N=14 + 1, K=96, ones=1, Mvalid=9, acc=0, amask=True), dict(M=200, N=129 + 1, K=96, ones=1, Mvalid=111, acc=1, amask=True)]
_g("splitk3_zmode_unequal_weight_gradients", "second_pass", lambda c: gemm_case(c, RC, RC, PLAIN, [dict(p) for p in _ZSK], 1, splitk=3))
_g("splitk4_zmode_unequal_weight_gradients", "second_pass", lambda c: gemm_case(c, RC, RC, PLAIN, [dict(p) for p in _ZSK], 1, splitk=4))

for _N, _dims, _B in [(1, -1, 3), (7, -1, 5), (17, 16, 6), (33, -1, 9), (64, 40, 5), (48, 0, 3)]:
    _add("mha_fwd", "mha_fwd_n%d_d%d_b%d_saved" % (_N, _dims, _B), "mha_fwd", (lambda a: lambda c: _mha(c, a[0], a[1], a[2], False, True))((_N, _dims, _B)))
    _add("mha_fwd", "mha_fwd_n%d_d%d_b%d" % (_N, _dims, _B), "mha_fwd", (lambda a: lambda c: _mha(c, a[0], a[1], a[2], False, False))((_N, _dims, _B)))
    _add("mha_bwd", "mha_bwd_n%d_d%d_b%d" % (_N, _dims, _B), "mha_bwd", (lambda a: lambda c: _mha(c, a[0], a[1], a[2], True))((_N, _dims, _B)))
# ... and the forms the plan compiler emits (tests/op_forms.py harvests them; tests/test_op_forms_cpu.py holds this table against the harvest).
# The Transformer's output is a token range of a block's slab: x 2 tokens into a slab of N + 3, out / dout 1 token into a slab of N + 5
# (ldx != ldo, both != N * 16; the slab's other tokens must keep their bits), the backward's partials the second node of a shared
# [B, 2 * 1696 + 3] buffer ...
_SHARED2 = (2 * L.MHA_PARAMS + 3, L.MHA_PARAMS)
for _N, _dims, _B in [(16, -1, 5), (48, -1, 3), (64, 40, 5), (7, -1, 6)]:
    _kw = dict(xs=(2, 1), os=(1, 4))
    _nm = "n%d_d%d_b%d_slabs" % (_N, _dims, _B)
    _add("mha_fwd", "mha_fwd_%s_saved" % _nm, "mha_fwd", (lambda a, kw: lambda c: _mha(c, a[0], a[1], a[2], False, True, **kw))((_N, _dims, _B), _kw))
    _add("mha_fwd", "mha_fwd_%s" % _nm, "mha_fwd", (lambda a, kw: lambda c: _mha(c, a[0], a[1], a[2], False, False, **kw))((_N, _dims, _B), _kw))
    _add("mha_bwd", "mha_bwd_%s_shared" % _nm, "mha_bwd", (lambda a, kw: lambda c: _mha(c, a[0], a[1], a[2], True, shared=_SHARED2, **kw))((_N, _dims, _B), _kw))
# ... and as the planner lays it out: x a buffer of the Transformer's own (ldx == N * 16), the output in its own buffer (`own`) or a
# token range in front of the 8 dense-to-sparse rows of the block's slab (`slab`); dims = N is what a supernet path at full width carries
_SHARED1 = (L.MHA_PARAMS + 3, 0)
for _N, _dims, _B, _os in [(16, -1, 5, (0, 8)), (48, -1, 3, (0, 0)), (48, -1, 3, (0, 8)), (64, 64, 5, (0, 0)), (64, 40, 5, (0, 8)), (64, -1, 3, (0, 8))]:
    _kw = dict(os=_os)
    _nm = "n%d_d%d_b%d_%s" % (_N, _dims, _B, "slab" if _os[1] else "own")
    _add("mha_fwd", "mha_fwd_%s_saved" % _nm, "mha_fwd", (lambda a, kw: lambda c: _mha(c, a[0], a[1], a[2], False, True, **kw))((_N, _dims, _B), _kw))
    _add("mha_fwd", "mha_fwd_%s" % _nm, "mha_fwd", (lambda a, kw: lambda c: _mha(c, a[0], a[1], a[2], False, False, **kw))((_N, _dims, _B), _kw))
    _add("mha_bwd", "mha_bwd_%s_shared" % _nm, "mha_bwd", (lambda a, kw: lambda c: _mha(c, a[0], a[1], a[2], True, shared=_SHARED1, **kw))((_N, _dims, _B), _kw))
for _B, _N, _acc in [(1, 1, 0), (5, 26, 1), (37, 48, 1), (37, 1, 0), (5, 48, 0), (1, 26, 1)]:
    _add("fm_fwd", "fm_fwd_b%d_n%d_acc%d" % (_B, _N, _acc), "fm_fwd", (lambda a: lambda c: _fm(c, a[0], a[1], a[2], False))((_B, _N, _acc)))
    _add("fm_bwd", "fm_bwd_b%d_n%d_acc%d" % (_B, _N, _acc), "fm_bwd", (lambda a: lambda c: _fm(c, a[0], a[1], a[2], True))((_B, _N, _acc)))
# the planner's strides: the interaction in a buffer of its own (ld_ix == 16), x a whole slab (ldx == N * 16: a sentinel tail stands
# in for the guards) or the node tokens in front of the slab's 8 dense-to-sparse rows; `add`: out = node sum + FM term in one pass
for _B in (1, 5):
    for _N in (16, 48):
        _add("fm_fwd", "fm_fwd_b%d_n%d_add_tight" % (_B, _N), "fm_fwd", (lambda a: lambda c: _fm(c, a[0], a[1], 0, False, extra=0, ld_ix=16, add=True))((_B, _N)))
for _N in (16, 48):
    for _extra in (0, 8):
        _nm = "b5_n%d_%s" % (_N, "tight" if not _extra else "slab")
        _add("fm_fwd", "fm_fwd_%s" % _nm, "fm_fwd", (lambda a: lambda c: _fm(c, 5, a[0], 0, False, extra=a[1], ld_ix=16))((_N, _extra)))
        _add("fm_bwd", "fm_bwd_%s_acc1" % _nm, "fm_bwd", (lambda a: lambda c: _fm(c, 5, a[0], 1, True, extra=a[1], ld_ix=16))((_N, _extra)))
for _k1, _B in [(2, 3), (9, 11), (16, 3), (17, 11), (33, 3), (46, 11)]:
    _add("dot_tri_fwd", "dot_tri_fwd_k%d_b%d" % (_k1, _B), "dot_tri_fwd", (lambda a: lambda c: _dot_tri(c, a[0], a[1], False))((_k1, _B)))
    _add("dot_tri_bwd", "dot_tri_bwd_k%d_b%d" % (_k1, _B), "dot_tri_bwd", (lambda a: lambda c: _dot_tri(c, a[0], a[1], True))((_k1, _B)))
# ld_out == k1 (k1 - 1) / 2 exactly (the planner's: rows start off 16-byte boundaries); 3 floats of sentinel behind the last row
for _k1, _B in [(9, 3), (17, 5), (33, 3), (40, 5), (46, 3)]:
    _add("dot_tri_fwd", "dot_tri_fwd_k%d_b%d_tight" % (_k1, _B), "dot_tri_fwd", (lambda a: lambda c: _dot_tri(c, a[0], a[1], False, pad=0))((_k1, _B)))
    _add("dot_tri_bwd", "dot_tri_bwd_k%d_b%d_tight" % (_k1, _B), "dot_tri_bwd", (lambda a: lambda c: _dot_tri(c, a[0], a[1], True, pad=0))((_k1, _B)))
_add("copy_segs", "copy_forward_gap", "copy_segs", lambda c: _copy(c, 21, False))
_add("copy_segs", "copy_reverse_gap", "copy_segs", lambda c: _copy(c, 21, True))
BIG_COPY = "copy_4097x4096_unpacked_table"
_add("copy_segs", BIG_COPY, "copy_segs", lambda c: _copy(c, 4097, False, big=True))
_add("copy_segs", "copy_forward_accumulate_gap", "copy_segs", lambda c: _copy_fwd(c, 21, [(0, 5, 2, False), (12, 9 * 16, 0, False)], True))
_add("copy_segs", "copy_forward_null_segment_gap", "copy_segs", lambda c: _copy_fwd(c, 21, [(0, 5, 2, False), (7, 40, 0, True), (50, 33, 1, False)], False))
_add("copy_segs", "copy_forward_accumulate_one_segment", "copy_segs", lambda c: _copy_fwd(c, 21, [(0, 37, 3, False)], True))  # (_alias_add, masked_copy)
_add("copy_segs", "copy_forward_zero_fill", "copy_segs", lambda c: _copy_fwd(c, 21, [(0, 37, 0, True)], False))  # (zero_fill)
_add("copy_segs", "copy_reverse_one_segment", "copy_segs", lambda c: _copy_rev(c, 21, 37, 0))
_add("gate_bwd", "gate_21x32_one_segment", "gate_bwd", lambda c: _gate(c, 21, 32, [(0, 13, 1)]))
_add("gate_bwd", "gate_21x32_two_segments", "gate_bwd", lambda c: _gate(c, 21, 32, [(0, 13, 1), (16, 10, 0)]))
# seven segments; the first wants no gradient (the raw dense features), one has no R, the accumulate flags mixed, three different wide
# strides, columns 30 .. 32 in no segment
_add("gate_bwd", "gate_5x61_seven_segments", "gate_bwd", lambda c: _gate(
    c, 5, 61, [(0, 13, 0, False), (13, 8, 1), (21, 9, 0), (33, 5, 1, True, False), (38, 7, 0), (45, 10, 1), (55, 6, 0)], pads=(3, 19, 7)))
# the planner's: one segment (a sampled path, a fixed sub-network) with and without a gradient, covering D or its head; the full path's
# k + 1 segments of block k, the first without a gradient; strides == D (batch 256) or all three padded alike (batch 2048)
for _pads in ((0, 0, 0), (19, 19, 19)):
    _p = "tight" if not _pads[0] else "wide"
    for _nm, _segs, _D in [("head_acc", [(0, 13, 1)], 29), ("head_set", [(0, 13, 0)], 29), ("head_no_dr", [(0, 13, 0, False)], 29),
                           ("all_set", [(0, 29, 0)], 29), ("all_no_dr", [(0, 13, 0, False)], 13)]:
        _add("gate_bwd", "gate_5x%d_%s_%s" % (_D, _nm, _p), "gate_bwd", (lambda a: lambda c: _gate(c, 5, a[0], a[1], pads=a[2]))((_D, _segs, _pads)))
    for _n in range(2, 8):
        _segs = [(0, 13, 0, False)] + [(13 + 8 * (q - 1), 8, 1) for q in range(1, _n)]
        _add("gate_bwd", "gate_5x%d_%d_segments_%s" % (13 + 8 * (_n - 1), _n, _p), "gate_bwd",
             (lambda a: lambda c: _gate(c, 5, a[0], a[1], pads=a[2]))((13 + 8 * (_n - 1), _segs, _pads)))
_MHA_LENS = [48 * 16, 48, 256, 16, 16, 16, 256, 16, 256, 16, 16, 16]
_16DST = [3, 1, 2, 5, 1, 1, 4, 2, 1, 3, 2, 1, 5, 2, 3, 1]
_add("reduce_rows", "reduce_r13_c1696_mha", "reduce_rows", lambda c: _reduce(c, 13, 1696, _MHA_LENS))
_add("reduce_rows", "reduce_r256_c1696_mha", "reduce_rows", lambda c: _reduce(c, 256, 1696, _MHA_LENS))
_add("reduce_rows", "reduce_r256_c37_16dst", "reduce_rows", lambda c: _reduce(c, 256, 37, _16DST))
_add("reduce_rows", "reduce_r1_c37_1dst", "reduce_rows", lambda c: _reduce(c, 1, 37, [26], first=5))
_add("reduce_rows", "reduce_r13_c37_16dst", "reduce_rows", lambda c: _reduce(c, 13, 37, _16DST))
# the three tiers of the row loop (256-row trips, 64-row trips, single rows): R = 64 runs the second alone, R = 300 the first and the third
_add("reduce_rows", "reduce_r64_c37_16dst", "reduce_rows", lambda c: _reduce(c, 64, 37, _16DST))
_add("reduce_rows", "reduce_r300_c37_16dst", "reduce_rows", lambda c: _reduce(c, 300, 37, _16DST))
# the planner's: ld == C, every column somebody's — LayerNorm partials [16 or 64 workgroups, 2 D], one Transformer's partials [256, 1696]
_add("reduce_rows", "reduce_r16_c34_2dst_tight", "reduce_rows", lambda c: _reduce(c, 16, 34, [17, 17], pad=0))
_add("reduce_rows", "reduce_r64_c34_2dst_tight", "reduce_rows", lambda c: _reduce(c, 64, 34, [17, 17], pad=0))
_add("reduce_rows", "reduce_r256_c1696_mha_tight", "reduce_rows", lambda c: _reduce(c, 256, 1696, _MHA_LENS, pad=0))
for _B in (1, 37, 255, 256):
    _add("dedup_ids", "dedup_b%d_fs5" % _B, "dedup_ids", (lambda b: lambda c: _dedup(c, b))(_B))
for _B in (5, 256, 1030):
    _add("final_fwd", "final_fwd_b%d" % _B, "final_fwd", (lambda b: lambda c: _final(c, b, L.OP_FINAL_FWD))(_B))
    _add("final_fused", "final_fused_b%d" % _B, "final_fused", (lambda b: lambda c: _final(c, b, L.OP_FINAL_FUSED, (0, 1)))(_B))
    _add("final_bwd", "final_bwd_b%d_acc01" % _B, "final_bwd", (lambda b: lambda c: _final(c, b, L.OP_FINAL_BWD, (0, 1)))(_B))
    _add("final_bwd", "final_bwd_b%d_acc10" % _B, "final_bwd", (lambda b: lambda c: _final(c, b, L.OP_FINAL_BWD, (1, 0)))(_B))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# every body of ps_run_item / wl_run
ALL_BODIES = (["dense_small.NB1", "dense_small.NB2", "dense_small_dx", "token_fwd", "token_dx", "second_pass"]
              + ["%s.%s.%s" % (t, b, m) for t in TILE_NAME.values() for b in BIND_NAME.values() for m in ("plain", "mask")]
              + ["mha_fwd", "mha_bwd", "fm_fwd", "fm_bwd", "dot_tri_fwd", "dot_tri_bwd", "copy_segs", "gate_bwd", "reduce_rows", "dedup_ids", "final_fwd",
                 "final_fused", "final_bwd"])
