"""Every kernel `launch_layernorm` (csrc/norm_loss_opt.hip) can pick, through the C-ABI, against plain torch fp64 on the same
fp32 inputs: `layer_norm -> act -> prefix mask`, autograd for the backward (run with `-m gpu` on an MI355X).

The launcher chooses the kernel from D, the row strides and the 16-byte alignment of the pointers.  `ln_branch` restates that
choice; every case DECLARES the kernel each direction must reach and the test asserts the restated choice equals it, so a
later change of case parameters cannot silently fold the coverage back onto one kernel (tests/test_layernorm_dispatch_cpu.py
pins `ln_branch` against a hand-written table and the case list against the coverage it has to give).

Tensors are flat allocations with the view starting `*_off` floats in, rows `ld` floats apart and a tail behind the last row.
Everything outside an output view is filled with a sentinel and must come back bit-identical; everything outside an input
view is NaN, so a read of padding poisons the result.

Bars (those of test_ops_gpu.py::test_layernorm): y and the saved mean / rstd within 1e-5, dx / dw / db within 2e-5, relative to
max(1, |ref|max)."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu

EPS = 1e-5
SENTINEL = -12345.678
TAIL = 37  # floats behind the last row of every flat allocation
NONE, RELU, SILU, SIGMOID = L.ACT_NONE, L.ACT_RELU, L.ACT_SILU, L.ACT_SIGMOID
ACT_NAME = {NONE: "none", RELU: "relu", SILU: "silu", SIGMOID: "sigmoid"}
FAMILIES = ("kc", "kc_vec1", "kc_vec2", "kc_vec4", "tokr_reg16", "tokr_reg32", "tokr_reg48", "tokr_reg64", "tok_wave")


# ---- the launcher's choice, restated -----------------------------------------------------------------------------------------
def ln_branch(d):
    """The kernel family launch_layernorm launches for LayerNormDesc `d`; None where it launches nothing (R = 0 or an error
    return).  Pure host logic on the descriptor's integers and pointer values."""
    def al(p):
        return ((p or 0) & 15) == 0
    fwd = d.kind == L.OP_LAYERNORM_FWD
    if d.R == 0:
        return None
    outs_aligned = al(d.y) if fwd else (al(d.dy) and al(d.dx))
    if d.mode == L.AM_KC:
        if d.D > 1024 or (not fwd and d.nblk < 1):
            return None
        vec = d.D % 4 == 0 and d.ldx % 4 == 0 and d.ldy % 4 == 0 and al(d.x) and al(d.w) and al(d.b) and outs_aligned
        if not vec:
            return "kc"
        return "kc_vec1" if d.D <= 256 else ("kc_vec2" if d.D <= 512 else "kc_vec4")
    if d.mode == L.AM_TOKR:
        if d.D > 64 or (not fwd and d.nblk != (d.R + 255) // 256):
            return None
        if d.R % 16 == 0 and d.ldx % 4 == 0 and d.ldy % 4 == 0 and al(d.x) and outs_aligned:
            return "tok_wave"
        return "tokr_reg%d" % (16 if d.D <= 16 else 32 if d.D <= 32 else 48 if d.D <= 48 else 64)
    return None


# ---- cases -------------------------------------------------------------------------------------------------------------------
def plan_nblk(mode, R):
    """workgroups of the backward as plan.emit_layernorm sizes them (_LN_NBLK = 512)"""
    return min((R + 3) // 4, 512) if mode == "kc" else (R + 255) // 256


# Seeds whose fp64 reference puts a ReLU pre-activation within 1e-5 of zero (relu_kink_clear), and what replaces them.
RESEED = {425: 1425, 861: 1861, 881: 1881}


def case(mode, rows, D, fwd, bwd, *, pad=False, ldx=None, ldy=None, x_off=0, y_off=0, dy_off=0, dx_off=0, act=NONE, dims=-1,
         acc=0, nblk=None, reduce=False, data="randn", seed=0):
    """mode "kc": rows = R; mode "tok": rows = B samples of [D, 16] (R = 16 B).  fwd / bwd: the kernel each direction must reach.
    pad: the strides the issue names for a view inside a wider buffer (dense D + 8 / D + 20, token 16 (D + 3) / 16 (D + 5))."""
    R = rows if mode == "kc" else rows * 16
    unit = 1 if mode == "kc" else 16
    if ldx is None:
        ldx = (D + 8 if mode == "kc" else 16 * (D + 3)) if pad else D * unit
    if ldy is None:
        ldy = (D + 20 if mode == "kc" else 16 * (D + 5)) if pad else D * unit
    if nblk is None:
        nblk = plan_nblk(mode, R)
    if act == RELU:
        seed = RESEED.get(seed, seed)
    c = SimpleNamespace(mode=mode, rows=rows, R=R, D=D, fwd=fwd, bwd=bwd, ldx=ldx, ldy=ldy, x_off=x_off, y_off=y_off, dy_off=dy_off,
                        dx_off=dx_off, act=act, dims=dims, acc=acc, nblk=nblk, reduce=reduce, data=data, seed=seed)
    c.id = "%s-%s%d-d%d-ld%d.%d-off%d%d%d%d-%s-dims%d-acc%d-nblk%d%s%s" % (
        mode, "r" if mode == "kc" else "b", rows, D, ldx, ldy, x_off, y_off, dy_off, dx_off, ACT_NAME[act], dims, acc, nblk,
        "-red" if reduce else "", "" if data == "randn" else "-" + data)
    return c


def _mid(D):
    """a prefix length that ends inside a 16-byte vector: 201 wherever the row is that long"""
    return 201 if D > 201 else D // 2 + 1


def _dense_family(Ds, name, n0):
    """Four variants per width: (A) R = 37 inside padded buffers, accumulate, a prefix mask, ONE workgroup in the backward (every wave
    sums 9-10 rows through the grid-stride loop); (B) R = 3, two workgroups (the second has no live row), (C) R = 1, accumulate,
    (D) R = 37 with the plan's workgroup count.  Activation and dims rotate through all their values."""
    acts, out, n = (NONE, RELU, SILU, SIGMOID), [], n0
    for q, D in enumerate(Ds):
        a_dims = (_mid(D), 1, D - 1 if D > 1 else 0)[q % 3]
        out.append(case("kc", 37, D, name, name, pad=True, acc=1, dims=a_dims, act=acts[n % 4], nblk=1, reduce=q == 0, seed=n))
        out.append(case("kc", 3, D, name, name, dims=(0, D + 5, 1)[q % 3], act=acts[(n + 1) % 4], nblk=2, seed=n + 1))
        out.append(case("kc", 1, D, name, name, acc=1, dims=(D, -1, _mid(D))[q % 3], act=acts[(n + 2) % 4], nblk=(1, 2)[q % 2],
                        seed=n + 2))
        out.append(case("kc", 37, D, name, name, dims=(-1, D, 0)[q % 3], act=acts[(n + 3) % 4], seed=n + 3))
        n += 5
    return out


def _dense_cases():
    cs = []
    cs += _dense_family((256, 4, 64), "kc_vec1", 100)
    cs += _dense_family((260, 512), "kc_vec2", 200)
    cs += _dense_family((516, 768, 1024), "kc_vec4", 300)
    cs += _dense_family((65, 1, 3, 63, 190, 1023), "kc", 400)  # D % 4 != 0
    # the scalar kernel through a stride that is no multiple of 4, and through each pointer ln_vec_ok looks at
    cs.append(case("kc", 37, 64, "kc", "kc", ldx=67, ldy=64, act=SILU, dims=33, acc=1, nblk=2, seed=501))
    cs.append(case("kc", 37, 64, "kc", "kc", ldx=64, ldy=67, act=RELU, dims=-1, nblk=1, seed=502))
    cs.append(case("kc", 37, 1024, "kc", "kc", x_off=1, act=NONE, dims=201, acc=1, nblk=2, reduce=True, seed=503))
    cs.append(case("kc", 3, 1024, "kc", "kc_vec4", y_off=1, act=SIGMOID, dims=1024, acc=1, nblk=1, seed=504))
    cs.append(case("kc", 37, 1024, "kc_vec4", "kc", dy_off=1, act=SILU, dims=1029, nblk=1, seed=505))
    cs.append(case("kc", 3, 1024, "kc_vec4", "kc", dx_off=1, pad=True, act=NONE, dims=0, acc=1, nblk=2, seed=506))
    cs.append(case("kc", 37, 512, "kc", "kc_vec2", y_off=3, pad=True, act=RELU, dims=201, nblk=2, seed=507))
    cs.append(case("kc", 37, 256, "kc_vec1", "kc", dx_off=2, pad=True, act=SIGMOID, dims=201, acc=1, seed=508))
    # zero-variance rows (row 0 = 0.5 everywhere, row 1 = 0): rstd = 1 / sqrt(eps), y = act(b) under the mask, bit for bit
    cs.append(case("kc", 3, 64, "kc_vec1", "kc_vec1", act=NONE, dims=40, data="degenerate", seed=601))
    cs.append(case("kc", 37, 516, "kc_vec4", "kc_vec4", act=RELU, dims=-1, nblk=1, data="degenerate", seed=602))
    cs.append(case("kc", 3, 63, "kc", "kc", act=RELU, dims=63, data="degenerate", seed=603))
    cs.append(case("kc", 3, 260, "kc_vec2", "kc_vec2", act=NONE, dims=-1, data="degenerate", seed=604))
    # x = 8 + randn: a one-pass E[x^2] - mu^2 variance loses the bar here, the two-pass kernels must not
    cs.append(case("kc", 37, 1024, "kc_vec4", "kc_vec4", act=NONE, dims=-1, data="mean8", seed=611))
    cs.append(case("kc", 37, 1023, "kc", "kc", act=SILU, dims=-1, nblk=2, data="mean8", seed=612))
    return cs


TOK_D = (1, 15, 16, 17, 32, 33, 48, 49, 64)  # the edges of the 16-token chunks


def _reg(D):
    return "tokr_reg%d" % (16 * ((D + 15) // 16))


def _token_cases():
    acts, cs = (NONE, RELU, SILU, SIGMOID), []
    # wavefront per sample (aligned sample blocks): idle waves (B = 1, 3, 5), a ragged 16-sample backward block and a second one (17, 33)
    for q, D in enumerate(TOK_D):
        n = 700 + 10 * q
        cs.append(case("tok", (17, 33, 5)[q % 3], D, "tok_wave", "tok_wave", pad=True, acc=1, dims=(D // 2, D, 0)[q % 3], act=acts[q % 4],
                       reduce=q == 0, seed=n))
        cs.append(case("tok", (1, 3, 5, 17, 33)[q % 5], D, "tok_wave", "tok_wave", dims=(-1, 0, D // 2, D)[q % 4], act=acts[(q + 1) % 4],
                       seed=n + 1))
        cs.append(case("tok", (33, 1, 3)[q % 3], D, "tok_wave", "tok_wave", acc=1, dims=(D, -1, D // 2, 0)[q % 4], act=acts[(q + 2) % 4],
                       seed=n + 2))
    # thread per row (a sample block off a 16-byte boundary): R = 272 leaves 16 live rows in the second workgroup's first wave,
    # R = 320 one full wave and three dead ones
    for q, D in enumerate(TOK_D):
        n = 800 + 10 * q
        r = _reg(D)
        cs.append(case("tok", (17, 20, 1)[q % 3], D, r, r, x_off=1, pad=q % 2 == 0, acc=q % 2, dims=(D // 2, -1, D, 0)[q % 4], act=acts[2 * q % 4],
                       reduce=D in (16, 32, 48, 64), seed=n))
        cs.append(case("tok", (20, 1, 17)[q % 3], D, r, "tok_wave", y_off=1, pad=q % 2 == 1, acc=(q + 1) % 2, dims=(D, D // 2, -1)[q % 3],
                       act=acts[(2 * q + 1) % 4], seed=n + 1))
        cs.append(case("tok", (1, 17, 20)[q % 3], D, "tok_wave", r, pad=q % 2 == 1, acc=(q + 1) % 2, dims=(-1, D // 2, 0, D)[q % 4],
                       act=acts[(2 * q + 1) % 4], seed=n + 2, **({"dy_off": 1} if q % 2 else {"dx_off": 1})))
    # a sample stride that is no multiple of 4 floats also takes the thread-per-row form
    cs.append(case("tok", 5, 45, "tokr_reg48", "tokr_reg48", ldx=16 * 45 + 2, ldy=16 * 45 + 6, act=RELU, dims=30, acc=1, seed=901))
    # zero-variance rows in both forms
    cs.append(case("tok", 3, 16, "tok_wave", "tok_wave", act=NONE, dims=9, data="degenerate", seed=911))
    cs.append(case("tok", 3, 33, "tok_wave", "tok_wave", act=RELU, dims=-1, data="degenerate", seed=912))
    cs.append(case("tok", 3, 17, "tokr_reg32", "tokr_reg32", x_off=1, act=RELU, dims=-1, data="degenerate", seed=913))
    cs.append(case("tok", 17, 64, "tokr_reg64", "tokr_reg64", x_off=1, act=NONE, dims=40, data="degenerate", seed=914))
    cs.append(case("tok", 5, 64, "tok_wave", "tok_wave", act=SILU, dims=-1, data="mean8", seed=921))
    cs.append(case("tok", 17, 49, "tokr_reg64", "tokr_reg64", x_off=1, act=NONE, dims=-1, data="mean8", seed=922))
    return cs


CASES = _dense_cases() + _token_cases()
assert len({c.id for c in CASES}) == len(CASES)


# ---- data and the fp64 reference ---------------------------------------------------------------------------------------------
def act64(u, act):
    if act == RELU:
        return u.clamp_min(0)
    if act == SILU:
        return u * torch.sigmoid(u)
    if act == SIGMOID:
        return torch.sigmoid(u)
    return u


@functools.lru_cache(maxsize=None)
def reference(seed, R, D, act, dims, data):
    """Seeded fp32 inputs in logical [R, D] form and what fp64 torch makes of them.  Computed once per distinct argument tuple and
    never modified."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, D, generator=g)
    x = 8 + x if data == "mean8" else x * 2 + 0.5
    if data == "degenerate":
        x[0] = 0.5
        x[1] = 0.0
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy, y0, dx0 = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = torch.nn.functional.layer_norm(xd, (D,), wd, bd, EPS)
    mask = (torch.arange(D) < (dims if dims >= 0 else D)).double()
    y = act64(pre, act) * mask
    y.backward(dy.double())
    mean = x.double().mean(1)
    rstd = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + EPS)
    return SimpleNamespace(x=x, w=w, b=b, dy=dy, y0=y0, dx0=dx0, pre=pre.detach(), mask=mask, y=y.detach(), dx=xd.grad, dw=wd.grad,
                           db=bd.grad, mean=mean, rstd=rstd)


def case_reference(c):
    return reference(c.seed, c.R, c.D, c.act, c.dims, c.data)


def relu_kink_clear(c, ref):
    """A ReLU case is only meaningful where no pre-activation sits on the kink: there an fp32 rounding flips a 0/1 gradient.  Decided on
    the fp64 reference alone; a seed that violates it is replaced, the bars are not."""
    return c.act != RELU or float(ref.pre.abs().min()) >= 1e-5


# ---- flat buffers ------------------------------------------------------------------------------------------------------------
def view_index(c, off, ld):
    """flat positions [R, D] of the view: KC x[r * ld + i]; TOKR x[(r >> 4) * ld + (r & 15) + 16 i]"""
    r, i = torch.arange(c.R)[:, None], torch.arange(c.D)[None, :]
    if c.mode == "kc":
        return off + r * ld + i
    return off + (r // 16) * ld + (r % 16) + 16 * i


def flat_len(c, off, ld):
    """sized for the wider of the two strides, so that a kernel that mixes ldx and ldy up still lands inside the allocation (and on
    the sentinel)"""
    return off + (c.R if c.mode == "kc" else c.R // 16) * max(ld, c.ldx, c.ldy) + TAIL


def make_flat(c, off, ld, values, fill):
    f = torch.full((flat_len(c, off, ld),), fill, dtype=torch.float32)
    if values is not None:
        f[view_index(c, off, ld).reshape(-1)] = values.reshape(-1)
    g = f.cuda()
    assert g.data_ptr() % 16 == 0
    return g


def split_flat(c, off, ld, g):
    """(the [R, D] view, True where nothing outside the view changed)"""
    f = g.cpu()
    idx = view_index(c, off, ld)
    out = torch.ones(f.numel(), dtype=torch.bool)
    out[idx.reshape(-1)] = False
    want = torch.full((int(out.sum()),), SENTINEL, dtype=torch.float32)
    return f[idx], torch.equal(f[out].view(torch.int32), want.view(torch.int32))


def guarded(n):
    """n floats of sentinel followed by TAIL more"""
    return torch.full((n + TAIL,), SENTINEL, dtype=torch.float32).cuda()


def tail_intact(g, n):
    want = torch.full((TAIL,), SENTINEL, dtype=torch.float32)
    return torch.equal(g[n:].cpu().view(torch.int32), want.view(torch.int32))


def close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), what + ": not finite"
    scale = max(1.0, float(ref.abs().max())) if ref.numel() else 1.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, scale)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def launch(lib, d):
    L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()


def case_desc(c, x, w, b, y, stats, dy, dx, part):
    """the forward descriptor of case c over flat allocations that start at these (16-byte aligned) addresses"""
    d = L.LayerNormDesc()
    d.kind, d.mode = L.OP_LAYERNORM_FWD, L.AM_KC if c.mode == "kc" else L.AM_TOKR
    d.R, d.D, d.ldx, d.ldy = c.R, c.D, c.ldx, c.ldy
    d.act, d.dims_in_use, d.accumulate, d.eps = c.act, c.dims, c.acc, EPS
    d.x, d.w, d.b = x + 4 * c.x_off, w, b
    d.y, d.stats = y + 4 * c.y_off, stats
    d.dy, d.dx = dy + 4 * c.dy_off, dx + 4 * c.dx_off
    d.dwb_partial, d.nblk = part, c.nblk
    return d


def run_case(lib, c, ref):
    """forward, then backward on the forward's saved statistics; asserts the declared kernels and the untouched surroundings, returns
    the views"""
    R, D = c.R, c.D
    gx = make_flat(c, c.x_off, c.ldx, ref.x, float("nan"))
    gdy = make_flat(c, c.dy_off, c.ldy, ref.dy, float("nan"))
    gy = make_flat(c, c.y_off, c.ldy, ref.y0 if c.acc else None, SENTINEL)
    gdx = make_flat(c, c.dx_off, c.ldx, ref.dx0 if c.acc else None, SENTINEL)
    dx_before = gdx.cpu()
    gw, gb = ref.w.cuda(), ref.b.cuda()
    stats, part = guarded(2 * R), guarded(c.nblk * 2 * D)
    d = case_desc(c, x=gx.data_ptr(), w=gw.data_ptr(), b=gb.data_ptr(), y=gy.data_ptr(), stats=stats.data_ptr(), dy=gdy.data_ptr(),
                  dx=gdx.data_ptr(), part=part.data_ptr())
    assert ln_branch(d) == c.fwd, "forward reaches %s, the case is meant for %s" % (ln_branch(d), c.fwd)
    launch(lib, d)
    y, y_clean = split_flat(c, c.y_off, c.ldy, gy)
    assert y_clean, "forward wrote outside the y view"
    assert tail_intact(stats, 2 * R), "forward wrote past the statistics"
    assert torch.equal(gdx.cpu().view(torch.int32), dx_before.view(torch.int32)), "forward touched dx"
    st = stats[:2 * R].cpu().view(R, 2).clone()
    d.kind = L.OP_LAYERNORM_BWD
    assert ln_branch(d) == c.bwd, "backward reaches %s, the case is meant for %s" % (ln_branch(d), c.bwd)
    launch(lib, d)
    dx, dx_clean = split_flat(c, c.dx_off, c.ldx, gdx)
    assert dx_clean, "backward wrote outside the dx view"
    assert tail_intact(part, c.nblk * 2 * D), "backward wrote past dwb_partial"
    assert torch.equal(split_flat(c, c.y_off, c.ldy, gy)[0], y), "backward touched y"
    assert torch.equal(stats[:2 * R].cpu().view(R, 2), st), "backward changed the statistics"
    partial = part[:c.nblk * 2 * D].cpu().view(c.nblk, 2 * D)
    if c.reduce:  # as plan.emit_layernorm: one fixed-order column reduction scattered to the two parameter gradients
        dw, db = guarded(D), guarded(D)
        r = L.ReduceRowsDesc()
        r.kind, r.R, r.C, r.ld, r.ndst = L.OP_REDUCE_ROWS, c.nblk, 2 * D, 2 * D, 2
        r.in_ = part.data_ptr()
        r.dst[0], r.dst_off[0], r.dst_len[0] = dw.data_ptr(), 0, D
        r.dst[1], r.dst_off[1], r.dst_len[1] = db.data_ptr(), D, D
        launch(lib, r)
        assert tail_intact(dw, D) and tail_intact(db, D)
        dw, db = dw[:D].cpu(), db[:D].cpu()
    else:
        s = partial.double().sum(0)
        dw, db = s[:D], s[D:]
    return SimpleNamespace(y=y, stats=st, dx=dx, dw=dw, db=db, partial=partial)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_layernorm_case(lib, c):
    ref = case_reference(c)
    assert relu_kink_clear(c, ref), "a pre-activation within 1e-5 of the ReLU kink: pick another seed"
    got = run_case(lib, c, ref)
    close(got.y, ref.y + (ref.y0.double() if c.acc else 0), 1e-5, "y")
    close(got.stats[:, 0], ref.mean, 1e-5, "saved mean")
    close(got.stats[:, 1], ref.rstd, 1e-5, "saved rstd")
    close(got.dx, ref.dx + (ref.dx0.double() if c.acc else 0), 2e-5, "dx")
    close(got.dw, ref.dw, 2e-5, "dw")
    close(got.db, ref.db, 2e-5, "db")
    if c.mode == "kc":  # a workgroup whose first row is past R adds nothing
        dead = got.partial[(c.R + 3) // 4:]
        assert dead.numel() == 0 or float(dead.abs().max()) == 0.0
    if c.data == "degenerate":
        assert not c.acc
        want = act64(ref.b, c.act) * ref.mask.float()  # exact in fp32 for NONE / RELU: (x - mu) is exactly 0
        assert c.act in (NONE, RELU) and torch.equal(got.y[:2], want[None, :].expand(2, -1))
        assert torch.equal(got.stats[:2, 0], torch.tensor([0.5, 0.0]))
        for t in (got.y, got.stats, got.dx, got.dw.float(), got.db.float(), got.partial):
            assert bool(torch.isfinite(t).all())


def test_wave_form_and_register_form_agree_on_identical_data(lib):
    """the same [B, D, 16] tensors once in aligned sample blocks (a wavefront per sample) and once one float off (a thread per row)"""
    kw = dict(pad=True, act=SILU, dims=20, acc=1, seed=77)
    wave = case("tok", 17, 33, "tok_wave", "tok_wave", **kw)
    reg = case("tok", 17, 33, "tokr_reg48", "tokr_reg48", x_off=1, y_off=1, dy_off=1, dx_off=1, **kw)
    ref = case_reference(wave)
    assert ref is case_reference(reg)
    a, b = run_case(lib, wave, ref), run_case(lib, reg, ref)
    close(a.y, b.y, 1e-5, "y")
    close(a.stats, b.stats, 1e-5, "stats")
    close(a.dx, b.dx, 2e-5, "dx")
    close(a.partial, b.partial, 2e-5, "dwb_partial")


# ---- error returns: nothing is launched ------------------------------------------------------------------------------------------
def _tiny_desc(kind, mode, R, D, nblk):
    t = [torch.full((4096,), SENTINEL, dtype=torch.float32).cuda() for _ in range(8)]
    d = L.LayerNormDesc()
    d.kind, d.mode, d.R, d.D, d.ldx, d.ldy = kind, mode, R, D, D * (16 if mode == L.AM_TOKR else 1), D * (16 if mode == L.AM_TOKR else 1)
    d.act, d.dims_in_use, d.accumulate, d.eps, d.nblk = NONE, -1, 0, EPS, nblk
    d.x, d.w, d.b, d.y, d.stats, d.dy, d.dx, d.dwb_partial = [b.data_ptr() for b in t]
    return d, t


@pytest.mark.parametrize("kind,mode,R,D,nblk,msg", [
    (L.OP_LAYERNORM_FWD, L.AM_KC, 2, 1025, 1, "D=1025"),
    (L.OP_LAYERNORM_BWD, L.AM_KC, 2, 1025, 1, "D=1025"),
    (L.OP_LAYERNORM_FWD, L.AM_TOKR, 16, 65, 1, "D=65"),
    (L.OP_LAYERNORM_BWD, L.AM_KC, 2, 8, 0, "nblk=0"),
    (L.OP_LAYERNORM_BWD, L.AM_TOKR, 272, 8, 1, "nblk=1, want 2"),
    (L.OP_LAYERNORM_FWD, L.AM_RC, 2, 8, 1, "unsupported mode"),
    (L.OP_LAYERNORM_BWD, L.AM_TOKK, 2, 8, 1, "unsupported mode"),
], ids=["dense-d1025-fwd", "dense-d1025-bwd", "token-d65", "dense-bwd-nblk0", "token-bwd-wrong-nblk", "mode-rc", "mode-tokk"])
def test_layernorm_error_returns_launch_nothing(lib, kind, mode, R, D, nblk, msg):
    d, t = _tiny_desc(kind, mode, R, D, nblk)
    assert ln_branch(d) is None
    assert lib.nasrec_launch(None, C.addressof(d)) != 0
    assert msg in lib.nasrec_last_error().decode()
    with pytest.raises(L.EngineError, match="layernorm"):
        L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()
    for b in t:
        assert bool((b == SENTINEL).all())


@pytest.mark.parametrize("kind", [L.OP_LAYERNORM_FWD, L.OP_LAYERNORM_BWD], ids=["fwd", "bwd"])
@pytest.mark.parametrize("mode", [L.AM_KC, L.AM_TOKR], ids=["dense", "token"])
def test_layernorm_of_no_rows_returns_zero_and_writes_nothing(lib, kind, mode):
    d, t = _tiny_desc(kind, mode, 0, 16, 1)
    assert ln_branch(d) is None
    assert lib.nasrec_launch(None, C.addressof(d)) == 0
    torch.cuda.synchronize()
    for b in t:
        assert bool((b == SENTINEL).all())
