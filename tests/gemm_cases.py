"""The case table of the GEMM kernels (csrc/gemm.hip and the six families beside it): one case per descriptor form the plan compiler emits
(tests/op_forms.py _gemm; tests/test_gemm_forms_cpu.py holds this table, together with the GEMM cases of tests/wl_cases.py, against the
harvest), plus the forms no plan emits today and a kernel has code for.  tests/test_gemm_forms_gpu.py launches them.

A case is ONE LINE of the table at the end: the words of the form it was written for.  build() turns the words into a descriptor and into
the reference of the same words — there is one builder for all bindings, because an operand is made as its logical [rows, k] matrix first
and laid out by its addressing mode afterwards.  The shapes are the smallest the routing rule accepts for the form: SHAPES lists candidates
per family, smallest first, and build() takes the first one for which the library's own nasrec_gemm_route and the restated tile rule of
op_forms.general_config answer with the family and the configuration the words claim (so nothing here restates a threshold).

The reference (reference(), in the dtype it is asked for) follows include/nasrec_hip.h: per problem, the sum over its live k-segments of
A(i, k) B(j, k) with A read as 0 where Aaux <= 0 or i >= Mvalid and B as 0 where Baux <= 0; the ones-column's row sums; then
((acc + pre_add + bias) -> save_z -> act -> save_act -> x R -> prefix mask -> + C).

Guards: every operand and every output lives in a wider buffer.  Pad columns of the inputs (operands, mask operands, pre_add, gating
operands) hold NaN — read, they poison the result; outputs that must be overwritten start as NaN, accumulation targets as finite random
values; pad columns of every output (C, save_z, save_act, the row sums, the split-K workspace) and a tail behind it hold the sentinel
and must keep their bits.  With a ones-column, column N - 1 of C is the first pad column.  Edge values that ride along: exact 0.0 and
-0.0 in the mask operands (both count as <= 0), gating segments that leave a gap or have a NULL pointer (both multiply by 0), SiLU and
sigmoid arguments of exactly +-30 and +-88 (row or column 0 of the product is zero and the bias holds them), dims_in_use = 0, a mid
value that is no multiple of 16 (every case with a prefix mask unless its words say otherwise) and the full width.

Plain Python: nothing here touches a GPU at import, and a case built with device="cpu" touches none at all."""
import torch

import op_forms as F
import wl_cases as W
from nasrec_amd import _lib as L

NAN, SENTINEL, TAIL = W.NAN, W.SENTINEL, W.TAIL
PAD = 3
ACT_FLOOR_MULTIPLE = 8.0  # (tests/test_op_forms_gpu.py)
AM = {"KC": L.AM_KC, "RC": L.AM_RC, "TOKR": L.AM_TOKR, "TOKK": L.AM_TOKK}
CM = {"PLAIN": L.CM_PLAIN, "TOKJ": L.CM_TOKJ}
ACT = {"act_none": L.ACT_NONE, "relu": L.ACT_RELU, "silu": L.ACT_SILU, "sigmoid": L.ACT_SIGMOID}
DEFAULTS = ("uniform", "s1", "act_none", "no_bias", "no_mask", "overwrite", "no_pre", "no_z", "no_sact", "no_gate", "no_ones", "aux_none", "mvalid=M",
            "live_A")
SATURATING = (30.0, -30.0, 88.0, -88.0)

# candidate shapes per family, smallest first: (M, N) of the first problem and of a second one (zmode batches); N is rounded up to whole
# samples of 16 where the binding needs it.  general: < 128, 128 .. 1023 and >= 1024 workgroups of a 64 x 64 tiling
SHAPES = {
    "general": [((70, 150), (13, 30)), ((150, 70), (30, 13)), ((763, 741), (13, 30)), ((150, 21850), (13, 30)), ((13, 65500), (5, 30))],
    "kslice": [((250, 500), None)],
    "skinny_n": [((1027, 13), None), ((8190, 13), None)],
    "tinyk": [((1027, 301), (1024, 256))],
    "fast": [((1243, 1507), (200, 300))],
}


def lay_out(logical, mode, pad_fill=NAN):
    """a logical [R, K] matrix as the operand's memory image under addressing mode `mode`, PAD extra columns / rows / tokens of `pad_fill`
    along the axis the leading dimension strides over -> (host image, ld)"""
    R, K = logical.shape
    if mode == L.AM_KC:
        h = torch.full((R, K + PAD), pad_fill)
        h[:, :K] = logical
        return h, K + PAD
    if mode == L.AM_RC:
        h = torch.full((K, R + PAD), pad_fill)
        h[:, :R] = logical.t()
        return h, R + PAD
    if mode == L.AM_TOKR:  # P(r, k) = p[(r >> 4) * ld + (r & 15) + 16 k]: t[b, k, e], r = 16 b + e
        h = torch.full((R // 16, K + 1, 16), pad_fill)
        h[:, :K, :] = logical.view(R // 16, 16, K).permute(0, 2, 1)
        return h, (K + 1) * 16
    h = torch.full((K // 16, R + 1, 16), pad_fill)  # TOKK: P(r, k) = p[(k >> 4) * ld + (k & 15) + 16 r]: t[b, r, e], k = 16 b + e
    h[:, :R, :] = logical.view(R, K // 16, 16).permute(1, 0, 2)
    return h, (R + 1) * 16


def ld_of(mode, R, K):
    """the leading dimension lay_out gives an [R, K] operand"""
    return {L.AM_KC: K + PAD, L.AM_RC: R + PAD, L.AM_TOKR: (K + 1) * 16, L.AM_TOKK: (R + 1) * 16}[mode]


class Plane:
    """an [M, N] array addressed like C (cmode, the problem's ldc) inside a wider buffer with a tail"""

    def __init__(self, cmode, M, N):
        self.cmode, self.M, self.N = cmode, M, N
        if cmode == L.CM_PLAIN:
            self.ld, self.numel = N + PAD, M * (N + PAD) + TAIL
            inside = torch.zeros(self.numel, dtype=torch.bool)
            inside[:M * self.ld].view(M, self.ld)[:, :N] = True
        else:  # C(i, j) = c[(j >> 4) * ldc + (j & 15) + 16 i]: t[b, i, e]
            self.ld, self.numel = (M + 1) * 16, (N // 16) * (M + 1) * 16 + TAIL
            inside = torch.zeros(self.numel, dtype=torch.bool)
            inside[:self.numel - TAIL].view(N // 16, M + 1, 16)[:, :M] = True
        self.inside = inside

    def image(self, fill, pad_fill):
        """flat host image: `fill` (a value, or a logical [M, N] tensor) inside, pad_fill in the pad columns and the tail"""
        h = torch.full((self.numel,), pad_fill)
        if not torch.is_tensor(fill):
            h[self.inside] = fill
        elif self.cmode == L.CM_PLAIN:
            h[:self.M * self.ld].view(self.M, self.ld)[:, :self.N] = fill
        else:
            h[:self.numel - TAIL].view(self.N // 16, self.M + 1, 16)[:, :self.M] = fill.view(self.M, self.N // 16, 16).permute(1, 0, 2)
        return h

    def logical(self, flat):
        if self.cmode == L.CM_PLAIN:
            return flat[:self.M * self.ld].view(self.M, self.ld)[:, :self.N]
        return flat[:self.numel - TAIL].view(self.N // 16, self.M + 1, 16)[:, :self.M].permute(1, 0, 2).reshape(self.M, self.N)


def act_apply(z, act):
    if act == L.ACT_RELU:
        return z.clamp_min(0)
    if act == L.ACT_SILU:
        return z * torch.sigmoid(z)
    return torch.sigmoid(z) if act == L.ACT_SIGMOID else z


class Built:
    """descs: the launches, in order (a deferred second pass is a NASREC_OP_SPLITK_EPILOGUES launch behind the product); desc: the
    product; outs: name -> device tensor, in full; check(got) -> [(output, error, bound)]; family: the route the words claim"""

    def __init__(self, ctx, descs, outs, check, family):
        self.ctx, self.descs, self.desc, self.outs, self.check, self.family = ctx, descs, descs[0], outs, check, family


def parse(words):
    w = words.split()
    s = dict(family=w[0], cfg=w[1], binding=w[2], zform=w[3], words=w)
    rest = set(w[4:])
    s["has"] = lambda x: x in rest
    s["pick"] = lambda *xs: [x for x in xs if x in rest]
    return s


def case_name(words):
    w = words.split()
    return "_".join(x.lstrip("@") for x in w).replace(".", "_").replace("<", "_lt_").replace("=", "_eq_").replace("/", "").replace("+", "_and_")


def _segments(s, M, N, second):
    """-> [problem] = [(M, N, [K of its k-segments], dead k-segments)]"""
    fam, cfg, zform, bind = s["family"], s["cfg"], s["zform"], s["binding"]
    tokk = bind.startswith("TOKK")
    if fam == "general":
        deep = ".deep" in cfg or cfg.startswith("big")
        ks = ([80] if deep else [32]) if tokk else ([77] if deep else [29])
        kn = [13, 77, 29] if deep else [13, 29, 7]
    elif fam == "kslice":
        ks, kn = [531], [13, 531]
    elif fam == "skinny_n":
        ks, kn = [269], [13, 269]
    elif fam == "tinyk":
        ks, kn = [13], [13]
    elif fam == "token_dw":
        ks, kn = [16 * 1024], None
    elif fam == "token_linear":
        ks, kn = [39], [13, 39]
    else:
        ks, kn = ([48] if tokk else [45]), [13, 45]
    dead = ()
    if zform == "kN":
        ks = list(kn)
        if s["has"]("null_A"):
            ks, dead = ks[:1] + [7] + ks[1:], (1,)
    probs = [(M, N, ks, dead)]
    if zform == "zN":
        n = 3 if fam == "token_linear" else 2
        for q in range(1, n):
            k2 = ks[0] if (fam != "general" or tokk) else (45 if ks[0] > 32 else 13)  # (a batch of the general template: unequal depths)
            probs.append((second[0], second[1], [k2], ()))
    return probs


def _candidates(s):
    fam, cfg = s["family"], s["cfg"]
    if fam == "token_linear":
        rb = int(cfg[2])
        return [((16 * rb - 3, 16384), (16 * rb - 7, 16384))]
    if fam == "token_dw":
        rb, cb = int(cfg[2]), int(cfg[6])
        return [((16 * rb - 3, 16 * cb - 5), (max(16 * rb - 20, 5), max(16 * cb - 9, 3)))]
    return SHAPES[fam]


def build(ctx, words):
    s = parse(words)
    for first, second in _candidates(s):
        b = _build(ctx, s, first, second, dry=True)
        f = F.form_of(b)
        if f[1] == s["family"] and f[3] == s["cfg"]:
            return _build(ctx, s, first, second, dry=False)
    raise AssertionError("no candidate shape of %s gives %s %s" % (s["family"], s["family"], s["cfg"]))


def _build(ctx, s, first, second, dry):
    """dry: the descriptor alone, with made-up non-NULL addresses (the routing rule reads shapes and which pointers are NULL)"""
    has = s["has"]
    am, bm, cm = [dict(AM, **CM)[x] for x in s["binding"].split(".")]
    tok_cols = bm == L.AM_TOKR
    ones = any(has(x) for x in ("ones_own_rowsum", "ones_rowsum_out", "ones_both"))
    zmode = s["zform"][0] == "z"

    def fix(mn):  # N = the real columns (whole samples of 16 on the token axis) + the virtual ones-column
        if mn is None:
            return None
        m, n = mn
        if tok_cols:
            n = (n + 15) // 16 * 16
        return m, n + (1 if ones and s["family"] != "token_dw" else 0)
    probs = _segments(s, *fix(first), second=fix(second))
    split = s["pick"]("split", "split_deferred", "balanced")
    S = 1 if not split else (L.SPLITK_BALANCED if split[0] == "balanced" else 3)
    act = ACT[(s["pick"](*ACT) or ["act_none"])[0]]
    Mmax, Nmax = max(p[0] for p in probs), max(p[1] for p in probs)

    d = L.GemmDesc()
    d.kind, d.amode, d.bmode, d.cmode, d.zmode, d.act, d.splitk, d.dims_in_use = L.OP_GEMM, am, bm, cm, int(zmode), act, S, -1
    d.defer_second_pass = int(has("split_deferred"))
    d.nseg = len(probs) if zmode else len(probs[0][2])
    fake = iter(range(1 << 20, 1 << 30, 1 << 12))
    outs = {}

    def dev(h):
        if dry:
            return next(fake)
        t = ctx.dev(h)
        return t.data_ptr()

    def out(name, h):
        if dry:
            return next(fake)
        outs[name] = ctx.dev(h)
        return outs[name].data_ptr()

    def randn(*shape):
        return None if dry else ctx.randn(*shape)

    # ---- what belongs to the launch: bias, prefix mask, gating operand, pre_add / save_z / save_act (addressed like seg[0].C) ----------
    P0 = Plane(cm, probs[0][0], probs[0][1] - (1 if ones else 0))
    bias_rows, mask_rows = has("bias_rows"), has("mask_rows")
    bias = None
    if has("bias_rows") or has("bias_cols"):
        n = Mmax if bias_rows else Nmax
        bias = randn(n)
        if not dry and act in (L.ACT_SILU, L.ACT_SIGMOID):
            bias[:4] = torch.tensor(SATURATING)
        d.bias, d.bias_on_rows = dev(None if dry else torch.cat([bias, torch.full((PAD,), NAN)])), int(bias_rows)
    dims = -1
    if has("mask_rows") or has("mask_cols"):
        n = Mmax if mask_rows else Nmax - (1 if ones else 0)
        dims = 0 if has("@dims0") else (n if has("@dims_full") else (n * 5 // 8) | 1)  # (a mid value that is no multiple of 16 unless the words say otherwise)
        d.dims_in_use, d.mask_on_rows = dims, int(mask_rows)
    gate = None
    if has("gate_covering") or has("gate_gap") or has("gate_gap_null") or has("gate_covering_null"):
        assert cm == L.CM_PLAIN and not zmode
        M, N = probs[0][0], probs[0][1]
        w0 = N // 3 + 1
        cuts = [(0, w0), (w0, N - w0)] if not any(has(x) for x in ("gate_gap", "gate_gap_null")) else [(0, w0), (w0 + 5, N - w0 - 9)]
        if has("gate_gap_null") or has("gate_covering_null"):
            cuts = [cuts[0], (cuts[1][0], 7), (cuts[1][0] + 7, cuts[1][1] - 7)]
        gate = None if dry else torch.zeros(M, N)
        d.mul_nseg = len(cuts)
        for q, (off, w) in enumerate(cuts):
            null = len(cuts) == 3 and q == 1
            r = randn(M, w)
            img = None if dry else lay_out(r, L.AM_KC)[0]
            d.mul_ptr[q], d.mul_off[q], d.mul_width[q], d.mul_ld[q] = (None if null else dev(img)), off, w, w + PAD
            if not dry and not null:
                gate[:, off:off + w] = r
    pre = None
    if has("pre_add"):
        pre = randn(P0.M, P0.N)
        d.pre_add = dev(None if dry else P0.image(pre, NAN))
    if has("save_z"):
        d.save_z = out("save_z", None if dry else P0.image(NAN, SENTINEL))
    if has("save_act"):
        d.save_act = out("save_act", None if dry else P0.image(NAN, SENTINEL))
    if has("ones_rowsum_out"):
        assert not zmode or len(probs) == 1
        d.rowsum_out = out("rowsum0", None if dry else torch.cat([torch.full((probs[0][0],), NAN), torch.full((TAIL,), SENTINEL)]))

    # ---- the problems and their k-segments ----------------------------------------------------------------------------------------------
    plist, q = [], 0
    for pi, (M, N, Ks, dead) in enumerate(probs):
        p_ones = ones and not (pi > 0 and "full_ones+plain" in s["cfg"])
        Nr = N - (1 if ones else 0)  # real columns (a problem of a batch that has no ones-column is as wide as the real columns of the others)
        if has("acc_mixed"):
            acc_c = pi % 2 == 0
        else:
            acc_c = has("accumulate")
        mv = M - 7 if (has("mvalid<M") and pi == 0 and M > 8) else (M - 1 if has("mvalid<M") and pi == 0 else M)
        plane = Plane(cm, M, Nr)
        c0 = randn(M, Nr) if acc_c else None
        cptr = out("C%d" % pi, None if dry else plane.image(c0 if acc_c else NAN, SENTINEL))
        rptr = None
        if p_ones and not has("ones_rowsum_out"):
            rptr = out("rowsum%d" % pi, None if dry else torch.cat([torch.full((M,), NAN), torch.full((TAIL,), SENTINEL)]))
        terms = []
        for ki, K in enumerate(Ks):
            sg = d.seg[q]
            is_dead = ki in dead
            a, b = randn(M, K), randn(Nr, K)
            if not dry:
                a, b = a * 0.5, b * 0.5
                if act in (L.ACT_SILU, L.ACT_SIGMOID) and bias is not None:
                    if bias_rows:
                        b[0] = 0.0  # (column 0 of the product is zero: z(i, 0) = bias[i], +-30 and +-88 among them)
                    else:
                        a[0] = 0.0  # (row 0 of the product is zero: z(0, j) = bias[j])
            want_a = has("aux_A") or has("aux_AB")
            want_b = has("aux_B") or has("aux_AB")
            if has("disagree") and ki % 2 == 1:
                want_a = want_b = False
            ai, lda = (None, ld_of(am, M, K)) if dry else lay_out(a, am)
            bi, ldb = (None, ld_of(bm, Nr, K)) if dry else lay_out(b, bm)
            sg.A, sg.B, sg.C = (None if is_dead else dev(ai)), dev(bi), cptr
            sg.M, sg.N, sg.K, sg.lda, sg.ldb, sg.ldc, sg.Mvalid, sg.ones_col = M, (Nr + 1 if p_ones else Nr), K, lda, ldb, plane.ld, mv, int(p_ones)
            sg.accumulate = int(acc_c and zmode)
            sg.rowsum = rptr
            ma = mb = None
            for want, logical, mode, field in ((want_a, a, am, "Aaux"), (want_b, b, bm, "Baux")):
                if want and not is_dead:
                    m = randn(*(logical.shape if not dry else (1,)))
                    if not dry:
                        m.view(-1)[::7] = 0.0   # exact zeros of both signs count as "<= 0"
                        m.view(-1)[3::11] = -0.0
                    setattr(sg, field, dev(None if dry else lay_out(m, mode)[0]))
                    if field == "Aaux":
                        ma = m
                    else:
                        mb = m
            if not is_dead:
                terms.append((a, b, ma, mb))
            q += 1
        if not zmode:
            d.beta = int(acc_c)
        plist.append(dict(plane=plane, M=M, Nr=Nr, mv=mv, ones=p_ones, acc=acc_c, c0=c0, terms=terms, pi=pi))
    if S != 1:
        n = L.SK_WORKSPACE_FLOATS if S < 0 else S * Mmax * Nmax * len(probs)
        if dry or ctx.device == "cpu":
            d.workspace = next(fake)
        else:  # (written on the device: the balanced schedule's workspace is 100 MB)
            ws = torch.full((n + TAIL,), NAN, device=ctx.device)
            ws[n:] = SENTINEL
            outs["workspace"] = ws
            d.workspace = ws.data_ptr()
    if dry:
        return d

    def reference(dt):
        """-> {output: logical tensor} in dtype dt"""
        res = {}
        for p in plist:
            acc = torch.zeros(p["M"], p["Nr"], dtype=dt)
            rs = torch.zeros(p["M"], dtype=dt)
            for a, b, ma, mb in p["terms"]:
                a, b = a.to(dt).clone(), b.to(dt)
                if ma is not None:
                    a = a * (ma > 0).to(dt)
                if mb is not None:
                    b = b * (mb > 0).to(dt)
                a[p["mv"]:] = 0
                acc += a @ b.t()
                rs += a.sum(1)
            z = acc
            if pre is not None:
                z = z + pre.to(dt)
            if bias is not None:
                z = z + (bias[:p["M"]].to(dt)[:, None] if bias_rows else bias[:p["Nr"]].to(dt)[None, :])
            v = act_apply(z, act)
            if p["pi"] == 0:
                res["save_z"], res["save_act"] = z, v
            if gate is not None:
                v = v * gate[:, :p["Nr"]].to(dt)
            if dims >= 0:
                v = v.clone()
                if mask_rows:
                    v[dims:, :] = 0
                else:
                    v[:, dims:] = 0
            if p["acc"]:
                v = v + p["c0"].to(dt)
            res["C%d" % p["pi"]] = v
            if p["ones"]:
                res["rowsum%d" % p["pi"]] = rs
        return res

    floor_rule = act in (L.ACT_SILU, L.ACT_SIGMOID)
    wgrad = s["family"] == "token_dw" or (s["family"] == "fast" and s["binding"] == "RC.RC.PLAIN")
    tol = 5e-5 if wgrad else 2e-5
    init = {k: v.clone() for k, v in outs.items() if k != "workspace"}

    def check(got):
        ref, ref32 = reference(torch.float64), (reference(torch.float32) if floor_rule else None)
        report = []

        def compare(name, g, want, want32):
            g = g.double().cpu()
            assert not bool(torch.isnan(g).any()), "%s: a NaN was left or produced" % name
            err = float((g - want).abs().max())
            if floor_rule:
                floor = float((want32.double() - want).abs().max())
                bound, how = ACT_FLOOR_MULTIPLE * floor, "%g x the fp32 floor %.3e" % (ACT_FLOOR_MULTIPLE, floor)
            else:
                bound = tol * max(1.0, float(want.abs().max()))
                how = "%g x max(1, |ref|max)" % tol
            report.append((name, err, bound))
            print("  %-9s max err %.3e  bound %.3e (%s)  ratio %.3f" % (name, err, bound, how, err / bound if bound else 0.0))
            assert err <= bound, "%s: max err %.3e against %.3e (%s)" % (name, err, bound, how)

        for p in plist:
            name, plane = "C%d" % p["pi"], p["plane"]
            g = got[name].cpu()
            compare(name, plane.logical(g), ref[name], ref32[name] if ref32 else None)
            assert torch.equal(g[~plane.inside], init[name].cpu()[~plane.inside]), "%s: pad columns or the tail were written" % name
            if dims >= 0:  # a masked element is exactly 0 (+ exactly what the accumulation target held)
                gl = plane.logical(g)
                masked = gl[dims:, :] if mask_rows else gl[:, dims:]
                base = (p["c0"][dims:, :] if mask_rows else p["c0"][:, dims:]) if p["acc"] else torch.zeros_like(masked)
                assert torch.equal(masked, base), "%s: masked elements are not exactly 0" % name
            if p["ones"]:
                rn = "rowsum%d" % p["pi"]
                r = got[rn].cpu()
                compare(rn, r[:p["M"]], ref[rn], ref32[rn] if ref32 else None)
                assert torch.equal(r[p["M"]:], init[rn].cpu()[p["M"]:]), "%s: written behind the last row" % rn
        for name in ("save_z", "save_act"):
            if name in got:
                g = got[name].cpu()
                compare(name, P0.logical(g), ref[name], ref32[name] if ref32 else None)
                assert torch.equal(g[~P0.inside], init[name].cpu()[~P0.inside]), "%s: pad columns or the tail were written" % name
        if "workspace" in got:
            assert bool((got["workspace"][-TAIL:] == SENTINEL).all()), "the tail behind the split-K workspace was written"
        return report

    descs = [d]
    if has("split_deferred"):
        e = L.SplitkEpiloguesDesc()
        e.kind, e.n = L.OP_SPLITK_EPILOGUES, 1
        e.g[0] = d
        descs.append(e)
    b = Built(ctx, descs, outs, check, s["family"])
    b.reference, b.planes = reference, dict([("C%d" % p["pi"], p["plane"]) for p in plist] + [("save_z", P0), ("save_act", P0)])
    return b


class Case:
    def __init__(self, words):
        self.words, self.name, self.family = words, case_name(words), words.split()[0]

    def build(self, device):
        return build(W.Ctx(device, W.hash_name(self.name) & 0xffff), self.words)

    def form(self):
        """the form of the case's product descriptor, from shapes and NULL-ness alone (no tensor is made)"""
        s = parse(self.words)
        for first, second in _candidates(s):
            f = F.form_of(_build(None, s, first, second, dry=True))
            if f[1] == s["family"] and f[3] == s["cfg"]:
                return f
        raise AssertionError("no candidate shape of %s gives %s" % (s["family"], self.words))


CASES = []


def _c(words):
    CASES.append(Case(words))


# ---- the forms the plan compiler emits: family, configuration, binding, k-segments / z-problems, then every word that is not a default
# (DEFAULTS) ------------------------------------------------------------------------------------------------------------------------------
_c("fast no_ones_template.acc_in_tile KC.RC.PLAIN z1 accumulate")
_c("fast no_ones_template.acc_in_tile KC.RC.PLAIN zN accumulate")
_c("fast no_ones_template.acc_in_tile RC.RC.PLAIN zN accumulate")
_c("fast no_ones_template.acc_in_tile+plain KC.RC.PLAIN zN acc_mixed")
_c("fast no_ones_template.nread0 KC.KC.PLAIN kN bias_cols mask_cols")
_c("fast no_ones_template.nread1 KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap")
_c("fast no_ones_template.nread1 KC.KC.PLAIN kN bias_cols mask_cols accumulate")
_c("fast no_ones_template.nread1 KC.KC.PLAIN kN sigmoid bias_cols save_act gate_covering")
_c("fast no_ones_template.plain KC.KC.PLAIN kN")
_c("fast no_ones_template.plain KC.RC.PLAIN z1")
_c("fast no_ones_template.plain KC.RC.PLAIN zN")
_c("fast no_ones_template.plain RC.RC.PLAIN zN")
_c("fast no_ones_template.second_pass KC.KC.PLAIN k1 split bias_cols mask_cols accumulate")
_c("fast no_ones_template.second_pass KC.KC.PLAIN k1 split bias_cols mask_cols")
_c("fast no_ones_template.second_pass KC.KC.PLAIN k1 split bias_cols")
_c("fast no_ones_template.second_pass KC.KC.PLAIN k1 split")
_c("fast no_ones_template.second_pass KC.KC.PLAIN k1 split sigmoid bias_cols save_act gate_gap")
_c("fast no_ones_template.second_pass KC.KC.PLAIN k1 split silu bias_cols mask_cols save_z")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split bias_cols mask_cols accumulate")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split bias_cols mask_cols")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split bias_cols")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split mask_cols accumulate")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split accumulate")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split relu bias_cols")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split sigmoid bias_cols save_act gate_covering")
_c("fast no_ones_template.second_pass KC.KC.PLAIN kN split silu bias_cols mask_cols save_z")
_c("fast no_ones_template.second_pass KC.RC.PLAIN z1 split accumulate")
_c("fast no_ones_template.second_pass KC.RC.PLAIN z1 split")
_c("fast no_ones_template.second_pass KC.RC.PLAIN zN split acc_mixed")
_c("fast no_ones_template.second_pass KC.RC.PLAIN zN split accumulate")
_c("fast no_ones_template.second_pass KC.RC.PLAIN zN split")
_c("fast no_ones_template.second_pass RC.RC.PLAIN z1 split accumulate mvalid<M")
_c("fast no_ones_template.second_pass RC.RC.PLAIN z1 split accumulate")
_c("fast no_ones_template.second_pass RC.RC.PLAIN z1 split")
_c("fast no_ones_template.second_pass RC.RC.PLAIN zN split accumulate mvalid<M")
_c("fast no_ones_template.second_pass RC.RC.PLAIN zN split")
_c("fast no_ones_template.second_pass RC.RC.PLAIN zN split_deferred")
_c("fast ones_template.full_ones RC.RC.PLAIN zN ones_own_rowsum mvalid<M")
_c("fast ones_template.full_ones+plain RC.RC.PLAIN zN ones_own_rowsum mvalid<M")
_c("fast ones_template.full_ones+plain RC.RC.PLAIN zN ones_own_rowsum")
_c("fast ones_template.second_pass RC.RC.PLAIN z1 split ones_own_rowsum")
_c("fast ones_template.second_pass RC.RC.PLAIN zN split ones_own_rowsum mvalid<M")
_c("fast ones_template.second_pass RC.RC.PLAIN zN split ones_own_rowsum")
_c("fast ones_template.second_pass RC.RC.PLAIN zN split_deferred ones_own_rowsum mvalid<M")
_c("fast ones_template.second_pass RC.RC.PLAIN zN split_deferred ones_own_rowsum")
_c("general 16x64.deep.ring KC.KC.PLAIN k1 bias_cols")
_c("general 16x64.deep.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering")
_c("general 16x64.deep.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap")
_c("general 16x64.deep.ring KC.KC.PLAIN k1 split bias_cols")
_c("general 16x64.deep.ring KC.KC.PLAIN k1 split")
_c("general 16x64.deep.ring KC.KC.PLAIN k1 split relu bias_cols")
_c("general 16x64.deep.ring KC.KC.PLAIN kN bias_cols")
_c("general 16x64.deep.ring KC.KC.PLAIN kN split bias_cols")
_c("general 16x64.deep.ring KC.KC.PLAIN kN split")
_c("general 16x64.deep.ring KC.KC.PLAIN kN split relu bias_cols")
_c("general 16x64.deep.ring KC.RC.PLAIN z1 accumulate")
_c("general 16x64.deep.ring KC.RC.PLAIN z1")
_c("general 16x64.deep.ring KC.RC.PLAIN z1 split")
_c("general 16x64.deep.ring RC.RC.PLAIN z1 split accumulate")
_c("general 16x64.deep.ring RC.RC.PLAIN z1 split")
_c("general 16x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum mvalid<M")
_c("general 16x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum")
_c("general 16x64.deep.ring RC.RC.PLAIN z1 split_deferred")
_c("general 16x64.deep.ring RC.RC.PLAIN z1 split_deferred ones_own_rowsum mvalid<M")
_c("general 16x64.deep.ring RC.RC.PLAIN zN split")
_c("general 16x64.deep.ring RC.RC.PLAIN zN split ones_own_rowsum")
_c("general 16x64.deep.ring RC.RC.PLAIN zN split_deferred")
_c("general 16x64.deep.ring RC.RC.PLAIN zN split_deferred ones_own_rowsum")
_c("general 16x64.deep.ring TOKK.TOKK.PLAIN z1 split ones_own_rowsum")
_c("general 16x64.deep.ring TOKK.TOKK.PLAIN z1 split_deferred")
_c("general 16x64.deep.ring TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("general 16x64.deep.ring TOKK.TOKK.PLAIN zN split_deferred")
_c("general 16x64.deep.ring TOKK.TOKK.PLAIN zN split_deferred ones_own_rowsum mvalid<M")
_c("general 16x64.deep.ring_aux KC.RC.PLAIN z1 aux_A")
_c("general 16x64.deep.ring_aux KC.RC.PLAIN z1 split accumulate aux_A")
_c("general 16x64.deep.ring_aux RC.RC.PLAIN z1 split ones_own_rowsum aux_A")
_c("general 16x64.deep.ring_aux TOKK.TOKK.PLAIN z1 split ones_own_rowsum aux_A")
_c("general 16x64.deep.ring_aux TOKK.TOKK.PLAIN zN split ones_own_rowsum aux_A")
_c("general 16x64.shallow.ring KC.KC.PLAIN k1 bias_cols accumulate")
_c("general 16x64.shallow.ring KC.KC.PLAIN k1 bias_cols")
_c("general 16x64.shallow.ring KC.KC.PLAIN k1 bias_cols pre_add")
_c("general 16x64.shallow.ring KC.KC.PLAIN k1")
_c("general 16x64.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering")
_c("general 16x64.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap")
_c("general 16x64.shallow.ring KC.KC.PLAIN kN bias_cols")
_c("general 16x64.shallow.ring KC.RC.PLAIN z1 accumulate")
_c("general 16x64.shallow.ring KC.RC.PLAIN z1")
_c("general 16x64.shallow.ring KC.RC.PLAIN zN accumulate")
_c("general 64x16.deep.ring KC.KC.PLAIN k1 bias_cols")
_c("general 64x16.deep.ring KC.RC.PLAIN z1 accumulate")
_c("general 64x16.deep.ring KC.RC.PLAIN z1")
_c("general 64x16.deep.ring KC.TOKR.TOKJ k1 bias_rows mask_rows")
_c("general 64x16.deep.ring KC.TOKR.TOKJ k1 bias_rows")
_c("general 64x16.deep.ring KC.TOKR.TOKJ k1")
_c("general 64x16.deep.ring KC.TOKR.TOKJ k1 relu bias_rows")
_c("general 64x16.deep.ring KC.TOKR.TOKJ k1 silu bias_rows mask_rows save_z")
_c("general 64x16.deep.ring KC.TOKR.TOKJ kN bias_rows mask_rows")
_c("general 64x16.deep.ring KC.TOKR.TOKJ kN bias_rows")
_c("general 64x16.deep.ring KC.TOKR.TOKJ kN")
_c("general 64x16.deep.ring KC.TOKR.TOKJ kN silu bias_rows mask_rows save_z")
_c("general 64x16.deep.ring RC.RC.PLAIN z1 split accumulate")
_c("general 64x16.deep.ring RC.RC.PLAIN z1 split")
_c("general 64x16.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum")
_c("general 64x16.deep.ring RC.RC.PLAIN z1 split_deferred ones_own_rowsum")
_c("general 64x16.deep.ring RC.RC.PLAIN zN split ones_own_rowsum")
_c("general 64x16.deep.ring RC.TOKR.TOKJ k1 accumulate")
_c("general 64x16.deep.ring RC.TOKR.TOKJ z1 accumulate")
_c("general 64x16.deep.ring TOKK.TOKK.PLAIN z1 split ones_own_rowsum")
_c("general 64x16.deep.ring TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("general 64x16.deep.ring_aux KC.RC.PLAIN z1 accumulate aux_A")
_c("general 64x16.deep.ring_aux KC.RC.PLAIN zN acc_mixed aux_A")
_c("general 64x16.deep.ring_aux KC.RC.PLAIN zN aux_A")
_c("general 64x16.deep.ring_aux RC.RC.PLAIN z1 split ones_own_rowsum aux_A")
_c("general 64x16.deep.ring_aux RC.RC.PLAIN zN split ones_own_rowsum aux_A")
_c("general 64x16.deep.ring_aux RC.TOKR.TOKJ z1 accumulate aux_B")
_c("general 64x16.deep.ring_aux RC.TOKR.TOKJ z1 aux_B")
_c("general 64x16.deep.ring_aux TOKK.TOKK.PLAIN z1 split aux_A")
_c("general 64x16.deep.ring_aux TOKK.TOKK.PLAIN z1 split ones_own_rowsum aux_A")
_c("general 64x16.deep.ring_aux TOKK.TOKK.PLAIN zN split ones_own_rowsum aux_A")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1 bias_cols mask_cols accumulate")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1 bias_cols accumulate")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1 bias_cols pre_add")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1 relu bias_cols")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap")
_c("general 64x16.shallow.ring KC.KC.PLAIN k1 silu bias_cols mask_cols save_z")
_c("general 64x16.shallow.ring KC.KC.PLAIN kN bias_cols mask_cols accumulate")
_c("general 64x16.shallow.ring KC.KC.PLAIN kN bias_cols mask_cols")
_c("general 64x16.shallow.ring KC.KC.PLAIN kN bias_cols")
_c("general 64x16.shallow.ring KC.KC.PLAIN kN")
_c("general 64x16.shallow.ring KC.RC.PLAIN z1 accumulate")
_c("general 64x16.shallow.ring KC.RC.PLAIN z1")
_c("general 64x16.shallow.ring KC.RC.PLAIN zN acc_mixed")
_c("general 64x16.shallow.ring KC.RC.PLAIN zN accumulate")
_c("general 64x16.shallow.ring KC.TOKR.TOKJ k1 bias_rows mask_rows")
_c("general 64x16.shallow.ring KC.TOKR.TOKJ k1 bias_rows")
_c("general 64x16.shallow.ring KC.TOKR.TOKJ k1")
_c("general 64x16.shallow.ring KC.TOKR.TOKJ k1 relu bias_rows")
_c("general 64x16.shallow.ring KC.TOKR.TOKJ k1 silu bias_rows mask_rows save_z")
_c("general 64x16.shallow.ring KC.TOKR.TOKJ kN bias_rows")
_c("general 64x16.shallow.ring KC.TOKR.TOKJ kN relu bias_rows")
_c("general 64x16.shallow.ring RC.TOKR.TOKJ z1 accumulate")
_c("general 64x16.shallow.ring_aux KC.RC.PLAIN z1 accumulate aux_A")
_c("general 64x16.shallow.ring_aux RC.TOKR.TOKJ z1 accumulate aux_B")
_c("general big64x64.plain_template RC.TOKR.TOKJ z1 accumulate aux_B")
_c("general big64x64.plain_template RC.TOKR.TOKJ z1 aux_B")
_c("general big64x64.plain_template RC.TOKR.TOKJ zN acc_mixed aux_B")
_c("general big64x64.plain_template RC.TOKR.TOKJ zN accumulate aux_B")
_c("general big64x64.plain_template RC.TOKR.TOKJ zN accumulate")
_c("general big64x64.plain_template RC.TOKR.TOKJ zN aux_B")
_c("general mid64x64.deep.plain_template RC.TOKR.TOKJ kN disagree aux_B")
_c("general mid64x64.deep.ring KC.KC.PLAIN k1 bias_cols")
_c("general mid64x64.deep.ring KC.KC.PLAIN k1 relu bias_cols")
_c("general mid64x64.deep.ring KC.KC.PLAIN k1 split bias_cols")
_c("general mid64x64.deep.ring KC.KC.PLAIN k1 split")
_c("general mid64x64.deep.ring KC.KC.PLAIN kN split bias_cols")
_c("general mid64x64.deep.ring KC.KC.PLAIN kN split")
_c("general mid64x64.deep.ring KC.KC.PLAIN kN split relu bias_cols")
_c("general mid64x64.deep.ring KC.RC.PLAIN z1 accumulate")
_c("general mid64x64.deep.ring KC.RC.PLAIN z1")
_c("general mid64x64.deep.ring KC.RC.PLAIN z1 split accumulate")
_c("general mid64x64.deep.ring KC.RC.PLAIN z1 split")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN bias_rows mask_rows")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN silu bias_rows mask_rows save_z")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN split bias_rows mask_rows")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN split bias_rows")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN split")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN split relu bias_rows")
_c("general mid64x64.deep.ring KC.TOKR.TOKJ kN split silu bias_rows mask_rows save_z")
_c("general mid64x64.deep.ring RC.RC.PLAIN z1 ones_own_rowsum")
_c("general mid64x64.deep.ring RC.RC.PLAIN z1 split accumulate mvalid<M")
_c("general mid64x64.deep.ring RC.RC.PLAIN z1 split accumulate")
_c("general mid64x64.deep.ring RC.RC.PLAIN z1 split")
_c("general mid64x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum mvalid<M")
_c("general mid64x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum")
_c("general mid64x64.deep.ring RC.TOKR.TOKJ kN split accumulate")
_c("general mid64x64.deep.ring RC.TOKR.TOKJ kN split")
_c("general mid64x64.deep.ring RC.TOKR.TOKJ z1 accumulate")
_c("general mid64x64.deep.ring RC.TOKR.TOKJ z1")
_c("general mid64x64.deep.ring_aux KC.RC.PLAIN z1 accumulate aux_A")
_c("general mid64x64.deep.ring_aux KC.RC.PLAIN z1 aux_A")
_c("general mid64x64.deep.ring_aux KC.RC.PLAIN z1 split accumulate aux_A")
_c("general mid64x64.deep.ring_aux RC.TOKR.TOKJ k1 accumulate aux_B")
_c("general mid64x64.deep.ring_aux RC.TOKR.TOKJ z1 accumulate aux_B")
_c("general mid64x64.deep.ring_aux RC.TOKR.TOKJ z1 aux_B")
_c("general mid64x64.shallow.ring KC.KC.PLAIN k1 bias_cols")
_c("general mid64x64.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap")
_c("general mid64x64.shallow.ring KC.KC.PLAIN kN bias_cols")
_c("general mid64x64.shallow.ring KC.RC.PLAIN z1 accumulate")
_c("general mid64x64.shallow.ring KC.RC.PLAIN z1")
_c("general mid64x64.shallow.ring KC.RC.PLAIN zN acc_mixed")
_c("general mid64x64.shallow.ring KC.RC.PLAIN zN accumulate")
_c("general mid64x64.shallow.ring KC.RC.PLAIN zN")
_c("general mid64x64.shallow.ring RC.TOKR.TOKJ z1 accumulate")
_c("general mid64x64.shallow.ring RC.TOKR.TOKJ z1")
_c("general mid64x64.shallow.ring RC.TOKR.TOKJ zN acc_mixed")
_c("general mid64x64.shallow.ring RC.TOKR.TOKJ zN accumulate")
_c("general mid64x64.shallow.ring RC.TOKR.TOKJ zN")
_c("general mid64x64.shallow.ring_aux KC.RC.PLAIN z1 accumulate aux_A")
_c("general mid64x64.shallow.ring_aux RC.TOKR.TOKJ z1 aux_B")
_c("general mid64x64.shallow.ring_aux RC.TOKR.TOKJ zN acc_mixed aux_B")
_c("general mid64x64.shallow.ring_aux RC.TOKR.TOKJ zN accumulate aux_B")
_c("general mid64x64.shallow.ring_aux RC.TOKR.TOKJ zN aux_B")
_c("general z32x32.deep.ring KC.RC.PLAIN zN accumulate")
_c("general z32x32.deep.ring RC.RC.PLAIN zN")
_c("general z32x32.deep.ring RC.RC.PLAIN zN ones_own_rowsum mvalid<M")
_c("general z32x32.deep.ring RC.RC.PLAIN zN ones_own_rowsum")
_c("general z32x32.deep.ring RC.RC.PLAIN zN split accumulate")
_c("general z32x32.deep.ring RC.RC.PLAIN zN split")
_c("general z32x32.deep.ring RC.RC.PLAIN zN split ones_own_rowsum mvalid<M")
_c("general z32x32.deep.ring RC.RC.PLAIN zN split ones_own_rowsum")
_c("general z32x32.deep.ring RC.RC.PLAIN zN split_deferred")
_c("general z32x32.deep.ring RC.RC.PLAIN zN split_deferred ones_own_rowsum mvalid<M")
_c("general z32x32.deep.ring RC.RC.PLAIN zN split_deferred ones_own_rowsum")
_c("general z32x32.deep.ring RC.TOKR.TOKJ zN acc_mixed")
_c("general z32x32.deep.ring RC.TOKR.TOKJ zN accumulate")
_c("general z32x32.deep.ring RC.TOKR.TOKJ zN")
_c("general z32x32.deep.ring TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("general z32x32.deep.ring TOKK.TOKK.PLAIN zN split_deferred")
_c("general z32x32.deep.ring TOKK.TOKK.PLAIN zN split_deferred ones_own_rowsum mvalid<M")
_c("general z32x32.deep.ring TOKK.TOKK.PLAIN zN split_deferred ones_own_rowsum")
_c("general z32x32.deep.ring_aux KC.RC.PLAIN zN acc_mixed aux_A")
_c("general z32x32.deep.ring_aux KC.RC.PLAIN zN accumulate aux_A")
_c("general z32x32.deep.ring_aux KC.RC.PLAIN zN aux_A")
_c("general z32x32.deep.ring_aux KC.RC.PLAIN zN split acc_mixed aux_A")
_c("general z32x32.deep.ring_aux KC.RC.PLAIN zN split accumulate aux_A")
_c("general z32x32.deep.ring_aux RC.RC.PLAIN zN aux_A")
_c("general z32x32.deep.ring_aux RC.RC.PLAIN zN ones_own_rowsum aux_A")
_c("general z32x32.deep.ring_aux RC.RC.PLAIN zN split ones_own_rowsum aux_A")
_c("general z32x32.deep.ring_aux RC.TOKR.TOKJ zN acc_mixed aux_B")
_c("general z32x32.deep.ring_aux RC.TOKR.TOKJ zN accumulate aux_B")
_c("general z32x32.deep.ring_aux RC.TOKR.TOKJ zN aux_B")
_c("general z32x32.deep.ring_aux TOKK.TOKK.PLAIN zN split aux_A")
_c("general z32x32.deep.ring_aux TOKK.TOKK.PLAIN zN split ones_own_rowsum aux_A")
_c("kslice - KC.KC.PLAIN k1 bias_cols mask_cols accumulate")
_c("kslice - KC.KC.PLAIN k1 bias_cols mask_cols")
_c("kslice - KC.KC.PLAIN k1 bias_cols")
_c("kslice - KC.KC.PLAIN k1")
_c("kslice - KC.KC.PLAIN k1 silu bias_cols mask_cols save_z")
_c("kslice - KC.KC.PLAIN kN bias_cols mask_cols accumulate")
_c("kslice - KC.KC.PLAIN kN bias_cols mask_cols")
_c("kslice - KC.KC.PLAIN kN mask_cols accumulate")
_c("kslice - KC.KC.PLAIN kN accumulate")
_c("kslice - KC.KC.PLAIN kN")
_c("kslice - KC.KC.PLAIN kN relu bias_cols")
_c("kslice - KC.KC.PLAIN kN sigmoid bias_cols save_act gate_covering")
_c("kslice - KC.KC.PLAIN kN silu bias_cols mask_cols save_z")
_c("skinny_n 8waves KC.KC.PLAIN k1 bias_cols")
_c("skinny_n 8waves KC.KC.PLAIN k1")
_c("skinny_n 8waves KC.KC.PLAIN k1 relu bias_cols")
_c("skinny_n 8waves KC.KC.PLAIN kN bias_cols")
_c("skinny_n 8waves KC.KC.PLAIN kN")
_c("skinny_n 8waves KC.KC.PLAIN kN relu bias_cols")
_c("skinny_n 8waves KC.RC.PLAIN z1")
_c("tinyk col4 KC.KC.PLAIN k1 bias_cols mask_cols accumulate")
_c("tinyk col4 KC.KC.PLAIN k1 bias_cols accumulate")
_c("tinyk col4 KC.KC.PLAIN k1 bias_cols pre_add")
_c("tinyk col4 KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering")
_c("tinyk col4 KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap")
_c("tinyk col4 KC.KC.PLAIN k1 silu bias_cols mask_cols save_z")
_c("tinyk simple KC.KC.PLAIN k1 bias_cols")
_c("tinyk simple KC.KC.PLAIN k1")
_c("tinyk simple KC.KC.PLAIN k1 relu bias_cols")
_c("token_dw rb1.cb4 TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("token_dw rb1.cb5 TOKK.TOKK.PLAIN z1 split ones_own_rowsum")
_c("token_dw rb3.cb2 TOKK.TOKK.PLAIN z1 split")
_c("token_dw rb3.cb2 TOKK.TOKK.PLAIN z1 split ones_own_rowsum")
_c("token_dw rb3.cb2 TOKK.TOKK.PLAIN zN split")
_c("token_dw rb3.cb2 TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("token_dw rb3.cb4 TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("token_dw rb3.cb5 TOKK.TOKK.PLAIN z1 split")
_c("token_dw rb3.cb5 TOKK.TOKK.PLAIN zN split")
_c("token_dw rb3.cb5 TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("token_dw rb4.cb2 TOKK.TOKK.PLAIN z1 split")
_c("token_dw rb4.cb2 TOKK.TOKK.PLAIN zN split")
_c("token_dw rb4.cb2 TOKK.TOKK.PLAIN zN split ones_own_rowsum mvalid<M")
_c("token_dw rb4.cb2 TOKK.TOKK.PLAIN zN split ones_own_rowsum")
_c("token_dw rb4.cb4 TOKK.TOKK.PLAIN z1 split ones_own_rowsum")
_c("token_dw rb4.cb5 TOKK.TOKK.PLAIN z1 split")
_c("token_dw rb4.cb5 TOKK.TOKK.PLAIN zN split mvalid<M")
_c("token_dw rb4.cb5 TOKK.TOKK.PLAIN zN split")
_c("token_dw rb4.cb5 TOKK.TOKK.PLAIN zN split ones_own_rowsum mvalid<M")
_c("token_linear rb1.one_problem KC.TOKR.TOKJ k1 bias_rows")
_c("token_linear rb1.one_problem KC.TOKR.TOKJ k1 relu bias_rows")
_c("token_linear rb1.one_problem KC.TOKR.TOKJ kN bias_rows")
_c("token_linear rb1.one_problem KC.TOKR.TOKJ kN relu bias_rows")
_c("token_linear rb1.one_problem RC.TOKR.TOKJ z1 accumulate")
_c("token_linear rb2.one_problem KC.TOKR.TOKJ k1 bias_rows")
_c("token_linear rb2.one_problem KC.TOKR.TOKJ kN relu bias_rows")
_c("token_linear rb2.one_problem RC.TOKR.TOKJ k1 accumulate")
_c("token_linear rb2.one_problem RC.TOKR.TOKJ kN accumulate")
_c("token_linear rb2.one_problem RC.TOKR.TOKJ kN")
_c("token_linear rb2.one_problem RC.TOKR.TOKJ z1")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ k1 bias_rows")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ k1")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ k1 relu bias_rows")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ kN bias_rows")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ kN")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ kN relu bias_rows")
_c("token_linear rb4.batch RC.TOKR.TOKJ zN acc_mixed")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ k1 bias_rows mask_rows")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ k1 bias_rows")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ k1")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ k1 relu bias_rows")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ k1 silu bias_rows mask_rows save_z")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ kN bias_rows mask_rows")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ kN")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ kN relu bias_rows")
_c("token_linear rb4.one_problem KC.TOKR.TOKJ kN silu bias_rows mask_rows save_z")
_c("token_linear rb4.one_problem RC.TOKR.TOKJ z1 accumulate")
_c("token_linear rb4.one_problem RC.TOKR.TOKJ z1")
_c("token_linear rb5.batch RC.TOKR.TOKJ zN acc_mixed")
_c("token_linear rb5.batch RC.TOKR.TOKJ zN accumulate")
_c("token_linear rb5.batch RC.TOKR.TOKJ zN")
_c("token_linear rb5.one_problem RC.TOKR.TOKJ z1 accumulate")
_c("token_linear rb5.one_problem RC.TOKR.TOKJ z1")

# ---- forms no plan emits today, kept on purpose (tests/test_gemm_forms_cpu.py lists them) --------------------------------------------------
# the balanced schedule of the throughput kernel with a non-trivial epilogue
_c("fast no_ones_template.nread1 KC.KC.PLAIN k1 balanced sigmoid bias_cols save_act gate_gap")
_c("fast no_ones_template.full_nread2+ KC.KC.PLAIN kN balanced relu bias_cols mask_cols accumulate pre_add save_z")
# a NULL A segment in each family that accepts several k-segments
_c("general 64x16.deep.ring KC.KC.PLAIN kN relu bias_cols null_A")
_c("general mid64x64.deep.ring KC.KC.PLAIN kN split bias_cols accumulate null_A")
_c("kslice - KC.KC.PLAIN kN relu bias_cols null_A")
_c("skinny_n 8waves KC.KC.PLAIN kN bias_cols null_A")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ kN relu bias_rows null_A")
_c("fast no_ones_template.nread0 KC.KC.PLAIN kN bias_cols null_A")
# the acc_in_tile start of the throughput kernel (un-split, accumulate, nothing else) and its nearest neighbour that must not take it
_c("fast no_ones_template.acc_in_tile KC.KC.PLAIN k1 accumulate")
_c("fast no_ones_template.nread1 KC.KC.PLAIN k1 bias_cols accumulate")
# a NULL gating pointer, the 4-wave instantiation of skinny_n, the full path of ft_epilogue with two arrays read
_c("fast no_ones_template.nread1 KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap_null")
_c("general 64x16.deep.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering_null")
_c("skinny_n 4waves KC.KC.PLAIN k1 relu bias_cols")
_c("fast no_ones_template.full_nread2+ KC.KC.PLAIN k1 sigmoid bias_cols accumulate save_act gate_covering")
# the nearest neighbours of two shortcuts, one per term of the predicate that guards it: ft_epilogue's `plain` (csrc/gemm_fast_common.h) ...
_c("fast no_ones_template.nread0 KC.KC.PLAIN k1 relu")
_c("fast no_ones_template.nread0 KC.KC.PLAIN k1 silu")
_c("fast no_ones_template.nread0 KC.KC.PLAIN k1 bias_cols")
_c("fast no_ones_template.nread1 KC.KC.PLAIN k1 pre_add")
_c("fast no_ones_template.nread0 KC.KC.PLAIN k1 save_z")
_c("fast no_ones_template.nread0 KC.KC.PLAIN k1 save_act")
_c("fast no_ones_template.nread1 KC.KC.PLAIN k1 gate_covering")
_c("fast no_ones_template.nread0 KC.KC.PLAIN k1 mask_cols")
_c("fast no_ones_template.nread0 KC.KC.PLAIN k1 mask_rows")
_c("fast no_ones_template.nread1 KC.RC.PLAIN z1 accumulate mvalid<M")
# ... and gemm_tinyk_kernel's `simple` (csrc/gemm_skinny.hip), with everything `simple` keeps for itself
_c("tinyk simple KC.KC.PLAIN k1 sigmoid bias_cols save_z save_act")
_c("tinyk col4 KC.KC.PLAIN k1 pre_add")
_c("tinyk col4 KC.KC.PLAIN k1 gate_gap")
_c("tinyk col4 KC.KC.PLAIN k1 accumulate")
_c("tinyk col4 KC.KC.PLAIN k1 mask_cols")
_c("tinyk col4 KC.KC.PLAIN k1 bias_rows")
# dims_in_use = 0 and = the full width, on both axes (a word that starts with @ is an option of the case that is no property of the form)
_c("general 64x16.deep.ring KC.KC.PLAIN k1 relu bias_cols mask_cols @dims0")
_c("general 64x16.deep.ring KC.KC.PLAIN k1 relu bias_cols mask_cols accumulate @dims_full")
_c("general 64x16.deep.ring KC.TOKR.TOKJ kN relu bias_rows mask_rows @dims0")
_c("token_linear rb3.one_problem KC.TOKR.TOKJ kN relu bias_rows mask_rows @dims_full")
_c("fast no_ones_template.nread0 KC.KC.PLAIN kN bias_cols mask_cols @dims_full")
# the 256-thread 64 x 64 template on a dense binding (a product too thin for the throughput kernel)
_c("general big64x64.plain_template KC.KC.PLAIN k1 relu bias_cols mask_cols")

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
