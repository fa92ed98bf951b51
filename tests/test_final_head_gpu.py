"""NASREC_OP_FINAL_FUSED with a head Linear (include/nasrec_hip.h, csrc/final_bodies.h): the last dense Linear y = pre + x W^T + b and its
input gradient dx (+)= dy W computed by the workgroup that sums the sample's logit.

The headed operator — as its stand-alone kernel and as a worklist item — must leave, bit for bit, what the three launches it replaces
leave on the same buffers: the Linear (a GEMM launch), the final-logit operator without a head, the input gradient (a zmode GEMM launch);
behind each, the FINAL_BWD with dseg_done that writes the loss and d logits.  Compared: y, logits, d logits, d y, dx, loss.

Both are also held to an fp64 restatement of the expressions; the headed operator's error may not exceed the three launches' (they are
bit-equal, so this only guards the comparison: two runs that both wrote nothing would be "equal").

Shapes: B in {1, 5, 256} x head K in {1, 13, 16, 32} x head N in {1, 17, 128, 256} x {pre_add, none} x {sparse segment, none} x {dx
stored, dx accumulated onto a pre-filled buffer}; row strides longer than the rows everywhere."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import schedule as S

pytestmark = pytest.mark.gpu
NS = 7 * 16  # width of the sparse final segment


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _launch(lib, d):
    L.check(lib.nasrec_launch(None, C.addressof(d)))


def _as_item(d):
    """`d` as the only item of a worklist launch (schedule.pack's layout)"""
    w = L.WorklistDesc()
    w.kind, w.n = L.OP_WORKLIST, 1
    it = w.item[0]
    it.kind, it.part, it.off = d.kind, L.WL_WHOLE, 0
    b = S.item_bytes(S.Node(d))
    assert b is not None
    C.memmove(C.addressof(w) + L.WorklistDesc.blob.offset, b, len(b))
    return w


class Case:
    def __init__(self, B, K, N, pre, sparse, acc, seed):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        self.B, self.K, self.N, self.pre, self.sparse, self.acc = B, K, N, pre, sparse, acc
        self.ldx, self.ldy, self.lddx, self.lds = K + 3, N + 5, K + 2, NS + 16
        KF = N + (NS if sparse else 0)
        h = dict(x=r(B, self.ldx), W=r(N, K) * 0.3, b=r(N), pre=r(B, self.ldy), s=r(B, self.lds), w=r(KF) * 0.05, bias=r(1),
                 label=(torch.rand(B, generator=g) < 0.25).float(), dx0=r(B, self.lddx))
        self.h = h
        self.dev = {k: v.cuda() for k, v in h.items()}
        nan = lambda *s: torch.full(s, float("nan"), device="cuda")
        self.out0 = dict(y=nan(B, self.ldy), logits=nan(B), dlogits=nan(B), dy=nan(B, self.ldy), ds=nan(B, self.lds),
                         dx=self.dev["dx0"].clone() if acc else nan(B, self.lddx), loss=nan(1), dw=nan(KF), dbias=nan(1))
        self.out = {k: v.clone() for k, v in self.out0.items()}

    def reset(self):
        for k, v in self.out.items():
            v.copy_(self.out0[k])

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.out.items()}

    # ---- descriptors ----
    def final(self, kind):
        d, o = self.dev, self.out
        f = L.FinalDesc()
        f.kind, f.B, f.nseg = kind, self.B, 2 if self.sparse else 1
        f.w, f.bias, f.logits, f.y, f.grad_scale = d["w"].data_ptr(), d["bias"].data_ptr(), o["logits"].data_ptr(), d["label"].data_ptr(), 1.0 / self.B
        f.seg[0], f.dseg[0], f.width[0], f.ld[0], f.off[0] = o["y"].data_ptr(), o["dy"].data_ptr(), self.N, self.ldy, 0
        if self.sparse:
            f.seg[1], f.dseg[1], f.width[1], f.ld[1], f.off[1] = d["s"].data_ptr(), o["ds"].data_ptr(), NS, self.lds, self.N
        if kind == L.OP_FINAL_BWD:  # the part that needs every sample's logit
            f.dseg_done = 1
            f.loss, f.dlogits_out, f.dw, f.dbias = o["loss"].data_ptr(), o["dlogits"].data_ptr(), o["dw"].data_ptr(), o["dbias"].data_ptr()
        return f

    def headed(self):
        d, o = self.dev, self.out
        f = self.final(L.OP_FINAL_FUSED)
        f.head_x, f.head_w, f.head_bias, f.head_y, f.head_dx = d["x"].data_ptr(), d["W"].data_ptr(), d["b"].data_ptr(), o["y"].data_ptr(), o["dx"].data_ptr()
        f.head_pre = d["pre"].data_ptr() if self.pre else None
        f.head_K, f.head_N, f.head_ldx, f.head_ldw, f.head_ldy, f.head_lddx = self.K, self.N, self.ldx, self.K, self.ldy, self.lddx
        f.head_dx_accumulate, f.head_seg = int(self.acc), 0
        return f

    def linear(self):
        d, o = self.dev, self.out
        g = L.GemmDesc()
        g.kind, g.amode, g.bmode, g.cmode, g.nseg, g.dims_in_use = L.OP_GEMM, L.AM_KC, L.AM_KC, L.CM_PLAIN, 1, -1
        g.bias, g.pre_add = d["b"].data_ptr(), (d["pre"].data_ptr() if self.pre else None)
        s = g.seg[0]
        s.A, s.B, s.C, s.M, s.N, s.K, s.lda, s.ldb, s.ldc = d["x"].data_ptr(), d["W"].data_ptr(), o["y"].data_ptr(), self.B, self.N, self.K, self.ldx, self.K, self.ldy
        return g

    def input_gradient(self):
        d, o = self.dev, self.out
        g = L.GemmDesc()
        g.kind, g.amode, g.bmode, g.cmode, g.nseg, g.zmode, g.dims_in_use = L.OP_GEMM, L.AM_KC, L.AM_RC, L.CM_PLAIN, 1, 1, -1
        s = g.seg[0]
        s.A, s.B, s.C, s.M, s.N, s.K, s.lda, s.ldb, s.ldc = o["dy"].data_ptr(), d["W"].data_ptr(), o["dx"].data_ptr(), self.B, self.K, self.N, self.ldy, self.K, self.lddx
        s.accumulate = int(self.acc)
        return g

    # ---- fp64 ----
    def fp64(self):
        h = {k: v.double().numpy() for k, v in self.h.items()}
        B, K, N = self.B, self.K, self.N
        y = h["x"][:, :K] @ h["W"].T + h["b"] + (h["pre"][:, :N] if self.pre else 0.0)
        z = y @ h["w"][:N] + h["bias"][0] + (h["s"][:, :NS] @ h["w"][N:] if self.sparse else 0.0)
        dl = (1.0 / (1.0 + np.exp(-z)) - h["label"]) / B
        dy = dl[:, None] * h["w"][None, :N]
        dx = dy @ h["W"] + (h["dx0"][:, :K] if self.acc else 0.0)
        loss = np.mean(np.maximum(z, 0) - z * h["label"] + np.log1p(np.exp(-np.abs(z))))
        return dict(y=y, logits=z, dlogits=dl, dy=dy, dx=dx, loss=np.array([loss]))

    def views(self, snap):
        N, K = self.N, self.K
        return dict(y=snap["y"][:, :N], logits=snap["logits"], dlogits=snap["dlogits"], dy=snap["dy"][:, :N], dx=snap["dx"][:, :K], loss=snap["loss"])


COMBOS = list(itertools.product((1, 13, 16, 32), (1, 17, 128, 256), (False, True), (False, True), (False, True)))


@pytest.mark.parametrize("as_item", [False, True], ids=["stand_alone", "worklist_item"])
@pytest.mark.parametrize("B", [1, 5, 256])
def test_headed_final_equals_the_three_launches_it_replaces(lib, B, as_item):
    for n, (K, N, pre, sparse, acc) in enumerate(COMBOS):
        c = Case(B, K, N, pre, sparse, acc, seed=1000 * B + n)
        what = "B=%d K=%d N=%d pre=%d sparse=%d acc=%d" % (B, K, N, pre, sparse, acc)
        rest = c.final(L.OP_FINAL_BWD)
        for d in (c.linear(), c.final(L.OP_FINAL_FUSED), c.input_gradient(), rest):
            _launch(lib, d)
        want = c.snapshot()
        c.reset()
        hd = c.headed()
        _launch(lib, _as_item(hd) if as_item else hd)
        _launch(lib, rest)
        got = c.snapshot()
        for k in got:  # whole buffers: the padding columns of every row and the NaN fill included
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), "%s: %s differs" % (what, k)
        ref, gv, wv = c.fp64(), c.views(got), c.views(want)
        for k, r in ref.items():
            eg = np.max(np.abs(gv[k].double().cpu().numpy() - r))
            ew = np.max(np.abs(wv[k].double().cpu().numpy() - r))
            scale = max(np.max(np.abs(r)), 1e-30)
            assert np.isfinite(eg) and eg <= ew, "%s: %s headed error %.3g > unfused %.3g" % (what, k, eg, ew)
            # fp32 sums of n <= 256 + 112 terms: rounding errors of ~sqrt(n) 2^-24 = 1e-6 of the largest value; one term dropped or
            # doubled is 1e-2 and more.  (Guards the reference: the two runs above could agree on a wrong result.)
            assert ew <= 1e-5 * scale + 1e-7, "%s: %s unfused error %.3g against fp64 (scale %.3g)" % (what, k, ew, scale)


def test_a_headed_operator_without_dx_leaves_the_forward_half(lib):
    c = Case(5, 16, 128, True, True, False, seed=7)
    for d in (c.linear(), c.final(L.OP_FINAL_FUSED)):
        _launch(lib, d)
    want = c.snapshot()
    c.reset()
    hd = c.headed()
    hd.head_dx = None
    _launch(lib, hd)
    got = c.snapshot()
    for k in got:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    assert not torch.isnan(got["y"][:, :128]).any() and not torch.isnan(got["logits"]).any()


def test_the_launcher_refuses_a_head_it_has_no_body_for(lib):
    c = Case(5, 16, 128, False, True, False, seed=8)
    for field, value in (("head_K", 33), ("head_N", 257), ("head_seg", 1), ("head_ldy", 128)):
        hd = c.headed()
        setattr(hd, field, value)
        assert lib.nasrec_launch(None, C.addressof(hd)) != 0, field
    torch.cuda.synchronize()
