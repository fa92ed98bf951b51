"""Chained token-axis input gradients (item part NASREC_WL_CHAIN, csrc/worklist_body.h wl_token_dx_chain) on the GPU: several products
that add into the same outputs, run as ONE worklist item.  Every member is a wl_cases.gemm_case descriptor (binding RC / TOKR / TOKJ,
zmode, three problems as in the batch-256 step; two in the chain of three, which NASREC_MAX_SEGS = 8 problems bound) — NaN where an output must be overwritten, sentinels in guard rows, weights with odd
leading dimensions and pointers — whose outputs are pointed at the first member's; the chained descriptor is what the scheduler itself
merges (schedule._merged_chain).  Every output buffer is compared in full, bit for bit, against

  a. the members launched one after another as stand-alone kernels,
  b. the members as plain token-dx items in consecutive worklist launches,

and against fp64 (wl_cases.close), in the kernel-argument form and in the device-resident form of the launch.

Shapes: 5 samples (N = 80) — with 4 to 7 row blocks per sample more units than one workgroup's four waves, and a last workgroup that is
not full; row counts 26, 17, 1 and 64 (a row block with one live row, exact blocks); member depths (32, 39) a partial last step, (8, 64),
(1, 16), (64, 64) the register-heaviest, and a chain of three; member 0 overwriting and accumulating; the ReLU mask operand on neither,
one and both members; dead problems (A = NULL) in member 0 (overwriting: zeros, then the sum) and in member 1."""
import ctypes as C

import pytest
import torch

import wl_cases as W
from nasrec_amd import _lib as L
from nasrec_amd import schedule as S

pytestmark = pytest.mark.gpu
RC, TOKR, TOKJ = L.AM_RC, L.AM_TOKR, L.CM_TOKJ
NB = 5  # samples

# name -> (rows of the three problems, depth per member, accumulate of member 0 per problem, mask operand per member, dead (member, problem))
CASES = {
    "k32_k39_overwrites": ((26, 17, 1), (32, 39), (0, 0, 0), (0, 0), ()),
    "k8_k64_accumulates_mask_on_second": ((26, 1, 64), (8, 64), (1, 1, 1), (0, 1), ()),
    "k1_k16_mask_on_first": ((17, 64, 1), (1, 16), (0, 1, 0), (1, 0), ()),
    "k64_k64_mask_on_both": ((64, 17, 1), (64, 64), (1, 0, 1), (1, 1), ()),
    "k32_k39_dead_problems": ((26, 1, 64), (32, 39), (0, 0, 1), (0, 1), ((0, 1), (1, 0), (0, 2))),
    "chain_of_three_k32_k39_k64": ((17, 64), (32, 39, 64), (0, 1), (0, 1, 0), ()),  # (two problems: 3 x 2 <= NASREC_MAX_SEGS)
}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _run(lib, d):
    L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()


def _worklist(kind, part, by):
    w = L.WorklistDesc()
    w.kind, w.n = L.OP_WORKLIST, 1
    w.item[0].kind, w.item[0].part, w.item[0].off = kind, part, 0
    C.memmove(C.addressof(w) + L.WorklistDesc.blob.offset, by, len(by))
    return w


def _host(ctx, ptr, count):
    """`count` floats at device address `ptr`, which lies in one of the case's tensors"""
    for t in ctx.keep:
        off = ptr - t.data_ptr()
        if 0 <= off < t.numel() * 4:
            return t.view(-1)[off // 4: off // 4 + count].cpu().double()
    raise AssertionError("pointer outside the case's tensors")


def _product(ctx, s):
    """fp64 sum_k A(r, k) B(j, k) of one problem from its descriptor fields: A(r, k) = A[k lda + r], B(16 b + e, k) = B[b ldb + 16 k + e]"""
    if not s.A:
        return torch.zeros(s.M, s.N, dtype=torch.float64)
    a = torch.stack([_host(ctx, s.A + 4 * k * s.lda, s.M) for k in range(s.K)], 1)  # [M, K]
    rows = []
    for b in range(s.N // 16):
        y = _host(ctx, s.B + 4 * b * s.ldb, 16 * s.K).view(s.K, 16)
        if s.Baux:
            y = y * (_host(ctx, s.Baux + 4 * b * s.ldb, 16 * s.K).view(s.K, 16) > 0).double()
        rows.append(y.t())  # [16, K]
    return a @ torch.cat(rows, 0).t()


class Live:
    """a case on the device: the members, the chained descriptor, and the outputs of references (a) and (b), computed once"""

    def __init__(self, lib, name):
        Ms, Ks, acc0, masks, dead = CASES[name]
        self.ctx = W.Ctx("cuda", 40 + (W.hash_name(name) & 0xfff))
        self.members = []
        for m, K in enumerate(Ks):
            probs = [dict(M=M, N=NB * 16, K=K, acc=(acc0[q] if m == 0 else 1), bmask=bool(masks[m]), dead=(m, q) in dead, extra_a=2 * q + 1 + m,
                          lead_a=1 + q, extra_b=m) for q, M in enumerate(Ms)]
            self.members.append(W.gemm_case(self.ctx, RC, TOKR, TOKJ, probs, 1))
        first = self.members[0]
        for b in self.members[1:]:  # every later member adds onto the first member's outputs
            for q in range(len(Ms)):
                b.desc.seg[q].C, b.desc.seg[q].ldc = first.desc.seg[q].C, first.desc.seg[q].ldc
        self.outs = first.outs
        self.init = {k: v.clone() for k, v in self.outs.items()}
        self.chain = first.desc
        for b in self.members[1:]:
            self.chain = S._merged_chain(self.chain, b.desc)
            assert self.chain is not None, L.load().nasrec_last_error()
        assert self.chain._chain == len(Ms) and self.chain.nseg == len(Ms) * len(Ks)
        # fp64: the sum of the members' products (+ what the buffer held where member 0 accumulates)
        self.ref = []
        for q, M in enumerate(Ms):
            r = sum(_product(self.ctx, b.desc.seg[q]) for b in self.members)
            if acc0[q]:
                r = r + self.logical(self.init["C%d" % q], M).double().cpu()
            self.ref.append(r)
        for b in self.members:  # (a) stand-alone kernels, one after another
            _run(lib, b.desc)
        self.alone = self.snapshot()
        self.reset()
        for b in self.members:  # (b) plain token-dx items, one launch each
            node = S.Node(b.desc)
            assert node.item is not None and node.item[1].body == L.WL_BODY_TOKEN_DX
            _run(lib, _worklist(b.desc.kind, L.WL_WHOLE, node.item[0]))
        self.items = self.snapshot()

    @staticmethod
    def logical(t, M):
        return t[:, :M, :].permute(1, 0, 2).reshape(M, -1)

    def reset(self):
        for k, v in self.outs.items():
            v.copy_(self.init[k])

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.outs.items()}

    def check_fp64(self, got):
        for q, r in enumerate(self.ref):
            M = r.shape[0]
            t = got["C%d" % q]
            W.close(self.logical(t, M), r)
            assert bool((t[:, M:, :] == W.SENTINEL).all()), "guard rows of C%d were written" % q


_LIVE = {}


def live(lib, name):
    if name not in _LIVE:
        _LIVE[name] = Live(lib, name)
    return _LIVE[name]


def _same(got, want, what):
    for k in want:
        assert torch.equal(got[k], want[k]), "%s: %s differs" % (what, k)  # (NaN nowhere: every NaN of the initial buffers is overwritten)


@pytest.mark.parametrize("resident", [False, True], ids=["kernarg", "resident"])
@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_chained_item_equals_its_members_run_in_turn_which_equal_fp64(lib, name, resident):
    lv = live(lib, name)
    assert not any(bool(torch.isnan(v).any()) for v in lv.alone.values())
    lv.check_fp64(lv.alone)
    _same(lv.items, lv.alone, "token-dx items against the stand-alone kernels")
    node = S.Node(lv.chain, "chain")
    by, g = node.item
    plain = S.Node(lv.members[0].desc).item[1]
    assert g.body == L.WL_BODY_TOKEN_DX_CHAIN and g.nblk == plain.nblk and g.geom[0] == plain.geom[0] and g.geom[1] == len(CASES[name][0])
    assert g.nblk > 1 and (NB * g.geom[0]) % 4 != 0  # more than one workgroup, the last one partial
    lv.reset()
    w = _worklist(lv.chain.kind, L.WL_CHAIN, by)
    if resident:
        buf = torch.empty(C.sizeof(L.WorklistDesc), dtype=torch.uint8, device="cuda")
        dv = L.WorklistDevDesc()
        L.check(lib.nasrec_worklist_prepare(C.addressof(w), buf.data_ptr(), C.addressof(dv)))
        _run(lib, dv)
    else:
        _run(lib, w)
    got = lv.snapshot()
    _same(got, lv.alone, "chained item against the stand-alone kernels")  # (a)
    _same(got, lv.items, "chained item against the token-dx items")       # (b)
    lv.check_fp64(got)
