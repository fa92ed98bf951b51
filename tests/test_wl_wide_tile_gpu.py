"""The wide form of the worklist's 32 x 32 GEMM tile (csrc/worklist_body.h WL_WIDE: 64 x 64 outputs over 32-deep staged tiles, two per
64-deep k unit) on the GPU.  Descriptors come from wl_cases.gemm_case — NaN where an output must be overwritten, sentinels in guard rows
and columns, operands with odd leading dimensions and pointers — and the wide tile is forced with nasrec_worklist_set_wide_min(1).
Every case is compared three ways, every output buffer in full (split-K workspaces, save_z and row sums included):

  a. bit for bit against the same item(s) with the wide tile switched off (the 32 x 32 x 64 tile),
  b. bit for bit against the stand-alone launch of the descriptor (the general kernel, plus its second pass at equal split-K),
  c. against fp64 with wl_cases.close (the tolerance of the case table).

Shapes are the smallest that still reach WL_T32x32 (64 x 64 tiles x S >= 128) and stay below the stand-alone launcher's 1024-workgroup
configuration; each covers a tile row and a tile column that hold ONE element.  The k extents meet every way a 64-deep unit can end: K = 32
(the unit's second half is empty), K = 100 (the unit ends inside its second half), K = 200, segments 13 + 100 + 64 around a NULL one, more
splits than units (empty splits write zero slabs) and S = 3 over the 4 units of K = 200 (split boundaries off the multiples of the split).
"""
import ctypes as C

import pytest
import torch

import wl_cases as W
from nasrec_amd import _lib as L
from nasrec_amd import plan as P
from nasrec_amd import schedule as S

pytestmark = pytest.mark.gpu
WIDE = 32  # bit 5 of geom[2]
KC, RC, TOKR, TOKK, PLAIN, TOKJ = L.AM_KC, L.AM_RC, L.AM_TOKR, L.AM_TOKK, L.CM_PLAIN, L.CM_TOKJ
PART_NAME = {L.WL_WHOLE: "whole", L.WL_MAIN: "main", L.WL_EPI: "epi"}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _with_save_z(b):
    """the pre-activation through desc.save_z: a buffer laid out like C (same offsets), NaN where the operator writes, sentinel elsewhere"""
    out = b.outs["C0"]
    z = torch.where(torch.isnan(out), out, torch.full_like(out, W.SENTINEL))
    b.ctx.keep.append(z)
    b.desc.save_z = z.data_ptr()
    b.outs["save_z"] = z
    return b


def _relu_out_is_relu_of_save_z(got):
    z, c = got["save_z"].cpu(), got["C0"].cpu()
    inside = z != W.SENTINEL
    assert bool(inside.any()) and not bool(torch.isnan(z).any()) and torch.equal(c[inside], z[inside].clamp_min(0))


# name -> (builder, extra check on the outputs or None)
CASES = {
    # x W^T (KC / KC / PLAIN), unsplit: 9 x 15 = 135 tiles, row 513 and column 897 alone in their tiles; 20 k-steps (past the dense body)
    "kckc_513x897_k100_200_bias_relu_save_z": (lambda c: _with_save_z(W.gemm_case(
        c, KC, KC, PLAIN, [dict(M=513, N=897, K=[100, 200], extra_a={0: 3, 1: 0}, lead_b={0: 1, 1: 0})], 0, bias=True, act=L.ACT_RELU)),
        _relu_out_is_relu_of_save_z),
    "kckc_513x897_k32_mvalid_beta": (lambda c: W.gemm_case(c, KC, KC, PLAIN, [dict(M=513, N=897, K=[32], Mvalid=450, extra_a={0: 1})], 0, beta=1, dims=500), None),
    # dy W (KC / RC / PLAIN): S = 11 over the 4 units of K = 200 — seven splits are empty; 3 x 4 x 11 = 132 tiles
    "kcrc_s11_129x193_k200": (lambda c: W.gemm_case(c, KC, RC, PLAIN, [dict(M=129, N=193, K=[200], extra_a={0: 5}, extra_b=2)], 0, splitk=11, bias=True), None),
    # segments 13 + 100 + NULL + 64: units 1 + 2 + 1 = 4 over S = 11
    "kcrc_s11_129x193_k13_100_dead7_64": (lambda c: W.gemm_case(
        c, KC, RC, PLAIN, [dict(M=129, N=193, K=[13, 100, 7, 64], dead_segs=(2,), extra_b=3)], 0, splitk=11, beta=1), None),
    # dy^T x (RC / RC / PLAIN) with the bias gradient as a column of ones and a row prefix: S = 3 over 4 units -> [0, 1) [1, 2) [2, 4); 8 x 7 x 3 = 168
    "rcrc_s3_450x391_k200_ones_mvalid": (lambda c: W.gemm_case(c, RC, RC, PLAIN, [dict(M=450, N=390 + 1, K=[200], ones=1, Mvalid=301, extra_a={0: 2}, extra_b=1)], 0, splitk=3), None),
    "rcrc_513x897_k100": (lambda c: W.gemm_case(c, RC, RC, PLAIN, [dict(M=513, N=896 + 1, K=[100], ones=1)], 0), None),
    # token-axis W x (KC / TOKR / TOKJ): 513 rows of W against 57 samples, bias on rows
    "tok_fwd_513x912_k13_100_64": (lambda c: W.gemm_case(
        c, KC, TOKR, TOKJ, [dict(M=513, N=57 * 16, K=[13, 100, 64], extra_b=3)], 0, bias=True, bias_on_rows=1, act=L.ACT_RELU, dims=300, mask_on_rows=1), None),
    # token-axis W^T dy (RC / TOKR / TOKJ), split
    "tok_dx_s3_450x400_k200": (lambda c: W.gemm_case(c, RC, TOKR, TOKJ, [dict(M=449, N=25 * 16, K=[200], extra_a={0: 7})], 0, splitk=3), None),
    # token-axis dW (TOKK / TOKK / PLAIN; k = 16 samples x ... : K a multiple of 16), ones column
    "tok_dw_s11_129x193_k208": (lambda c: W.gemm_case(c, TOKK, TOKK, PLAIN, [dict(M=129, N=192 + 1, K=208, ones=1, Mvalid=100, acc=1)], 1, splitk=11), None),
    # zmode, problems of unequal size: (2 x 3 + 3 x 4 + 2 x 1) x 7 = 140 tiles, 2 units each against S = 7
    "zmode_s7_unequal_k100": (lambda c: W.gemm_case(c, KC, RC, PLAIN, [dict(M=130, N=70, K=100, acc=1, extra_a=3), dict(M=130, N=200, K=100, acc=0, Mvalid=77),
                                                                        dict(M=65, N=64, K=100, acc=1, extra_b=5)], 1, splitk=7), None),
    # zmode unsplit, eight problems: 5 x 25 + 6 + 2 + 12 = 145 tiles
    "zmode_eight_unsplit_k45": (lambda c: W.gemm_case(c, RC, RC, PLAIN, [dict(M=300, N=300 + 1, K=45, ones=1, acc=q % 2, Mvalid=300 - 7 * (q % 3)) for q in range(5)]
                                                       + [dict(M=130, N=70 + 1, K=45, ones=1, acc=1), dict(M=65, N=64 + 1, K=45, ones=1), dict(M=130, N=200 + 1, K=45, ones=1, acc=1)], 1),
                                None),
}


def _run(lib, d):
    L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()


def _item(b, part):
    by = S.item_bytes(S.Node(b.desc, PART_NAME[part]))
    assert by is not None
    return (b.desc.kind, part, by)


def _worklist(entries):
    w = L.WorklistDesc()
    w.kind, w.n = L.OP_WORKLIST, len(entries)
    off = 0
    for k, (kind, part, by) in enumerate(entries):
        it = w.item[k]
        it.kind, it.part, it.off = kind, part, off
        C.memmove(C.addressof(w) + L.WorklistDesc.blob.offset + off, by, len(by))
        off += (len(by) + 15) & ~15
    assert off <= L.WL_BLOB_BYTES
    return w


def _geom(lib, b, part):
    g = L.WlGeometry()
    by = _item(b, part)[2]
    L.check(lib.nasrec_worklist_item_geometry(b.desc.kind, part, by, len(by), C.byref(g)))
    return g


class Live:
    """a case on the device: buffers as built, after the stand-alone launch (b) and after the item launches with the wide tile off (a) —
    each computed once and left unchanged"""

    def __init__(self, lib, name):
        self.name = name
        self.b = CASES[name][0](W.Ctx("cuda", 20 + (W.hash_name(name) & 0xfff)))
        self.b.desc._wl_force = True  # (routing policy aside: the launcher's geometry accepts it)
        assert P.gemm_route(self.b.desc)[0] == L.GEMM_ROUTE_GENERAL  # (the items promise the bits of the general template)
        self.init = {k: v.clone() for k, v in self.b.outs.items()}
        _run(lib, self.b.desc)
        self.alone = self.snapshot()
        self.reset()
        prev = lib.nasrec_worklist_set_wide_min(0)
        try:
            for part in self.b.parts:
                g = _geom(lib, self.b, part)
                assert part == L.WL_EPI or (g.geom[2] & 3 == W.WL_T32x32 and not g.geom[2] & WIDE), (name, list(g.geom))
                _run(lib, _worklist([_item(self.b, part)]))
        finally:
            lib.nasrec_worklist_set_wide_min(prev)
        self.narrow = self.snapshot()

    def reset(self):
        for k, v in self.b.outs.items():
            v.copy_(self.init[k])

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.b.outs.items()}


_LIVE = {}


def live(lib, name):
    if name not in _LIVE:
        _LIVE[name] = Live(lib, name)
    return _LIVE[name]


def _same(got, want, what):
    for k in want:
        assert torch.equal(got[k], want[k]), "%s: %s differs" % (what, k)  # (NaN nowhere: every NaN of the initial buffers is overwritten)


@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_wide_item_equals_the_32x32_item_and_the_stand_alone_launch_which_equals_fp64(lib, name):
    lv = live(lib, name)
    lv.b.check(lv.alone)  # (c) the stand-alone launch against fp64 ...
    if CASES[name][1]:
        CASES[name][1](lv.alone)
    assert not any(bool(torch.isnan(v).any()) for v in lv.alone.values())
    lv.reset()
    prev = lib.nasrec_worklist_set_wide_min(1)
    try:
        for part in lv.b.parts:
            g = _geom(lib, lv.b, part)
            if part != L.WL_EPI:
                assert g.geom[2] & WIDE and g.geom[2] & 3 == W.WL_T32x32 and g.body == L.WL_BODY_TILE, (name, list(g.geom))
                assert g.nblk >= 128 and g.nblk < 1024
            _run(lib, _worklist([_item(lv.b, part)]))
    finally:
        lib.nasrec_worklist_set_wide_min(prev)
    wide = lv.snapshot()
    _same(wide, lv.narrow, "wide item against the 32 x 32 item")   # (a)
    _same(wide, lv.alone, "wide item against the stand-alone launch")  # (b)
    lv.b.check(wide)  # (c) ... and the wide item itself


def test_a_wide_item_beside_a_transformer_backward_in_one_launch(lib):
    """the instantiation that carries the Transformer backward (the 39.5 KB LDS buffer): both items of one launch against their stand-alone
    launches, in both orders (an even and an odd slot of the packed item table)"""
    mha = W.BY_NAME["mha_bwd_n16_d-1_b5_slabs_shared"].build("cuda")
    for d in mha.setup:
        _run(lib, d)
    mha_init = {k: v.clone() for k, v in mha.outs.items()}
    _run(lib, mha.desc)
    torch.cuda.synchronize()
    mha_alone = {k: v.clone() for k, v in mha.outs.items()}
    mha.check(mha_alone)
    lv = live(lib, "kckc_513x897_k100_200_bias_relu_save_z")
    mha_item = (mha.desc.kind, L.WL_WHOLE, S.item_bytes(S.Node(mha.desc)))
    for order in (0, 1):
        lv.reset()
        for k, v in mha.outs.items():
            v.copy_(mha_init[k])
        prev = lib.nasrec_worklist_set_wide_min(1)
        try:
            entries = [mha_item, _item(lv.b, L.WL_WHOLE)][::-1 if order else 1]
            w = _worklist(entries)
            buf = torch.empty(C.sizeof(L.WorklistDesc), dtype=torch.uint8, device="cuda")
            dv = L.WorklistDevDesc()
            L.check(lib.nasrec_worklist_prepare(C.addressof(w), buf.data_ptr(), C.addressof(dv)))
            up = L.WorklistDesc.from_buffer_copy(buf.cpu().numpy().tobytes())
            assert dv.big == 1 and up.item[1 - order].geom[2] & WIDE
            _run(lib, dv if order else w)  # (resident and by value: worklist_dev_kernel<true>, worklist_kernel<true>)
        finally:
            lib.nasrec_worklist_set_wide_min(prev)
        _same(lv.snapshot(), lv.alone, "wide item beside a Transformer backward")
        torch.cuda.synchronize()
        for k, v in mha.outs.items():
            assert torch.equal(v, mha_alone[k]), "the Transformer backward beside a wide item: %s differs" % k
