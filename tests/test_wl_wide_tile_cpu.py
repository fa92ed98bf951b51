"""The launcher's routing of GEMM items to the wide form of the 32 x 32 tile (csrc/worklist.hip wl_gemm_geometry, csrc/worklist_body.h
WL_WIDE) and its per-problem sizing of multi-problem items, asked through nasrec_worklist_item_geometry — host only, no device.

  * nasrec_worklist_set_wide_min(1): every eligible descriptor answers bit 5 of geom[2] on top of WL_T32x32, the 64 x 64 grid in geom[0] /
    geom[1] and the body NASREC_WL_BODY_TILE; a descriptor with a mask operand, with a problem below 64 rows or columns, or of a skinny
    launch answers what it answers with the wide tile switched off;
  * the threshold counts the 32 x 32 workgroups of the launch (gx gy nprob S) and is inclusive;
  * with the value the library starts with, every case of wl_cases.CASES keeps the geom the parent of this change answered
    (tests/golden/wl_geometry_parent.json, recorded from that build); nblk too for one-problem items — multi-problem (zmode) items are now
    sized by the per-problem counts, which the last test states on its own: nblk = sum of per-problem tiles x S for a tile item, sum of
    per-problem ceil(M N / 256) for a second pass.
"""
import ctypes as C
import json
import os

import pytest

import wl_cases as W
from nasrec_amd import _lib as L

WIDE = 32  # bit 5 of geom[2]
KC, RC, TOKR, TOKK, PLAIN, TOKJ = L.AM_KC, L.AM_RC, L.AM_TOKR, L.AM_TOKK, L.CM_PLAIN, L.CM_TOKJ
PART_NAME = {L.WL_WHOLE: "whole", L.WL_MAIN: "main", L.WL_EPI: "epi"}
TILE_DIMS = {W.WL_T32x32: (32, 32), W.WL_T64x16: (64, 16), W.WL_T16x64: (16, 64)}


@pytest.fixture(scope="module")
def lib():
    return L.load()


class wide_min:
    """the setter as a context: the previous value comes back in `finally`"""

    def __init__(self, lib, value):
        self.lib, self.value = lib, value

    def __enter__(self):
        self.prev = self.lib.nasrec_worklist_set_wide_min(self.value)
        return self.prev

    def __exit__(self, *exc):
        self.lib.nasrec_worklist_set_wide_min(self.prev)


def raw_bytes(d):
    return C.string_at(C.addressof(d), L.GemmDesc.seg.offset + d.nseg * C.sizeof(L.GemmSeg))


def query(lib, d, part):
    g = L.WlGeometry()
    b = raw_bytes(d)
    rc = lib.nasrec_worklist_item_geometry(d.kind, part, b, len(b), C.byref(g))
    assert rc == 0, lib.nasrec_last_error().decode(errors="replace")
    return g.nblk, list(g.geom), g.body


def cdiv(a, b):
    return -(-a // b)


def problems(d):
    n = d.nseg if d.zmode else 1
    return [(d.seg[q].M, d.seg[q].N) for q in range(n)]


def build(am, bm, cm, probs, zmode, **kw):
    return W.gemm_case(W.Ctx("cpu", 1), am, bm, cm, probs, zmode, **kw)


# (name, descriptor factory): every one reaches WL_T32x32 (64 x 64 tiles x S >= 128), has no mask operand and no problem below 64 x 64
ELIGIBLE = [
    ("kckc_513x897_k100_200", lambda: build(KC, KC, PLAIN, [dict(M=513, N=897, K=[100, 200])], 0)),  # (20 k-steps: past the dense_small body)
    ("kcrc_s11_129x193_k200", lambda: build(KC, RC, PLAIN, [dict(M=129, N=193, K=[200])], 0, splitk=11)),
    ("rcrc_s3_450x391_k200_ones", lambda: build(RC, RC, PLAIN, [dict(M=450, N=391, K=[200], ones=1, Mvalid=301)], 0, splitk=3)),
    ("tok_fwd_130x912_k13_100_64", lambda: build(KC, TOKR, TOKJ, [dict(M=513, N=57 * 16, K=[13, 100, 64])], 0)),
    ("zmode_s7_unequal", lambda: build(KC, RC, PLAIN, [dict(M=130, N=70, K=100), dict(M=130, N=200, K=100), dict(M=65, N=64, K=100)], 1, splitk=7)),
    ("zmode_eight_unsplit", lambda: build(RC, RC, PLAIN, [dict(M=300, N=300, K=45) for _ in range(5)]
                                          + [dict(M=130, N=70, K=45), dict(M=65, N=64, K=45), dict(M=130, N=200, K=45)], 1)),
]
# ... and one that is not, for each clause of the rule
INELIGIBLE = [
    ("mask_operand", lambda: build(KC, KC, PLAIN, [dict(M=513, N=897, K=[100], amask=True)], 0)),
    ("a_problem_of_63_rows", lambda: build(KC, RC, PLAIN, [dict(M=300, N=300, K=100), dict(M=63, N=300, K=100)], 1, splitk=7)),
    ("a_problem_of_14_columns", lambda: build(KC, RC, PLAIN, [dict(M=128, N=14, K=256), dict(M=128, N=32, K=256), dict(M=128, N=768, K=256)], 1, splitk=4)),
    ("skinny_launch_127_tiles", lambda: build(KC, KC, PLAIN, [dict(M=64, N=127 * 64, K=[100, 200])], 0)),
    ("skinny_launch_s3_36_tiles", lambda: build(KC, RC, PLAIN, [dict(M=130, N=200, K=[200])], 0, splitk=3)),
]


@pytest.mark.parametrize("name,make", ELIGIBLE, ids=[e[0] for e in ELIGIBLE])
def test_eligible_items_take_the_wide_tile_when_forced(lib, name, make):
    d = make().desc
    part = L.WL_MAIN if d.splitk > 1 else L.WL_WHOLE
    S = max(d.splitk, 1)
    with wide_min(lib, 0):
        n0, g0, body0 = query(lib, d, part)
    with wide_min(lib, 1):
        n1, g1, body1 = query(lib, d, part)
        epi = query(lib, d, L.WL_EPI) if d.splitk > 1 else None
    with wide_min(lib, 0):
        assert epi == (query(lib, d, L.WL_EPI) if d.splitk > 1 else None)  # (a second pass knows no tiles)
    Mmax, Nmax = max(p[0] for p in problems(d)), max(p[1] for p in problems(d))
    assert g0[2] & 3 == W.WL_T32x32 and not g0[2] & WIDE and g0[:2] == [cdiv(Nmax, 32), cdiv(Mmax, 32)]
    assert g1[2] == g0[2] | WIDE and g1[:2] == [cdiv(Nmax, 64), cdiv(Mmax, 64)]
    assert body0 == body1 == L.WL_BODY_TILE
    assert W.body_of(d.kind, part, g1) == W.body_of(d.kind, part, g0)  # (the decoding of the existing tests names the same body)
    assert n1 == sum(cdiv(M, 64) * cdiv(N, 64) for M, N in problems(d)) * S
    assert n0 == sum(cdiv(M, 32) * cdiv(N, 32) for M, N in problems(d)) * S


@pytest.mark.parametrize("name,make", INELIGIBLE, ids=[e[0] for e in INELIGIBLE])
def test_ineligible_items_keep_their_geometry_when_forced(lib, name, make):
    d = make().desc
    for part in ((L.WL_MAIN, L.WL_EPI) if d.splitk > 1 else (L.WL_WHOLE,)):
        with wide_min(lib, 0):
            off = query(lib, d, part)
        with wide_min(lib, 1):
            on = query(lib, d, part)
        assert on == off and not on[1][2] & WIDE, (name, part, on, off)


def test_the_threshold_counts_32x32_workgroups_and_is_inclusive(lib):
    d = build(KC, RC, PLAIN, [dict(M=129, N=193, K=[200])], 0, splitk=11).desc
    count = cdiv(193, 32) * cdiv(129, 32) * 11
    for value, wide in ((count, True), (count + 1, False), (0, False), (-1, False), (1, True)):
        with wide_min(lib, value):
            assert bool(query(lib, d, L.WL_MAIN)[1][2] & WIDE) == wide, value
    z = build(KC, RC, PLAIN, [dict(M=130, N=70, K=100), dict(M=130, N=200, K=100), dict(M=65, N=64, K=100)], 1, splitk=7).desc
    count = cdiv(200, 32) * cdiv(130, 32) * 3 * 7  # (the grid of the largest problem, once per problem and split)
    for value, wide in ((count, True), (count + 1, False)):
        with wide_min(lib, value):
            assert bool(query(lib, z, L.WL_MAIN)[1][2] & WIDE) == wide, value


def test_the_setter_returns_the_previous_value_and_finally_restores_it(lib):
    start = lib.nasrec_worklist_set_wide_min(77)
    try:
        assert lib.nasrec_worklist_set_wide_min(5) == 77
        with pytest.raises(RuntimeError):
            with wide_min(lib, 9) as prev:
                assert prev == 5
                raise RuntimeError("leaves through finally")
        assert lib.nasrec_worklist_set_wide_min(5) == 5
    finally:
        lib.nasrec_worklist_set_wide_min(start)
    assert lib.nasrec_worklist_set_wide_min(start) == start


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wl_geometry_parent.json")


def test_with_the_default_every_case_of_the_table_keeps_the_parents_geometry(lib):
    parent = json.load(open(GOLDEN))
    gemm = [c for c in W.CASES if c.gemm]
    assert sorted(parent) == sorted(c.name for c in gemm)
    for c in gemm:
        d = c.build("cpu").desc
        for part in ((L.WL_MAIN, L.WL_EPI) if d.splitk > 1 else (L.WL_WHOLE,)):
            nblk, geom, _ = query(lib, d, part)
            p_nblk, p_geom = parent[c.name][PART_NAME[part]]
            assert geom == p_geom, (c.name, part, geom, p_geom)
            if not d.zmode:
                assert nblk == p_nblk, (c.name, part)
            else:
                assert nblk <= p_nblk, (c.name, part)  # (never more than the grid of the largest problem; exactly what: the next test)


def test_multi_problem_items_are_sized_by_their_problems(lib):
    zs = [c for c in W.CASES if c.gemm and c.build("cpu").desc.zmode]
    extra = [make().desc for _, make in ELIGIBLE + INELIGIBLE]
    tiles = passes = 0
    for d in [c.build("cpu").desc for c in zs] + [e for e in extra if e.zmode]:
        S = max(d.splitk, 1)
        for value in (0, 1):
            with wide_min(lib, value):
                nblk, geom, body = query(lib, d, L.WL_MAIN if d.splitk > 1 else L.WL_WHOLE)
                if body == L.WL_BODY_TILE:
                    tbm, tbn = (64, 64) if geom[2] & WIDE else TILE_DIMS[geom[2] & 3]
                    assert nblk == sum(cdiv(M, tbm) * cdiv(N, tbn) for M, N in problems(d)) * S
                    tiles += 1
                if d.splitk > 1:
                    assert query(lib, d, L.WL_EPI)[0] == sum(cdiv(M * N, 256) for M, N in problems(d))
                    passes += 1
    assert tiles >= 8 and passes >= 4
    # the input gradients of the batch-256 step that launched 2 x 48 x 3 x 4 = 1152 workgroups of 64 x 16 strips where 408 have a strip, and
    # 1152 in the second pass where 407 have an element
    d = build(KC, RC, PLAIN, [dict(M=128, N=14, K=256), dict(M=128, N=32, K=256), dict(M=128, N=768, K=256)], 1, splitk=4).desc
    assert query(lib, d, L.WL_MAIN)[1][2] & 3 == W.WL_T64x16
    assert query(lib, d, L.WL_MAIN)[0] == 4 * (2 * 1 + 2 * 2 + 2 * 48) == 408
    assert query(lib, d, L.WL_EPI)[0] == 7 + 16 + 384 == 407
