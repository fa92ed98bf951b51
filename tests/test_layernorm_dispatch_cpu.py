"""The host-side half of tests/test_layernorm_kernel_gpu.py, checked without a GPU: `ln_branch` (the restated kernel choice of
launch_layernorm) against a hand-written table, and the case list against the coverage it is there to give — every kernel
family in both directions, each with an accumulating launch, a padded stride and a prefix mask that cuts the row."""
import collections

import pytest

import test_layernorm_kernel_gpu as K
from nasrec_amd import _lib as L

BASE = 0x7F0000001000  # a 16-byte aligned address; nothing is dereferenced here
FWD, BWD = L.OP_LAYERNORM_FWD, L.OP_LAYERNORM_BWD


def desc(kind, mode, R, D, ldx, ldy, nblk=1, x=0, w=0, b=0, y=0, dy=0, dx=0):
    """pointer arguments are offsets in floats from an aligned base"""
    d = L.LayerNormDesc()
    d.kind, d.mode, d.R, d.D, d.ldx, d.ldy, d.nblk = kind, mode, R, D, ldx, ldy, nblk
    d.x, d.w, d.b, d.y, d.dy, d.dx = (BASE + 4 * o for o in (x, w, b, y, dy, dx))
    d.stats = d.dwb_partial = BASE
    return d


TABLE = [
    # dense: the width decides the number of 16-byte vectors per lane
    (desc(FWD, L.AM_KC, 37, 4, 4, 4), "kc_vec1"),
    (desc(FWD, L.AM_KC, 37, 256, 256, 256), "kc_vec1"),
    (desc(BWD, L.AM_KC, 37, 260, 260, 260), "kc_vec2"),
    (desc(FWD, L.AM_KC, 37, 512, 520, 532), "kc_vec2"),
    (desc(BWD, L.AM_KC, 37, 516, 516, 516, nblk=10), "kc_vec4"),
    (desc(FWD, L.AM_KC, 1, 1024, 1024, 1024), "kc_vec4"),
    # ... unless the width, a stride or a pointer is off the 16-byte grid
    (desc(FWD, L.AM_KC, 37, 1023, 1023, 1023), "kc"),
    (desc(BWD, L.AM_KC, 37, 190, 190, 190), "kc"),
    (desc(FWD, L.AM_KC, 37, 64, 67, 64), "kc"),
    (desc(BWD, L.AM_KC, 37, 64, 64, 66), "kc"),
    (desc(FWD, L.AM_KC, 37, 1024, 1024, 1024, x=1), "kc"),
    (desc(BWD, L.AM_KC, 37, 1024, 1024, 1024, x=2), "kc"),
    (desc(FWD, L.AM_KC, 37, 64, 64, 64, w=1), "kc"),
    (desc(BWD, L.AM_KC, 37, 64, 64, 64, b=3), "kc"),
    # the forward looks at y only, the backward at dy and dx only
    (desc(FWD, L.AM_KC, 37, 1024, 1024, 1024, y=1), "kc"),
    (desc(BWD, L.AM_KC, 37, 1024, 1024, 1024, y=1), "kc_vec4"),
    (desc(FWD, L.AM_KC, 37, 1024, 1024, 1024, dy=1, dx=1), "kc_vec4"),
    (desc(BWD, L.AM_KC, 37, 1024, 1024, 1024, dy=1), "kc"),
    (desc(BWD, L.AM_KC, 37, 1024, 1024, 1024, dx=1), "kc"),
    (desc(FWD, L.AM_KC, 37, 64, 64, 64, x=4, y=8), "kc_vec1"),  # 16 and 32 bytes in: still aligned
    # token axis: a wavefront per sample where the sample blocks are aligned
    (desc(FWD, L.AM_TOKR, 16, 1, 16, 16), "tok_wave"),
    (desc(BWD, L.AM_TOKR, 272, 64, 16 * 67, 16 * 69, nblk=2), "tok_wave"),
    (desc(FWD, L.AM_TOKR, 80, 45, 16 * 45, 16 * 45, dy=1, dx=1), "tok_wave"),
    (desc(BWD, L.AM_TOKR, 80, 45, 16 * 45, 16 * 45, y=1), "tok_wave"),
    # ... else a thread per row, registers by the next multiple of 16 tokens
    (desc(FWD, L.AM_TOKR, 16, 1, 16, 16, x=1), "tokr_reg16"),
    (desc(FWD, L.AM_TOKR, 16, 16, 256, 256, y=1), "tokr_reg16"),
    (desc(BWD, L.AM_TOKR, 16, 17, 272, 272, dy=1), "tokr_reg32"),
    (desc(BWD, L.AM_TOKR, 16, 32, 512, 512, dx=1), "tokr_reg32"),
    (desc(FWD, L.AM_TOKR, 16, 33, 528, 528, x=1), "tokr_reg48"),
    (desc(BWD, L.AM_TOKR, 320, 48, 768, 768, nblk=2, x=1), "tokr_reg48"),
    (desc(FWD, L.AM_TOKR, 16, 49, 784, 784, x=1), "tokr_reg64"),
    (desc(BWD, L.AM_TOKR, 16, 64, 1024, 1024, x=3), "tokr_reg64"),
    (desc(FWD, L.AM_TOKR, 80, 45, 16 * 45 + 2, 16 * 45), "tokr_reg48"),  # sample stride off the grid
    (desc(FWD, L.AM_TOKR, 75, 20, 320, 320), "tokr_reg32"),  # a partial last sample
    # nothing is launched: no rows, or an error return
    (desc(FWD, L.AM_KC, 0, 64, 64, 64), None),
    (desc(BWD, L.AM_TOKR, 0, 16, 256, 256, nblk=7), None),
    (desc(FWD, L.AM_KC, 2, 1025, 1025, 1025), None),
    (desc(FWD, L.AM_TOKR, 16, 65, 16 * 65, 16 * 65), None),
    (desc(BWD, L.AM_KC, 2, 8, 8, 8, nblk=0), None),
    (desc(BWD, L.AM_TOKR, 272, 8, 128, 128, nblk=1), None),
    (desc(BWD, L.AM_TOKR, 256, 8, 128, 128, nblk=2), None),
    (desc(FWD, L.AM_RC, 2, 8, 8, 8), None),
    (desc(BWD, L.AM_TOKK, 2, 8, 8, 8), None),
]


@pytest.mark.parametrize("n", range(len(TABLE)))
def test_ln_branch_against_the_table(n):
    d, want = TABLE[n]
    assert K.ln_branch(d) == want


def branches(c):
    d = K.case_desc(c, x=BASE, w=BASE, b=BASE, y=BASE, stats=BASE, dy=BASE, dx=BASE, part=BASE)
    f = K.ln_branch(d)
    d.kind = BWD
    return f, K.ln_branch(d)


def test_every_case_reaches_the_kernels_it_declares():
    for c in K.CASES:
        assert branches(c) == (c.fwd, c.bwd), c.id
        assert c.fwd in K.FAMILIES and c.bwd in K.FAMILIES


def hits():
    """(family, direction) -> the cases that run it"""
    h = collections.defaultdict(list)
    for c in K.CASES:
        h[c.fwd, "fwd"].append(c)
        h[c.bwd, "bwd"].append(c)
    return h


def test_every_kernel_meets_accumulate_a_padded_stride_and_a_cutting_mask_in_both_directions():
    h = hits()
    unit = {"kc": 1, "tok": 16}
    for fam in K.FAMILIES:
        for direction in ("fwd", "bwd"):
            cs = h[fam, direction]
            assert cs, (fam, direction)
            assert any(c.acc == 1 for c in cs), (fam, direction, "accumulate")
            assert any(c.acc == 0 for c in cs), (fam, direction, "overwrite")
            assert any(c.ldx > c.D * unit[c.mode] and c.ldy > c.D * unit[c.mode] and c.ldx != c.ldy for c in cs), (fam, direction, "padding")
            assert any(0 < c.dims < c.D for c in cs) or all(c.D == 1 for c in cs), (fam, direction, "mask")
            assert {c.act for c in cs} == {K.NONE, K.RELU, K.SILU, K.SIGMOID}, (fam, direction, "activations")
        assert any(c.reduce for c in h[fam, "bwd"]), (fam, "OP_REDUCE_ROWS")


def test_the_case_list_holds_every_value_it_is_there_for():
    h = hits()
    dense = [c for c in K.CASES if c.mode == "kc"]
    token = [c for c in K.CASES if c.mode == "tok"]
    widths = {"kc_vec1": {4, 64, 256}, "kc_vec2": {260, 512}, "kc_vec4": {516, 768, 1024}, "kc": {1, 3, 63, 65, 190, 1023, 64, 1024}}
    for fam, want in widths.items():
        for direction in ("fwd", "bwd"):
            cs = h[fam, direction]
            assert want <= {c.D for c in cs}, (fam, direction)
            assert {1, 3, 37} <= {c.R for c in cs}, (fam, direction)
            # dims: none, everything masked, one column, inside a 16-byte vector, exactly D, past D
            assert {-1, 0, 1} <= {c.dims for c in cs}, (fam, direction)
            assert any(c.dims == c.D for c in cs) and any(c.dims == c.D + 5 for c in cs), (fam, direction)
            assert any(0 < c.dims < c.D and c.dims % 4 for c in cs), (fam, direction)
        bw = h[fam, "bwd"]
        assert any(c.nblk == 1 and c.R == 37 for c in bw), fam                        # every wave loops over 9-10 rows
        assert any(c.nblk == 2 and c.R <= 4 for c in bw), fam                         # a workgroup without a live row
        assert any(c.nblk == K.plan_nblk("kc", c.R) and c.R == 37 for c in bw), fam   # the plan's grid
    assert any(c.dims == 201 and c.D > 204 for c in h["kc_vec1", "fwd"])
    # the scalar kernel through each way ln_vec_ok fails, per direction
    assert any(c.ldx % 4 and c.D % 4 == 0 for c in dense) and any(c.ldy % 4 and c.D % 4 == 0 for c in dense)
    assert any(c.x_off % 4 and c.D == 1024 for c in dense)
    assert any(c.y_off % 4 and not c.x_off and (c.fwd, c.bwd) == ("kc", "kc_vec4") for c in dense)
    assert any(c.dy_off % 4 and not c.x_off and (c.fwd, c.bwd) == ("kc_vec4", "kc") for c in dense)
    assert any(c.dx_off % 4 and not c.x_off and (c.fwd, c.bwd) == ("kc_vec4", "kc") for c in dense)
    assert any(c.data == "degenerate" for c in dense) and any(c.data == "mean8" and c.D == 1024 for c in dense)
    # token axis: every chunk edge in both forms, the batch sizes that leave idle waves / ragged blocks / dead waves
    for direction in ("fwd", "bwd"):
        wave = h["tok_wave", direction]
        assert set(K.TOK_D) <= {c.D for c in wave}
        assert {1, 3, 5, 17, 33} <= {c.rows for c in wave}
        assert any(c.dims == -1 for c in wave) and any(c.dims == 0 for c in wave)
        assert any(c.dims == c.D // 2 and c.D > 1 for c in wave) and any(c.dims == c.D for c in wave)
        for nr, lo, hi in ((16, 1, 16), (32, 17, 32), (48, 33, 48), (64, 49, 64)):
            reg = h["tokr_reg%d" % nr, direction]
            assert {lo, hi} <= {c.D for c in reg}, (nr, direction)
        regs = [c for nr in (16, 32, 48, 64) for c in h["tokr_reg%d" % nr, direction]]
        assert {1, 17, 20} <= {c.rows for c in regs}
    assert any(c.y_off and not c.x_off for c in token) and any(c.dy_off and not c.x_off for c in token)
    assert any(c.dx_off and not c.x_off for c in token)
    assert 100 <= len(K.CASES) <= 200


def test_no_relu_case_sits_on_the_kink():
    """decided on the fp64 reference alone (the GPU test asserts the same before it compares anything)"""
    for c in K.CASES:
        if c.act == K.RELU:
            assert K.relu_kink_clear(c, K.case_reference(c)), c.id
