"""Every body of the worklist kernels (csrc/worklist_body.h wl_run; csrc/worklist.hip ps_run_item) against the stand-alone kernel on the
SAME descriptor, bit for bit, and that stand-alone launch against plain fp64 math.  The header of csrc/worklist.hip promises that an item
gives the bits of its stand-alone launch; the engine relies on it (level_schedule and NASREC_PERSIST may be toggled without changing a
training run).  The cases come from tests/wl_cases.py; each one runs in five forms from identical inputs, every output buffer compared in
full (guard rows and columns, split-K workspaces and saved states included):

  a. the stand-alone launch (nasrec_launch on the descriptor)           -> fp64, with the tolerance tests/test_ops_gpu.py uses for the operator
  b. a one-item NASREC_OP_WORKLIST, descriptor by value                 -> torch.equal with (a)
  c. the same launch resident (nasrec_worklist_prepare, _WORKLIST_DEV)  -> torch.equal with (a); the uploaded item's geometry is read back
                                                                           and must name the body the case was written for
  d. at an even and at an odd slot of mixed launches of up to 12 items, with and without a Transformer backward in the launch (the BIG
     instantiation: another dynamic LDS size), behind an empty item, and behind 65535 workgroups (the item table in memory)
  e. as an item of NASREC_OP_PERSIST launches of independent items, once a workgroup per unit and once with a hint of 3 workgroups on
     every item that walks its units (tiles, second passes, the final-logit backward): several units through the same LDS buffer

No tolerance and no timing is introduced here: (b) - (e) are torch.equal with (a).  A split-K product runs as a WL_MAIN item launch
followed by a WL_EPI item launch.  The per-sample token-axis bodies keep their shape tests at the end of this module.

Which case reaches which body (tests/test_worklist_geometry_cpu.py holds this table against wl_cases.CASES and the launcher's geometry;
for the split-K cases the body named is the second pass, their main passes run on tile bodies):

  dense_70x77_k13_dead7_45_bias_relu     -> dense_small.NB1
  dense_70x77_k13_dead7_45_dims40_beta   -> dense_small.NB1
  dense_3x13_k16                         -> dense_small.NB1
  dense_17x36_k128_eight_steps           -> dense_small.NB1
  dense_33x16_k100_60_two_batches        -> dense_small.NB2
  dense_33x16_k260_leaves_the_body       -> T64x16.KC.KC.plain
  dense_dx_three_problems                -> dense_small_dx
  dense_dx_three_problems_relu_mask      -> dense_small_dx
  dense_dx_k129_leaves_the_body          -> T64x16.KC.RC.plain
  token_fwd_17x64_tok5_16_33             -> token_fwd
  token_dx_5x48_tok72_32                 -> token_dx
  t32_kckc_plain_k45                     -> T32x32.KC.KC.plain
  t32_kcrc_plain_k65                     -> T32x32.KC.RC.plain
  t32_rcrc_plain_k64                     -> T32x32.RC.RC.plain
  t64x16_kckc_plain_k4096                -> T64x16.KC.KC.plain
  t64x16_kcrc_plain_tok45                -> T64x16.KC.RC.plain
  t64x16_rcrc_plain_k65                  -> T64x16.RC.RC.plain
  t16x64_kckc_plain_k300                 -> T16x64.KC.KC.plain
  t16x64_kcrc_plain_k129                 -> T16x64.KC.RC.plain
  t16x64_rcrc_plain_tok_k_concat         -> T16x64.RC.RC.plain
  t32_kckc_mask_k45                      -> T32x32.KC.KC.mask
  t32_kcrc_mask_k65                      -> T32x32.KC.RC.mask
  t32_rcrc_mask_k64                      -> T32x32.RC.RC.mask
  t64x16_kckc_mask_k4096                 -> T64x16.KC.KC.mask
  t64x16_kcrc_mask_tok45                 -> T64x16.KC.RC.mask
  t64x16_rcrc_mask_k65                   -> T64x16.RC.RC.mask
  t16x64_kckc_mask_k300                  -> T16x64.KC.KC.mask
  t16x64_kcrc_mask_k129                  -> T16x64.KC.RC.mask
  t16x64_rcrc_mask_tok_k_concat          -> T16x64.RC.RC.mask
  tie_80x16_16x80_wide                   -> T64x16.RC.RC.plain
  tie_128x64_tall                        -> T16x64.RC.RC.plain
  splitk3_plain_70x77_k13_dead7_781      -> second_pass
  splitk4_plain_70x77_k13_dead7_781      -> second_pass
  splitk3_tokj_40x144_tok26_45           -> second_pass
  splitk4_tokj_40x144_tok26_45           -> second_pass
  splitk3_zmode_unequal_weight_gradients -> second_pass
  splitk4_zmode_unequal_weight_gradients -> second_pass
  mha_fwd_n1_d-1_b3_saved                -> mha_fwd
  mha_fwd_n1_d-1_b3                      -> mha_fwd
  mha_bwd_n1_d-1_b3                      -> mha_bwd
  mha_fwd_n7_d-1_b5_saved                -> mha_fwd
  mha_fwd_n7_d-1_b5                      -> mha_fwd
  mha_bwd_n7_d-1_b5                      -> mha_bwd
  mha_fwd_n17_d16_b6_saved               -> mha_fwd
  mha_fwd_n17_d16_b6                     -> mha_fwd
  mha_bwd_n17_d16_b6                     -> mha_bwd
  mha_fwd_n33_d-1_b9_saved               -> mha_fwd
  mha_fwd_n33_d-1_b9                     -> mha_fwd
  mha_bwd_n33_d-1_b9                     -> mha_bwd
  mha_fwd_n64_d40_b5_saved               -> mha_fwd
  mha_fwd_n64_d40_b5                     -> mha_fwd
  mha_bwd_n64_d40_b5                     -> mha_bwd
  mha_fwd_n48_d0_b3_saved                -> mha_fwd
  mha_fwd_n48_d0_b3                      -> mha_fwd
  mha_bwd_n48_d0_b3                      -> mha_bwd
  mha_fwd_n16_d-1_b5_slabs_saved         -> mha_fwd
  mha_fwd_n16_d-1_b5_slabs               -> mha_fwd
  mha_bwd_n16_d-1_b5_slabs_shared        -> mha_bwd
  mha_fwd_n48_d-1_b3_slabs_saved         -> mha_fwd
  mha_fwd_n48_d-1_b3_slabs               -> mha_fwd
  mha_bwd_n48_d-1_b3_slabs_shared        -> mha_bwd
  mha_fwd_n64_d40_b5_slabs_saved         -> mha_fwd
  mha_fwd_n64_d40_b5_slabs               -> mha_fwd
  mha_bwd_n64_d40_b5_slabs_shared        -> mha_bwd
  mha_fwd_n7_d-1_b6_slabs_saved          -> mha_fwd
  mha_fwd_n7_d-1_b6_slabs                -> mha_fwd
  mha_bwd_n7_d-1_b6_slabs_shared         -> mha_bwd
  mha_fwd_n16_d-1_b5_slab_saved          -> mha_fwd
  mha_fwd_n16_d-1_b5_slab                -> mha_fwd
  mha_bwd_n16_d-1_b5_slab_shared         -> mha_bwd
  mha_fwd_n48_d-1_b3_own_saved           -> mha_fwd
  mha_fwd_n48_d-1_b3_own                 -> mha_fwd
  mha_bwd_n48_d-1_b3_own_shared          -> mha_bwd
  mha_fwd_n48_d-1_b3_slab_saved          -> mha_fwd
  mha_fwd_n48_d-1_b3_slab                -> mha_fwd
  mha_bwd_n48_d-1_b3_slab_shared         -> mha_bwd
  mha_fwd_n64_d64_b5_own_saved           -> mha_fwd
  mha_fwd_n64_d64_b5_own                 -> mha_fwd
  mha_bwd_n64_d64_b5_own_shared          -> mha_bwd
  mha_fwd_n64_d40_b5_slab_saved          -> mha_fwd
  mha_fwd_n64_d40_b5_slab                -> mha_fwd
  mha_bwd_n64_d40_b5_slab_shared         -> mha_bwd
  mha_fwd_n64_d-1_b3_slab_saved          -> mha_fwd
  mha_fwd_n64_d-1_b3_slab                -> mha_fwd
  mha_bwd_n64_d-1_b3_slab_shared         -> mha_bwd
  fm_fwd_b1_n1_acc0                      -> fm_fwd
  fm_bwd_b1_n1_acc0                      -> fm_bwd
  fm_fwd_b5_n26_acc1                     -> fm_fwd
  fm_bwd_b5_n26_acc1                     -> fm_bwd
  fm_fwd_b37_n48_acc1                    -> fm_fwd
  fm_bwd_b37_n48_acc1                    -> fm_bwd
  fm_fwd_b37_n1_acc0                     -> fm_fwd
  fm_bwd_b37_n1_acc0                     -> fm_bwd
  fm_fwd_b5_n48_acc0                     -> fm_fwd
  fm_bwd_b5_n48_acc0                     -> fm_bwd
  fm_fwd_b1_n26_acc1                     -> fm_fwd
  fm_bwd_b1_n26_acc1                     -> fm_bwd
  fm_fwd_b1_n16_add_tight                -> fm_fwd
  fm_fwd_b1_n48_add_tight                -> fm_fwd
  fm_fwd_b5_n16_add_tight                -> fm_fwd
  fm_fwd_b5_n48_add_tight                -> fm_fwd
  fm_fwd_b5_n16_tight                    -> fm_fwd
  fm_bwd_b5_n16_tight_acc1               -> fm_bwd
  fm_fwd_b5_n16_slab                     -> fm_fwd
  fm_bwd_b5_n16_slab_acc1                -> fm_bwd
  fm_fwd_b5_n48_tight                    -> fm_fwd
  fm_bwd_b5_n48_tight_acc1               -> fm_bwd
  fm_fwd_b5_n48_slab                     -> fm_fwd
  fm_bwd_b5_n48_slab_acc1                -> fm_bwd
  dot_tri_fwd_k2_b3                      -> dot_tri_fwd
  dot_tri_bwd_k2_b3                      -> dot_tri_bwd
  dot_tri_fwd_k9_b11                     -> dot_tri_fwd
  dot_tri_bwd_k9_b11                     -> dot_tri_bwd
  dot_tri_fwd_k16_b3                     -> dot_tri_fwd
  dot_tri_bwd_k16_b3                     -> dot_tri_bwd
  dot_tri_fwd_k17_b11                    -> dot_tri_fwd
  dot_tri_bwd_k17_b11                    -> dot_tri_bwd
  dot_tri_fwd_k33_b3                     -> dot_tri_fwd
  dot_tri_bwd_k33_b3                     -> dot_tri_bwd
  dot_tri_fwd_k46_b11                    -> dot_tri_fwd
  dot_tri_bwd_k46_b11                    -> dot_tri_bwd
  dot_tri_fwd_k9_b3_tight                -> dot_tri_fwd
  dot_tri_bwd_k9_b3_tight                -> dot_tri_bwd
  dot_tri_fwd_k17_b5_tight               -> dot_tri_fwd
  dot_tri_bwd_k17_b5_tight               -> dot_tri_bwd
  dot_tri_fwd_k33_b3_tight               -> dot_tri_fwd
  dot_tri_bwd_k33_b3_tight               -> dot_tri_bwd
  dot_tri_fwd_k40_b5_tight               -> dot_tri_fwd
  dot_tri_bwd_k40_b5_tight               -> dot_tri_bwd
  dot_tri_fwd_k46_b3_tight               -> dot_tri_fwd
  dot_tri_bwd_k46_b3_tight               -> dot_tri_bwd
  copy_forward_gap                       -> copy_segs
  copy_reverse_gap                       -> copy_segs
  copy_4097x4096_unpacked_table          -> copy_segs
  copy_forward_accumulate_gap            -> copy_segs
  copy_forward_null_segment_gap          -> copy_segs
  copy_forward_accumulate_one_segment    -> copy_segs
  copy_forward_zero_fill                 -> copy_segs
  copy_reverse_one_segment               -> copy_segs
  gate_21x32_one_segment                 -> gate_bwd
  gate_21x32_two_segments                -> gate_bwd
  gate_5x61_seven_segments               -> gate_bwd
  gate_5x29_head_acc_tight               -> gate_bwd
  gate_5x29_head_set_tight               -> gate_bwd
  gate_5x29_head_no_dr_tight             -> gate_bwd
  gate_5x29_all_set_tight                -> gate_bwd
  gate_5x13_all_no_dr_tight              -> gate_bwd
  gate_5x21_2_segments_tight             -> gate_bwd
  gate_5x29_3_segments_tight             -> gate_bwd
  gate_5x37_4_segments_tight             -> gate_bwd
  gate_5x45_5_segments_tight             -> gate_bwd
  gate_5x53_6_segments_tight             -> gate_bwd
  gate_5x61_7_segments_tight             -> gate_bwd
  gate_5x29_head_acc_wide                -> gate_bwd
  gate_5x29_head_set_wide                -> gate_bwd
  gate_5x29_head_no_dr_wide              -> gate_bwd
  gate_5x29_all_set_wide                 -> gate_bwd
  gate_5x13_all_no_dr_wide               -> gate_bwd
  gate_5x21_2_segments_wide              -> gate_bwd
  gate_5x29_3_segments_wide              -> gate_bwd
  gate_5x37_4_segments_wide              -> gate_bwd
  gate_5x45_5_segments_wide              -> gate_bwd
  gate_5x53_6_segments_wide              -> gate_bwd
  gate_5x61_7_segments_wide              -> gate_bwd
  reduce_r13_c1696_mha                   -> reduce_rows
  reduce_r256_c1696_mha                  -> reduce_rows
  reduce_r256_c37_16dst                  -> reduce_rows
  reduce_r1_c37_1dst                     -> reduce_rows
  reduce_r13_c37_16dst                   -> reduce_rows
  reduce_r64_c37_16dst                   -> reduce_rows
  reduce_r300_c37_16dst                  -> reduce_rows
  reduce_r16_c34_2dst_tight              -> reduce_rows
  reduce_r64_c34_2dst_tight              -> reduce_rows
  reduce_r256_c1696_mha_tight            -> reduce_rows
  dedup_b1_fs5                           -> dedup_ids
  dedup_b37_fs5                          -> dedup_ids
  dedup_b255_fs5                         -> dedup_ids
  dedup_b256_fs5                         -> dedup_ids
  final_fwd_b5                           -> final_fwd
  final_fused_b5                         -> final_fused
  final_bwd_b5_acc01                     -> final_bwd
  final_bwd_b5_acc10                     -> final_bwd
  final_fwd_b256                         -> final_fwd
  final_fused_b256                       -> final_fused
  final_bwd_b256_acc01                   -> final_bwd
  final_bwd_b256_acc10                   -> final_bwd
  final_fwd_b1030                        -> final_fwd
  final_fused_b1030                      -> final_fused
  final_bwd_b1030_acc01                  -> final_bwd
  final_bwd_b1030_acc10                  -> final_bwd
"""
import ctypes as C

import pytest
import torch

import wl_cases as W
from nasrec_amd import _lib as L
from nasrec_amd import schedule as S

pytestmark = pytest.mark.gpu
PART_NAME = {L.WL_WHOLE: "whole", L.WL_MAIN: "main", L.WL_EPI: "epi"}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _run(lib, d):
    L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()


_KEEP = []


def _resident(lib, w):
    """the same worklist launch with its descriptor uploaded once (ABI 17: nasrec_worklist_prepare -> NASREC_OP_WORKLIST_DEV)"""
    buf = torch.empty(C.sizeof(L.WorklistDesc), dtype=torch.uint8, device="cuda")
    dv = L.WorklistDevDesc()
    torch.cuda.synchronize()
    L.check(lib.nasrec_worklist_prepare(C.addressof(w), buf.data_ptr(), C.addressof(dv)))
    assert dv.kind == L.OP_WORKLIST_DEV and dv.total_blocks > 0 and dv.dev == buf.data_ptr()
    _KEEP.append(buf)
    return dv


# ---- the case table in its five forms --------------------------------------------------------------------------------------------------
class Live:
    """a case on the device: its buffers as built (`init`) and after the stand-alone launch (`a`, form a: computed once, left unchanged)"""

    def __init__(self, lib, case):
        self.case, self.b = case, case.build("cuda")
        for d in self.b.setup:
            _run(lib, d)
        self.init = {k: v.clone() for k, v in self.b.outs.items()}
        _run(lib, self.b.desc)
        self.a = self.snapshot()
        assert any(not torch.equal(self.init[k], self.a[k]) for k in self.a), "a launch that leaves every buffer as it was compares nothing"

    def reset(self):
        for k, v in self.b.outs.items():
            v.copy_(self.init[k])

    def snapshot(self):
        return {k: v.clone() for k, v in self.b.outs.items()}

    def assert_same_bits(self, what):
        torch.cuda.synchronize()
        for k, v in self.b.outs.items():
            assert torch.equal(v, self.a[k]), "%s: %s of %s differs from the stand-alone launch" % (what, k, self.case.name)

    def item(self, part):
        b = S.item_bytes(S.Node(self.b.desc, PART_NAME[part]))
        assert b is not None, self.case.name
        return (self.b.desc.kind, part, b)


_LIVE = {}


def live(lib, case):
    if case.name not in _LIVE:
        _LIVE[case.name] = Live(lib, case)
    return _LIVE[case.name]


def worklists(entries):
    """(kind, part, bytes) items -> NASREC_OP_WORKLIST descriptors: up to 12 items each, as many launches as the blobs need"""
    out, cur, off = [], None, 0
    for kind, part, b in entries:
        size = (len(b) + 15) & ~15
        if cur is None or cur.n == L.WL_MAX_ITEMS or off + size > L.WL_BLOB_BYTES:
            cur = L.WorklistDesc()
            cur.kind, cur.n = L.OP_WORKLIST, 0
            off = 0
            out.append(cur)
        it = cur.item[cur.n]
        it.kind, it.part, it.off = kind, part, off
        C.memmove(C.addressof(cur) + L.WorklistDesc.blob.offset + off, b, len(b))
        cur.n += 1
        off += size
    return out


def uploaded(dv):
    """the completed descriptor nasrec_worklist_prepare left in device memory"""
    buf = next(t for t in _KEEP if t.data_ptr() == dv.dev)
    return L.WorklistDesc.from_buffer_copy(buf.cpu().numpy().tobytes())


def expected_body(case, b, part):
    return case.body if part == b.parts[-1] else None  # (a main pass: some tile body)


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_item_by_value_and_resident_equal_the_stand_alone_launch_which_equals_fp64(lib, case):
    lv = live(lib, case)
    if case.gemm:  # (the items promise the bits of the general template, not of the other GEMM families)
        from nasrec_amd import plan as P
        assert P.gemm_route(lv.b.desc)[0] == L.GEMM_ROUTE_GENERAL
    lv.b.check(lv.a)  # (a) against fp64
    lv.reset()
    for part in lv.b.parts:  # (b)
        (w,) = worklists([lv.item(part)])
        _run(lib, w)
    lv.assert_same_bits("item by value")
    lv.reset()
    for part in lv.b.parts:  # (c)
        (w,) = worklists([lv.item(part)])
        dv = _resident(lib, w)
        it = uploaded(dv).item[0]
        body = W.body_of(it.kind, it.part, it.geom)
        assert it.nblk == dv.total_blocks and it.first == 0
        assert body == case.body if part == lv.b.parts[-1] else body.startswith("T"), (case.name, part, body)
        _run(lib, dv)
        _KEEP.pop()
    lv.assert_same_bits("resident item")


def _one_per_body():
    seen, out = set(), []
    for c in W.CASES:
        if c.body not in seen and c.name != W.BIG_COPY:
            seen.add(c.body)
            out.append(c)
    # ... and the tile bodies the main passes of the split-K cases run on come with those cases
    return out + [c for c in W.CASES if c.body == "second_pass" and c not in out]


def _mixed_launch_lists(lib, big):
    """groups of cases that share launches.  big: every launch is headed by a Transformer backward (the BIG instantiation) and the
    cases are one per body; otherwise every case of the table (but the backward ones and the 65535-workgroup copy)"""
    bwd = [c for c in W.CASES if c.kind == "mha_bwd"]
    rest = _one_per_body() if big else [c for c in W.CASES if c.name != W.BIG_COPY]
    rest = [c for c in rest if c.kind != "mha_bwd"]
    groups, cur, size = [], [], 0
    for c in rest:
        lv = live(lib, c)
        sz = max((len(lv.item(p)[2]) + 15) & ~15 for p in lv.b.parts)
        head = ((len(live(lib, bwd[0]).item(L.WL_WHOLE)[2]) + 15) & ~15) if big else 0
        limit = L.WL_MAX_ITEMS - (1 if big else 0)
        if cur and (len(cur) == limit or size + sz > L.WL_BLOB_BYTES - head - _EMPTY_BYTES):
            groups.append(cur)
            cur, size = [], 0
        cur.append(c)
        size += sz
    groups.append(cur)
    if big:
        groups = [[bwd[i % len(bwd)]] + g for i, g in enumerate(groups)]
    return groups


def _empty_gemm():
    """a GEMM item with M = 0: no workgroups, the same `first` as the item behind it"""
    d = L.GemmDesc()
    d.kind, d.amode, d.bmode, d.cmode, d.nseg, d.zmode, d.dims_in_use, d.splitk = L.OP_GEMM, L.AM_KC, L.AM_KC, L.CM_PLAIN, 1, 0, -1, 1
    s = d.seg[0]
    s.M, s.N, s.K, s.lda, s.ldb, s.ldc = 0, 77, 45, 45, 45, 77
    return (L.OP_GEMM, L.WL_WHOLE, C.string_at(C.addressof(d), L.GemmDesc.seg.offset + C.sizeof(L.GemmSeg)))


_EMPTY_BYTES = (len(_empty_gemm()[2]) + 15) & ~15


def _ordered(entries, reverse):
    """as built, or reversed — behind an empty item when the count is odd, so that EVERY item changes the parity of its slot"""
    if not reverse:
        return list(entries)
    return ([_empty_gemm()] if len(entries) % 2 else []) + list(entries[::-1])


def _slot(k, n, reverse):
    return k if not reverse else (n - 1 - k) + (n % 2)


def _run_group_as_worklists(lib, group, reverse):
    lvs = [live(lib, c) for c in group]
    for lv in lvs:
        lv.reset()
    ws = worklists(_ordered([lv.item(lv.b.parts[0]) for lv in lvs], reverse))
    assert len(ws) == 1, "a group fits one launch"
    _run(lib, ws[0])
    second = [lv.item(L.WL_EPI) for lv in lvs if len(lv.b.parts) == 2]
    for w in worklists(_ordered(second, reverse)):
        _run(lib, w)
    return lvs, ws[0]


@pytest.mark.parametrize("reverse", [False, True], ids=["as_built", "reversed"])
@pytest.mark.parametrize("big", [False, True], ids=["plain", "with_mha_bwd"])
def test_items_of_mixed_launches_equal_their_stand_alone_launches(lib, big, reverse):
    """form (d): up to 12 items of different kinds in one launch, disjoint outputs; in the two orders every item sits at an even and at an
    odd slot of the packed table (two 16-bit halves per scalar).  with_mha_bwd: a Transformer backward heads every launch, so every body
    runs in the BIG instantiation."""
    groups = _mixed_launch_lists(lib, big)
    bodies = set()
    for gi, group in enumerate(groups):
        lvs, w = _run_group_as_worklists(lib, group, reverse)
        dv = _resident(lib, w)  # (geometry only: which launch this was)
        assert bool(dv.big) == big and dv.pf[0] != 0xffffffff
        up = uploaded(dv)
        for k, lv in enumerate(lvs):
            slot = _slot(k, len(lvs), reverse)
            assert (up.item[slot].kind, up.item[slot].part) == lv.item(lv.b.parts[0])[:2] and (slot - k) % 2 == (1 if reverse else 0)
            lv.assert_same_bits("launch %d, slot %d of %d" % (gi, slot, up.n))
            bodies.add(lv.case.body)
        _KEEP.pop()
    assert len(groups) > 1 and bodies >= set(W.ALL_BODIES) - ({"mha_bwd"} if not big else set())


@pytest.mark.parametrize("names", [("dense_70x77_k13_dead7_45_bias_relu", "fm_bwd_b37_n48_acc1"), ("dot_tri_bwd_k46_b11", "t16x64_kcrc_mask_k129"),
                                   ("final_bwd_b256_acc01", "dense_dx_three_problems_relu_mask")], ids=lambda n: "+".join(n))
def test_an_empty_item_between_two_live_ones(lib, names):
    """a GEMM item with M = 0 has no workgroups: its neighbours share its `first`, and the search must skip it in both orders"""
    for order in (names, names[::-1]):
        lvs = [live(lib, W.BY_NAME[n]) for n in order]
        for lv in lvs:
            lv.reset()
        (w,) = worklists([lvs[0].item(L.WL_WHOLE), _empty_gemm(), lvs[1].item(L.WL_WHOLE)])
        dv = _resident(lib, w)
        up = uploaded(dv)
        assert up.item[1].nblk == 0 and up.item[2].first == up.item[1].first == up.item[0].nblk
        _KEEP.pop()
        _run(lib, w)
        for lv in lvs:
            lv.assert_same_bits("beside an empty item")


def test_items_behind_65535_workgroups_are_found_through_the_table_in_memory(lib):
    """the packed table holds 16 bits per item: a launch of >= 65535 workgroups carries WL_PACKED_NONE and every workgroup searches the
    copy in memory — three small items of other kinds BEHIND the large copy have `first` >= 0xffff"""
    names = [W.BIG_COPY, "dense_dx_three_problems", "dot_tri_fwd_k17_b11", "final_bwd_b5_acc10"]
    lvs = [live(lib, W.BY_NAME[n]) for n in names]
    for resident in (False, True):
        for lv in lvs:
            lv.reset()
        (w,) = worklists([lv.item(L.WL_WHOLE) for lv in lvs])
        dv = _resident(lib, w)
        up = uploaded(dv)
        assert dv.pf[0] == 0xffffffff and dv.total_blocks >= 65535 + 3 and all(up.item[k].first >= 0xffff for k in (1, 2, 3))
        _run(lib, dv if resident else w)
        _KEEP.pop()
        for lv in lvs:
            lv.assert_same_bits("behind 65535 workgroups (%s)" % ("resident" if resident else "by value"))


# ---- form (e): NASREC_OP_PERSIST launches of independent items ------------------------------------------------------------------------
def _walks(kind, part, body):
    return kind == L.OP_FINAL_BWD or (kind == L.OP_GEMM and (part == L.WL_EPI or body.startswith("T")))


def _persist(lib, entries, hint):
    """entries: (kind, part, bytes, walks); tables as schedule.pack_persistent allocates them, PersistItem filled by hand, no dependencies"""
    n = len(entries)
    items = (L.PersistItem * n)()
    blob = bytearray()
    for k, (kind, part, b, walks) in enumerate(entries):
        it = items[k]
        it.kind, it.part, it.off, it.ndeps = kind, part, len(blob), 0
        it._pad[1] = hint if walks else 0
        blob += b
        blob += bytes((-len(blob)) % 16)
    hb = C.create_string_buffer(bytes(blob), len(blob))
    d = L.PersistDesc()
    d.kind, d.n, d.blob_bytes = L.OP_PERSIST, n, len(blob)
    d.host_items, d.host_blob = C.addressof(items), C.addressof(hb)
    cap = 4096

    def alloc(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    t = [alloc(C.sizeof(L.PersistItem) * n), alloc(len(blob) + 64), alloc(2 * cap), alloc(8 * n * (L.PS_SHARDS + 1) * L.PS_COUNTER_STRIDE),
         alloc(4 * n * L.PS_REPL * L.PS_FLAG_STRIDE), alloc(16)]
    d.items, d.blob, d.chunk_item, d.counters, d.flags, d.err = (x.data_ptr() for x in t)
    d.chunk_cap = cap
    torch.cuda.synchronize()
    L.check(lib.nasrec_persist_prepare(C.addressof(d)))
    up = (L.PersistItem * n).from_buffer_copy(t[0].cpu().numpy().tobytes())
    _run(lib, d)
    assert not bool(t[5].any()), "a wait of the persistent kernel ran out of its budget"
    return up, (items, hb, t)


@pytest.mark.parametrize("hint", [0, 3], ids=["a_workgroup_per_unit", "three_workgroups_walk"])
def test_items_of_persistent_launches_equal_their_stand_alone_launches(lib, hint):
    """form (e).  With the hint every item that walks runs on at most 3 workgroups, each taking several units through the same LDS buffer
    (the `for (u = vb; u < nblk; u += nwg)` loops of ps_run_item and the barrier between two units)."""
    cases = [c for c in W.CASES if c.name != W.BIG_COPY]  # (65552 workgroups: more than a launch's chunk table describes)
    walked = set()
    for g0 in range(0, len(cases), 12):
        lvs = [live(lib, c) for c in cases[g0:g0 + 12]]
        for lv in lvs:
            lv.reset()
        for stage in (0, 1):
            entries, who = [], []
            for lv in lvs:
                if stage < len(lv.b.parts):
                    kind, part, b = lv.item(lv.b.parts[stage])
                    entries.append((kind, part, b, True))  # (the launcher ignores the hint on the kinds that do not walk; checked below)
                    who.append(lv)
            if not entries:
                continue
            up, keep = _persist(lib, entries, hint)
            for k, lv in enumerate(who):
                body = W.body_of(up[k].kind, up[k].part, up[k].geom)
                if stage == len(lv.b.parts) - 1:
                    assert body == lv.case.body, (lv.case.name, body)
                if _walks(up[k].kind, up[k].part, body):
                    cap = hint if hint else (1 << 30 if body.startswith("T") else 512)  # (nasrec_persist_prepare: units per workgroup, then workgroups)
                    upw = -(-up[k].nblk // cap)
                    assert up[k]._pad[1] == -(-up[k].nblk // upw), (lv.case.name, up[k]._pad[1], up[k].nblk)
                    if hint and up[k].nblk > 3:
                        walked.add(body)
                else:
                    assert up[k]._pad[1] == up[k].nblk
        for lv in lvs:
            lv.assert_same_bits("persistent launch (hint %d)" % hint)
    if hint:
        tiles = {b for b in W.ALL_BODIES if b.startswith("T")}
        assert walked >= tiles | {"second_pass", "final_bwd"}, sorted((tiles | {"second_pass", "final_bwd"}) - walked)


# ---- the per-sample token-axis bodies on ragged shapes ----------------------------------------------------------------------------------
def _as_item(d):
    n = S.Node(d)
    b = S.item_bytes(n)
    assert b is not None
    one = L.WorklistDesc()
    one.kind, one.n = L.OP_WORKLIST, 1
    it = one.item[0]
    it.kind, it.part, it.off = d.kind, L.WL_WHOLE, 0
    C.memmove(C.addressof(one) + L.WorklistDesc.blob.offset, b, len(b))
    return one


@pytest.mark.parametrize("B,M,toks,bias,act", [(256, 39, [26, 72, 64], True, L.ACT_NONE), (3, 8, [26], False, L.ACT_RELU), (17, 64, [5, 16, 33], True, L.ACT_NONE),
                                               (256, 48, [26, 72, 64, 32], False, L.ACT_NONE), (64, 16, [72, 56], True, L.ACT_RELU)])
def test_token_forward_item_is_bit_identical(lib, B, M, toks, bias, act):
    g = torch.Generator(device="cuda").manual_seed(B + M)
    K = sum(toks)
    w = torch.randn(M, K, device="cuda", generator=g)
    xs = [torch.randn(B, t, 16, device="cuda", generator=g) for t in toks]
    bvec = torch.randn(M, device="cuda", generator=g) if bias else None
    outs = []
    for as_item in (False, True):
        y = torch.zeros(B, M, 16, device="cuda")
        d = L.GemmDesc()
        d.kind, d.amode, d.bmode, d.cmode, d.nseg, d.zmode, d.dims_in_use, d.splitk = L.OP_GEMM, L.AM_KC, L.AM_TOKR, L.CM_TOKJ, len(toks), 0, -1, 1
        d.act = act
        if bvec is not None:
            d.bias, d.bias_on_rows = bvec.data_ptr(), 1
        off = 0
        for q, t in enumerate(toks):
            s = d.seg[q]
            s.A, s.B, s.C, s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.Mvalid = w.data_ptr() + 4 * off, xs[q].data_ptr(), y.data_ptr(), M, B * 16, t, K, t * 16, M * 16, M
            off += t
        _run(lib, _as_item(d) if as_item else d)
        outs.append(y)
    ref = torch.einsum("mk,bke->bme", w.double(), torch.cat(xs, 1).double()) + (bvec.double().view(1, M, 1) if bvec is not None else 0.0)
    if act == L.ACT_RELU:
        ref = torch.relu(ref)
    assert float((outs[0].double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("B,rows_out,toks,acc", [(256, 32, [26, 72, 64], False), (5, 48, [72, 32], True), (256, 64, [26], False), (33, 16, [27, 5], True)])
def test_token_input_gradient_item_is_bit_identical(lib, B, rows_out, toks, acc, mask):
    """stand-alone kernel, worklist item (descriptor by value) and worklist item with the descriptor resident in device memory; with
    `mask` the gradient counts as 0 where the Linear's saved activation is <= 0 (the fused ReLU backward: Baux), which the
    wavefront-per-tile body applies as it loads the operand (round 6; the general tile before)"""
    g = torch.Generator(device="cuda").manual_seed(B * 3 + rows_out)
    K = sum(toks)
    w = torch.randn(rows_out, K, device="cuda", generator=g)       # the Linear's weight [out rows, tokens]
    dy = torch.randn(B, rows_out, 16, device="cuda", generator=g)  # gradient of its output
    act = torch.randn(B, rows_out, 16, device="cuda", generator=g)  # its saved activation (the mask)
    init = [torch.randn(B, t, 16, device="cuda", generator=g) for t in toks]
    outs = []
    for as_item in (False, True, "resident"):
        dx = [t.clone() for t in init]
        d = L.GemmDesc()
        d.kind, d.amode, d.bmode, d.cmode, d.nseg, d.zmode, d.dims_in_use, d.splitk = L.OP_GEMM, L.AM_RC, L.AM_TOKR, L.CM_TOKJ, len(toks), 1, -1, 1
        off = 0
        for q, t in enumerate(toks):
            s = d.seg[q]
            s.A, s.B, s.C, s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.Mvalid = w.data_ptr() + 4 * off, dy.data_ptr(), dx[q].data_ptr(), t, B * 16, rows_out, K, rows_out * 16, t * 16, t
            s.accumulate = 1 if acc else 0
            if mask:
                s.Baux = act.data_ptr()
            off += t
        _run(lib, d if not as_item else (_resident(lib, _as_item(d)) if as_item == "resident" else _as_item(d)))
        outs.append(dx)
    off = 0
    dz = dy.double() * ((act > 0).double() if mask else 1.0)
    for q, t in enumerate(toks):
        ref = torch.einsum("ik,bie->bke", w[:, off:off + t].double(), dz) + (init[q].double() if acc else 0.0)
        assert float((outs[0][q].double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
        assert torch.equal(outs[0][q], outs[1][q])
        assert torch.equal(outs[0][q], outs[2][q])
        off += t
