"""Every descriptor form the plan compiler emits is the form of a kernel case.

tests/op_forms.py compiles launch plans on the host — the six fixed sub-networks of nasrec_amd/configs, the 7-block full-path supernets
of both search spaces with LayerNorm, the same with SiLU and without LayerNorm, 24 sampled sub-paths, each at batch 256 and 2048, for
training and for inference — and reduces every operator descriptor of the forward and backward programs to its form: the properties that
select code or addressing in its kernel (NASREC_OP_GEMM included: its cases are the table of tests/gemm_cases.py, and
tests/test_gemm_forms_cpu.py carries the table of its forms).  A kind is either EXEMPT below (another test file owns it, named there) or known to
op_forms.form_of; every harvested form of a known kind must be the form of a case of tests/wl_cases.py (which runs stand-alone, as a
worklist item by value and resident, in mixed and in persistent launches: tests/test_worklist_items_gpu.py) or of the STANDALONE table
of tests/test_op_forms_gpu.py.  Nothing is skipped and no list of tolerated gaps exists: a planner change that emits a new form fails
here until a kernel case sets it.

The harvested forms and a case that covers each (held against the harvest by the last test of this module):

  act_bwd kc silu dims ld_dy_tight ld_z_tight ld_dz_tight    <- act_bwd_kc_silu_dims45_tight
  act_bwd tokr silu dims ld_dy_tight ld_z_tight ld_dz_tight  <- act_bwd_tokr_silu_dims7_tight
  act_bwd tokr silu dims ld_dy_wide ld_z_tight ld_dz_tight   <- act_bwd_tokr_silu_dims7_dy_in_slab
  copy_segs forward accumulate {seg/set} no_gap              <- copy_forward_accumulate_one_segment
  copy_segs forward overwrite {null/set} no_gap              <- copy_forward_zero_fill
  copy_segs forward overwrite {seg/set} no_gap               <- copy_4097x4096_unpacked_table
  copy_segs reverse overwrite {seg/set} no_gap               <- copy_reverse_one_segment
  dot_tri_bwd blocks1 ragged_block ld_out_tight              <- dot_tri_bwd_k9_b3_tight
  dot_tri_bwd blocks2 ragged_block ld_out_tight              <- dot_tri_bwd_k17_b5_tight
  dot_tri_bwd blocks3 ragged_block ld_out_tight              <- dot_tri_bwd_k33_b3_tight
  dot_tri_fwd blocks1 ragged_block ld_out_tight              <- dot_tri_fwd_k9_b3_tight
  dot_tri_fwd blocks2 ragged_block ld_out_tight              <- dot_tri_fwd_k17_b5_tight
  dot_tri_fwd blocks3 ragged_block ld_out_tight              <- dot_tri_fwd_k33_b3_tight
  fm_bwd no_add accumulate ldx_tight ld_ix_tight n<=32       <- fm_bwd_b5_n16_tight_acc1
  fm_bwd no_add accumulate ldx_tight ld_ix_tight n>32        <- fm_bwd_b5_n48_tight_acc1
  fm_bwd no_add accumulate ldx_wide ld_ix_tight n<=32        <- fm_bwd_b5_n16_slab_acc1
  fm_bwd no_add accumulate ldx_wide ld_ix_tight n>32         <- fm_bwd_b5_n48_slab_acc1
  fm_fwd add overwrite ldx_tight ld_ix_tight n<=32           <- fm_fwd_b1_n16_add_tight
  fm_fwd add overwrite ldx_tight ld_ix_tight n>32            <- fm_fwd_b1_n48_add_tight
  fm_fwd no_add overwrite ldx_tight ld_ix_tight n<=32        <- fm_fwd_b5_n16_tight
  fm_fwd no_add overwrite ldx_tight ld_ix_tight n>32         <- fm_fwd_b5_n48_tight
  fm_fwd no_add overwrite ldx_wide ld_ix_tight n<=32         <- fm_fwd_b5_n16_slab
  fm_fwd no_add overwrite ldx_wide ld_ix_tight n>32          <- fm_fwd_b5_n48_slab
  gate_bwd nseg1 {dr/acc/r} ld_dout_tight ld_g_tight ld_dz_tight gap <- gate_21x32_one_segment
  gate_bwd nseg1 {dr/acc/r} ld_dout_wide ld_g_wide ld_dz_wide gap <- gate_5x29_head_acc_wide
  gate_bwd nseg1 {dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight gap <- gate_5x29_head_set_tight
  gate_bwd nseg1 {dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x29_all_set_tight
  gate_bwd nseg1 {dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide gap <- gate_5x29_head_set_wide
  gate_bwd nseg1 {no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight gap <- gate_5x29_head_no_dr_tight
  gate_bwd nseg1 {no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x13_all_no_dr_tight
  gate_bwd nseg1 {no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide gap <- gate_5x29_head_no_dr_wide
  gate_bwd nseg1 {no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide no_gap <- gate_5x13_all_no_dr_wide
  gate_bwd nseg2 {dr/acc/r,no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x21_2_segments_tight
  gate_bwd nseg2 {dr/acc/r,no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide no_gap <- gate_5x21_2_segments_wide
  gate_bwd nseg3 {dr/acc/r,no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x29_3_segments_tight
  gate_bwd nseg3 {dr/acc/r,no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide no_gap <- gate_5x29_3_segments_wide
  gate_bwd nseg4 {dr/acc/r,no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x37_4_segments_tight
  gate_bwd nseg4 {dr/acc/r,no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide no_gap <- gate_5x37_4_segments_wide
  gate_bwd nseg5 {dr/acc/r,no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x45_5_segments_tight
  gate_bwd nseg5 {dr/acc/r,no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide no_gap <- gate_5x45_5_segments_wide
  gate_bwd nseg6 {dr/acc/r,no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x53_6_segments_tight
  gate_bwd nseg6 {dr/acc/r,no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide no_gap <- gate_5x53_6_segments_wide
  gate_bwd nseg7 {dr/acc/r,no_dr/set/r} ld_dout_tight ld_g_tight ld_dz_tight no_gap <- gate_5x61_7_segments_tight
  gate_bwd nseg7 {dr/acc/r,no_dr/set/r} ld_dout_wide ld_g_wide ld_dz_wide no_gap <- gate_5x61_7_segments_wide
  memset flat kernel no_tail one_pass                        <- memset_flat_98304
  memset flat kernel no_tail strided                         <- memset_flat_2359296_strided
  mha_bwd blocks1 full_block ldx_tight ldo_wide dims_none no_masked_block saved shared_partials <- mha_bwd_n16_d-1_b5_slab_shared
  mha_bwd blocks3 full_block ldx_tight ldo_tight dims_none no_masked_block saved shared_partials <- mha_bwd_n48_d-1_b3_own_shared
  mha_bwd blocks3 full_block ldx_tight ldo_wide dims_none no_masked_block saved shared_partials <- mha_bwd_n48_d-1_b3_slab_shared
  mha_bwd blocks4 full_block ldx_tight ldo_tight dims_none no_masked_block saved shared_partials <- mha_bwd_n64_d64_b5_own_shared
  mha_bwd blocks4 full_block ldx_tight ldo_wide dims_mid masked_block saved shared_partials <- mha_bwd_n64_d40_b5_slab_shared
  mha_bwd blocks4 full_block ldx_tight ldo_wide dims_none no_masked_block saved shared_partials <- mha_bwd_n64_d-1_b3_slab_shared
  mha_fwd blocks1 full_block ldx_tight ldo_wide dims_none no_masked_block saved own_partials <- mha_fwd_n16_d-1_b5_slab_saved
  mha_fwd blocks1 full_block ldx_tight ldo_wide dims_none no_masked_block unsaved own_partials <- mha_fwd_n16_d-1_b5_slab
  mha_fwd blocks3 full_block ldx_tight ldo_tight dims_none no_masked_block saved own_partials <- mha_fwd_n48_d-1_b3_own_saved
  mha_fwd blocks3 full_block ldx_tight ldo_tight dims_none no_masked_block unsaved own_partials <- mha_fwd_n48_d-1_b3_own
  mha_fwd blocks3 full_block ldx_tight ldo_wide dims_none no_masked_block saved own_partials <- mha_fwd_n48_d-1_b3_slab_saved
  mha_fwd blocks3 full_block ldx_tight ldo_wide dims_none no_masked_block unsaved own_partials <- mha_fwd_n48_d-1_b3_slab
  mha_fwd blocks4 full_block ldx_tight ldo_tight dims_none no_masked_block saved own_partials <- mha_fwd_n64_d64_b5_own_saved
  mha_fwd blocks4 full_block ldx_tight ldo_tight dims_none no_masked_block unsaved own_partials <- mha_fwd_n64_d64_b5_own
  mha_fwd blocks4 full_block ldx_tight ldo_wide dims_mid masked_block saved own_partials <- mha_fwd_n64_d40_b5_slab_saved
  mha_fwd blocks4 full_block ldx_tight ldo_wide dims_mid masked_block unsaved own_partials <- mha_fwd_n64_d40_b5_slab
  mha_fwd blocks4 full_block ldx_tight ldo_wide dims_none no_masked_block saved own_partials <- mha_fwd_n64_d-1_b3_slab_saved
  mha_fwd blocks4 full_block ldx_tight ldo_wide dims_none no_masked_block unsaved own_partials <- mha_fwd_n64_d-1_b3_slab
  reduce_rows r16-63 no_remainder ndst2-16 ld_tight no_null_dst no_gap <- reduce_r16_c34_2dst_tight
  reduce_rows r64-255 no_remainder ndst2-16 ld_tight no_null_dst no_gap <- reduce_r64_c34_2dst_tight
  reduce_rows r>=256 no_remainder ndst17-48 ld_tight no_null_dst no_gap <- reduce_r256_c72_24dst_tight
  reduce_rows r>=256 no_remainder ndst2-16 ld_tight no_null_dst no_gap <- reduce_r256_c1696_mha_tight
"""
import os

import pytest

import gemm_cases
import op_forms as F
import test_op_forms_gpu as G
import wl_cases as W
from nasrec_amd import _lib as L
from nasrec_amd import schedule as S

HERE = os.path.dirname(os.path.abspath(__file__))

# kinds whose kernels other test files hold to their own references: kind -> the file that owns it
EXEMPT = {
    L.OP_LAYERNORM_FWD: "test_layernorm_kernel_gpu.py",
    L.OP_LAYERNORM_BWD: "test_layernorm_kernel_gpu.py",
    L.OP_WORKLIST: "test_worklist_items_gpu.py",
    L.OP_WORKLIST_DEV: "test_worklist_items_gpu.py",
    L.OP_PERSIST: "test_worklist_items_gpu.py",
    L.OP_SPLITK_EPILOGUES: "test_ops_gpu.py",
    # the optimizer kinds
    L.OP_ADAGRAD_DENSE: "test_ops_gpu.py",
    L.OP_ADAGRAD_ROWS: "test_ops_gpu.py",
    L.OP_OPT_REDUCE: "test_ops_gpu.py",
    L.OP_OPT_APPLY: "test_ops_gpu.py",
    L.OP_OPT_REDUCE2: "test_dedup_split_gpu.py",
    L.OP_WEIGHT_DECAY: "test_weight_decay_kernel_gpu.py",
    L.OP_OPT_MOMENTS: "test_fused_optimizers_kernel_gpu.py",
    L.OP_LAST_LAYER_STEP: "test_last_layer_step_kernel_gpu.py",
    L.OP_WEIGHT_EMA: "test_weight_ema_kernel_gpu.py",
    # the embedding kinds
    L.OP_EMBED_GATHER: "test_ops_gpu.py",
    L.OP_EMB_DEDUP: "test_ops_gpu.py",
    L.OP_DEDUP_IDS: "test_dedup_split_gpu.py",
    # staging and the loss
    L.OP_STAGE_INPUTS: "test_ops_gpu.py",
    L.OP_BCE: "test_ops_gpu.py",
    L.OP_SUMSQ: "test_ops_gpu.py",
    L.OP_CLIP_COEF: "test_ops_gpu.py",
}


EVERY = []


@pytest.fixture(scope="module")
def harvested():
    del EVERY[:]
    return F.harvest(every=EVERY)


def case_forms():
    """form -> name of the first kernel case that sets it (the cases are built on the host: no pointer is dereferenced)"""
    out = {}
    for c in W.CASES:
        b = c.build("cpu")
        for d in list(b.setup) + [b.desc]:
            if d.kind in F.FORM_FN:
                out.setdefault(F.form_of(d), c.name)
    for name, fn in G.STANDALONE:
        for d in fn("cpu").descs:
            if d.kind in F.FORM_FN:
                out.setdefault(F.form_of(d), name)
    for c in gemm_cases.CASES:  # (NASREC_OP_GEMM: tests/test_gemm_forms_cpu.py carries their table)
        out.setdefault(c.form(), c.name)
    return out


@pytest.fixture(scope="module")
def covered():
    return case_forms()


def show(form):
    return " ".join(str(p) if not isinstance(p, tuple) else "{" + ",".join("/".join(s) for s in p) + "}" for p in form)


def test_every_exempt_kind_names_the_test_file_that_owns_it():
    assert not set(EXEMPT) & set(F.FORM_FN)
    for kind, owner in EXEMPT.items():
        path = os.path.join(HERE, owner)
        assert os.path.exists(path), owner
        assert ("OP_" + F.KIND_NAME[kind].upper()) in open(path).read(), (F.KIND_NAME[kind], owner)


def test_every_harvested_kind_is_exempt_or_known_to_form_of(harvested):
    _, unknown = harvested
    stray = sorted(F.KIND_NAME.get(k, str(k)) for k in unknown if k not in EXEMPT)
    assert not stray, "the planner emits kinds that are neither exempt nor known to op_forms.form_of: %s" % stray


def test_every_harvested_form_is_the_form_of_a_kernel_case(harvested, covered):
    forms, _ = harvested
    uncovered = sorted(show(f) for f in forms if f not in covered)
    assert not uncovered, "forms the planner emits and no kernel case sets:\n  " + "\n  ".join(uncovered)


def test_the_harvest_contains_the_forms_the_planner_is_known_to_emit(harvested):
    """... so that an empty or a crippled harvest does not pass for full coverage"""
    forms, _ = harvested
    fs = list(forms)

    def some(kind, *props):
        return any(f[0] == kind and all(p in f for p in props) for f in fs)

    assert len(fs) >= 60
    assert some("mha_fwd", "ldo_wide") and some("mha_bwd", "ldo_wide", "shared_partials")
    assert not some("mha_bwd", "own_partials")  # (every training plan shares one partial buffer)
    assert some("fm_fwd", "add", "overwrite", "ldx_tight", "ld_ix_tight")
    assert any(f[0] == "gate_bwd" and "nseg7" in f and any(s[0] == "no_dr" for s in f[2]) for f in fs)
    assert some("gate_bwd", "ld_dout_wide", "ld_g_wide", "ld_dz_wide")
    assert some("copy_segs", "forward", "accumulate")
    assert any(d.kind == L.OP_REDUCE_ROWS and d.ndst == L.REDUCE_MAX_DST for d in EVERY) and some("reduce_rows", "ndst17-48")
    assert some("reduce_rows", "r16-63") and some("reduce_rows", "r64-255") and some("reduce_rows", "r>=256")
    assert some("act_bwd", "kc", "silu", "dims") and some("act_bwd", "tokr", "silu", "dims")
    for kind in ("dot_tri_fwd", "dot_tri_bwd"):
        for blocks in ("blocks1", "blocks2", "blocks3"):
            assert some(kind, blocks, "ld_out_tight"), (kind, blocks)
    assert some("memset", "flat")


def test_the_cases_the_issue_of_this_table_asked_for_have_their_forms(covered):
    """the forms no planner emits today but a kernel case must keep setting: wide strides on both sides of the Transformer, the widest
    reduction with a NULL destination and a column gap, the activation backward with three different wide strides"""
    fs = list(covered)
    assert any(f[0] == "mha_bwd" and "ldx_wide" in f and "ldo_wide" in f and "shared_partials" in f for f in fs)
    assert any(f[0] == "reduce_rows" and "ndst17-48" in f and "null_dst" in f and "gap" in f and "ld_wide" in f and "remainder" in f for f in fs)
    assert any(f[0] == "gate_bwd" and "nseg7" in f and "gap" in f and any(s[2] == "no_r" for s in f[2]) for f in fs)
    for mode in ("kc", "tokr"):
        for act in ("relu", "silu", "sigmoid"):
            assert any(f[:3] == ("act_bwd", mode, act) and "ld_dz_wide" in f for f in fs)
    assert F.reduce_tiers(64) == (False, True, False) and F.reduce_tiers(300) == (True, False, True) and F.reduce_tiers(16) == (False, False, True)


@pytest.mark.parametrize("name", G.WIDE_REDUCES)
def test_a_reduction_of_more_than_16_destinations_is_refused_as_an_item_by_the_destination_rule_alone(name):
    """schedule.item_bytes accepts NASREC_OP_REDUCE_ROWS with 1 .. WL_REDUCE_DST destinations (the compact WlReduce): the same
    descriptor cut to 16 destinations is an item, with 17 it is not — so these run stand-alone only (tests/test_op_forms_gpu.py)"""
    d = dict(G.STANDALONE)[name]("cpu").descs[0]
    assert d.ndst > L.WL_REDUCE_DST and S.item_bytes(S.Node(d)) is None
    d.ndst = L.WL_REDUCE_DST
    assert S.item_bytes(S.Node(d)) is not None
    d.ndst = L.WL_REDUCE_DST + 1
    assert S.item_bytes(S.Node(d)) is None


def coverage_table(forms, covered):
    """(without the NASREC_OP_GEMM forms: tests/test_gemm_forms_cpu.py holds their table against the same harvest)"""
    return ["  %-58s <- %s" % (show(f), covered[f]) for f in sorted(forms, key=show) if f[0] != "gemm"]


def test_the_table_in_this_modules_docstring_is_the_harvest(harvested, covered):
    forms, _ = harvested
    rows = [line.rstrip() for line in __doc__.splitlines() if " <- " in line]
    assert rows == [r.rstrip() for r in coverage_table(forms, covered)]
