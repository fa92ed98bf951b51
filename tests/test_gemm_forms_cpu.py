"""Every NASREC_OP_GEMM descriptor form the plan compiler emits is the form of a GEMM kernel case.

tests/op_forms.py compiles launch plans on the host (the plans of tests/test_op_forms_cpu.py: the fixed sub-networks, the full-path
supernets, SiLU supernets and 24 sampled sub-paths, at batch 256 and 2048, for training and for inference) and reduces every GEMM
descriptor to its form (op_forms._gemm): the kernel family and kernel name the library itself answers, the general template's tile
configuration and body or the branch the family's launcher takes, the operand binding, k-segments or z-problems, whether the k-segments
disagree, the split-K class, and the predicates the five copies of the epilogue are written in.  Every harvested form must be the form of
a case of tests/gemm_cases.py or of a GEMM case of tests/wl_cases.py; tests/test_gemm_forms_gpu.py runs the former against fp64,
tests/test_worklist_items_gpu.py the latter.  Nothing is skipped and no list of tolerated gaps exists.

The harvest holds 324 GEMM forms.  The words of a form: family, kernel, configuration, binding, k1 / kN (one / several k-segments of one
product) or z1 / zN (a batch of one / several problems), then what is not the default (uniform, s1 = unsplit, act_none, no_bias, no_mask,
overwrite, no_pre, no_z, no_sact, no_gate, no_ones, aux_none, mvalid=M, live_A, highest).  The harvested forms and a case that covers each
(held against the harvest by the last test of this module; a case of tests/gemm_cases.py is named by its words):

  fast gemm_fast_kernel no_ones_template.acc_in_tile KC.RC.PLAIN z1 accumulate <- fast_no_ones_template_acc_in_tile_KC_RC_PLAIN_z1_accumulate
  fast gemm_fast_kernel no_ones_template.acc_in_tile KC.RC.PLAIN zN accumulate <- fast_no_ones_template_acc_in_tile_KC_RC_PLAIN_zN_accumulate
  fast gemm_fast_kernel no_ones_template.acc_in_tile RC.RC.PLAIN zN accumulate <- fast_no_ones_template_acc_in_tile_RC_RC_PLAIN_zN_accumulate
  fast gemm_fast_kernel no_ones_template.acc_in_tile+plain KC.RC.PLAIN zN acc_mixed <- fast_no_ones_template_acc_in_tile_and_plain_KC_RC_PLAIN_zN_acc_mixed
  fast gemm_fast_kernel no_ones_template.nread0 KC.KC.PLAIN kN bias_cols mask_cols <- fast_no_ones_template_nread0_KC_KC_PLAIN_kN_bias_cols_mask_cols
  fast gemm_fast_kernel no_ones_template.nread1 KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap <- fast_no_ones_template_nread1_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_gap
  fast gemm_fast_kernel no_ones_template.nread1 KC.KC.PLAIN kN bias_cols mask_cols accumulate <- fast_no_ones_template_nread1_KC_KC_PLAIN_kN_bias_cols_mask_cols_accumulate
  fast gemm_fast_kernel no_ones_template.nread1 KC.KC.PLAIN kN sigmoid bias_cols save_act gate_covering <- fast_no_ones_template_nread1_KC_KC_PLAIN_kN_sigmoid_bias_cols_save_act_gate_covering
  fast gemm_fast_kernel no_ones_template.plain KC.KC.PLAIN kN <- fast_no_ones_template_plain_KC_KC_PLAIN_kN
  fast gemm_fast_kernel no_ones_template.plain KC.RC.PLAIN z1 <- fast_no_ones_template_plain_KC_RC_PLAIN_z1
  fast gemm_fast_kernel no_ones_template.plain KC.RC.PLAIN zN <- fast_no_ones_template_plain_KC_RC_PLAIN_zN
  fast gemm_fast_kernel no_ones_template.plain RC.RC.PLAIN zN <- fast_no_ones_template_plain_RC_RC_PLAIN_zN
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN k1 split <- fast_no_ones_template_second_pass_KC_KC_PLAIN_k1_split
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN k1 split bias_cols <- fast_no_ones_template_second_pass_KC_KC_PLAIN_k1_split_bias_cols
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN k1 split bias_cols mask_cols <- fast_no_ones_template_second_pass_KC_KC_PLAIN_k1_split_bias_cols_mask_cols
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN k1 split bias_cols mask_cols accumulate <- fast_no_ones_template_second_pass_KC_KC_PLAIN_k1_split_bias_cols_mask_cols_accumulate
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN k1 split sigmoid bias_cols save_act gate_gap <- fast_no_ones_template_second_pass_KC_KC_PLAIN_k1_split_sigmoid_bias_cols_save_act_gate_gap
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN k1 split silu bias_cols mask_cols save_z <- fast_no_ones_template_second_pass_KC_KC_PLAIN_k1_split_silu_bias_cols_mask_cols_save_z
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split accumulate <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_accumulate
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split bias_cols <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_bias_cols
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split bias_cols mask_cols <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_bias_cols_mask_cols
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split bias_cols mask_cols accumulate <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_bias_cols_mask_cols_accumulate
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split mask_cols accumulate <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_mask_cols_accumulate
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split relu bias_cols <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_relu_bias_cols
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split sigmoid bias_cols save_act gate_covering <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_sigmoid_bias_cols_save_act_gate_covering
  fast gemm_fast_kernel no_ones_template.second_pass KC.KC.PLAIN kN split silu bias_cols mask_cols save_z <- fast_no_ones_template_second_pass_KC_KC_PLAIN_kN_split_silu_bias_cols_mask_cols_save_z
  fast gemm_fast_kernel no_ones_template.second_pass KC.RC.PLAIN z1 split <- fast_no_ones_template_second_pass_KC_RC_PLAIN_z1_split
  fast gemm_fast_kernel no_ones_template.second_pass KC.RC.PLAIN z1 split accumulate <- fast_no_ones_template_second_pass_KC_RC_PLAIN_z1_split_accumulate
  fast gemm_fast_kernel no_ones_template.second_pass KC.RC.PLAIN zN split <- fast_no_ones_template_second_pass_KC_RC_PLAIN_zN_split
  fast gemm_fast_kernel no_ones_template.second_pass KC.RC.PLAIN zN split acc_mixed <- fast_no_ones_template_second_pass_KC_RC_PLAIN_zN_split_acc_mixed
  fast gemm_fast_kernel no_ones_template.second_pass KC.RC.PLAIN zN split accumulate <- fast_no_ones_template_second_pass_KC_RC_PLAIN_zN_split_accumulate
  fast gemm_fast_kernel no_ones_template.second_pass RC.RC.PLAIN z1 split <- fast_no_ones_template_second_pass_RC_RC_PLAIN_z1_split
  fast gemm_fast_kernel no_ones_template.second_pass RC.RC.PLAIN z1 split accumulate <- fast_no_ones_template_second_pass_RC_RC_PLAIN_z1_split_accumulate
  fast gemm_fast_kernel no_ones_template.second_pass RC.RC.PLAIN z1 split accumulate mvalid<M <- fast_no_ones_template_second_pass_RC_RC_PLAIN_z1_split_accumulate_mvalid_lt_M
  fast gemm_fast_kernel no_ones_template.second_pass RC.RC.PLAIN zN split <- fast_no_ones_template_second_pass_RC_RC_PLAIN_zN_split
  fast gemm_fast_kernel no_ones_template.second_pass RC.RC.PLAIN zN split accumulate mvalid<M <- fast_no_ones_template_second_pass_RC_RC_PLAIN_zN_split_accumulate_mvalid_lt_M
  fast gemm_fast_kernel no_ones_template.second_pass RC.RC.PLAIN zN split_deferred <- fast_no_ones_template_second_pass_RC_RC_PLAIN_zN_split_deferred
  fast gemm_fast_kernel ones_template.full_ones RC.RC.PLAIN zN ones_own_rowsum mvalid<M <- fast_ones_template_full_ones_RC_RC_PLAIN_zN_ones_own_rowsum_mvalid_lt_M
  fast gemm_fast_kernel ones_template.full_ones+plain RC.RC.PLAIN zN ones_own_rowsum <- fast_ones_template_full_ones_and_plain_RC_RC_PLAIN_zN_ones_own_rowsum
  fast gemm_fast_kernel ones_template.full_ones+plain RC.RC.PLAIN zN ones_own_rowsum mvalid<M <- fast_ones_template_full_ones_and_plain_RC_RC_PLAIN_zN_ones_own_rowsum_mvalid_lt_M
  fast gemm_fast_kernel ones_template.second_pass RC.RC.PLAIN z1 split ones_own_rowsum <- fast_ones_template_second_pass_RC_RC_PLAIN_z1_split_ones_own_rowsum
  fast gemm_fast_kernel ones_template.second_pass RC.RC.PLAIN zN split ones_own_rowsum <- fast_ones_template_second_pass_RC_RC_PLAIN_zN_split_ones_own_rowsum
  fast gemm_fast_kernel ones_template.second_pass RC.RC.PLAIN zN split ones_own_rowsum mvalid<M <- fast_ones_template_second_pass_RC_RC_PLAIN_zN_split_ones_own_rowsum_mvalid_lt_M
  fast gemm_fast_kernel ones_template.second_pass RC.RC.PLAIN zN split_deferred ones_own_rowsum <- fast_ones_template_second_pass_RC_RC_PLAIN_zN_split_deferred_ones_own_rowsum
  fast gemm_fast_kernel ones_template.second_pass RC.RC.PLAIN zN split_deferred ones_own_rowsum mvalid<M <- fast_ones_template_second_pass_RC_RC_PLAIN_zN_split_deferred_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN k1 bias_cols <- general_16x64_deep_ring_KC_KC_PLAIN_k1_bias_cols
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering <- general_16x64_deep_ring_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_covering
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap <- general_16x64_deep_ring_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_gap
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN k1 split <- general_16x64_deep_ring_KC_KC_PLAIN_k1_split
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN k1 split bias_cols <- general_16x64_deep_ring_KC_KC_PLAIN_k1_split_bias_cols
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN k1 split relu bias_cols <- general_16x64_deep_ring_KC_KC_PLAIN_k1_split_relu_bias_cols
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN kN bias_cols <- general_16x64_deep_ring_KC_KC_PLAIN_kN_bias_cols
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN kN relu bias_cols <- wl_cases.dense_33x16_k260_leaves_the_body
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN kN split <- general_16x64_deep_ring_KC_KC_PLAIN_kN_split
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN kN split bias_cols <- general_16x64_deep_ring_KC_KC_PLAIN_kN_split_bias_cols
  general gemm_kernel 16x64.deep.ring KC.KC.PLAIN kN split relu bias_cols <- general_16x64_deep_ring_KC_KC_PLAIN_kN_split_relu_bias_cols
  general gemm_kernel 16x64.deep.ring KC.RC.PLAIN z1 <- general_16x64_deep_ring_KC_RC_PLAIN_z1
  general gemm_kernel 16x64.deep.ring KC.RC.PLAIN z1 accumulate <- general_16x64_deep_ring_KC_RC_PLAIN_z1_accumulate
  general gemm_kernel 16x64.deep.ring KC.RC.PLAIN z1 split <- general_16x64_deep_ring_KC_RC_PLAIN_z1_split
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN z1 split <- general_16x64_deep_ring_RC_RC_PLAIN_z1_split
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN z1 split accumulate <- general_16x64_deep_ring_RC_RC_PLAIN_z1_split_accumulate
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum <- general_16x64_deep_ring_RC_RC_PLAIN_z1_split_ones_own_rowsum
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum mvalid<M <- general_16x64_deep_ring_RC_RC_PLAIN_z1_split_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN z1 split_deferred <- general_16x64_deep_ring_RC_RC_PLAIN_z1_split_deferred
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN z1 split_deferred ones_own_rowsum mvalid<M <- general_16x64_deep_ring_RC_RC_PLAIN_z1_split_deferred_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN zN split <- general_16x64_deep_ring_RC_RC_PLAIN_zN_split
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN zN split ones_own_rowsum <- general_16x64_deep_ring_RC_RC_PLAIN_zN_split_ones_own_rowsum
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN zN split_deferred <- general_16x64_deep_ring_RC_RC_PLAIN_zN_split_deferred
  general gemm_kernel 16x64.deep.ring RC.RC.PLAIN zN split_deferred ones_own_rowsum <- general_16x64_deep_ring_RC_RC_PLAIN_zN_split_deferred_ones_own_rowsum
  general gemm_kernel 16x64.deep.ring TOKK.TOKK.PLAIN z1 split ones_own_rowsum <- general_16x64_deep_ring_TOKK_TOKK_PLAIN_z1_split_ones_own_rowsum
  general gemm_kernel 16x64.deep.ring TOKK.TOKK.PLAIN z1 split_deferred <- general_16x64_deep_ring_TOKK_TOKK_PLAIN_z1_split_deferred
  general gemm_kernel 16x64.deep.ring TOKK.TOKK.PLAIN zN split ones_own_rowsum <- general_16x64_deep_ring_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  general gemm_kernel 16x64.deep.ring TOKK.TOKK.PLAIN zN split_deferred <- general_16x64_deep_ring_TOKK_TOKK_PLAIN_zN_split_deferred
  general gemm_kernel 16x64.deep.ring TOKK.TOKK.PLAIN zN split_deferred ones_own_rowsum mvalid<M <- general_16x64_deep_ring_TOKK_TOKK_PLAIN_zN_split_deferred_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel 16x64.deep.ring_aux KC.RC.PLAIN z1 aux_A <- general_16x64_deep_ring_aux_KC_RC_PLAIN_z1_aux_A
  general gemm_kernel 16x64.deep.ring_aux KC.RC.PLAIN z1 split accumulate aux_A <- general_16x64_deep_ring_aux_KC_RC_PLAIN_z1_split_accumulate_aux_A
  general gemm_kernel 16x64.deep.ring_aux RC.RC.PLAIN z1 split ones_own_rowsum aux_A <- general_16x64_deep_ring_aux_RC_RC_PLAIN_z1_split_ones_own_rowsum_aux_A
  general gemm_kernel 16x64.deep.ring_aux TOKK.TOKK.PLAIN z1 split ones_own_rowsum aux_A <- general_16x64_deep_ring_aux_TOKK_TOKK_PLAIN_z1_split_ones_own_rowsum_aux_A
  general gemm_kernel 16x64.deep.ring_aux TOKK.TOKK.PLAIN zN split ones_own_rowsum aux_A <- general_16x64_deep_ring_aux_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum_aux_A
  general gemm_kernel 16x64.shallow.ring KC.KC.PLAIN k1 <- general_16x64_shallow_ring_KC_KC_PLAIN_k1
  general gemm_kernel 16x64.shallow.ring KC.KC.PLAIN k1 bias_cols <- general_16x64_shallow_ring_KC_KC_PLAIN_k1_bias_cols
  general gemm_kernel 16x64.shallow.ring KC.KC.PLAIN k1 bias_cols accumulate <- general_16x64_shallow_ring_KC_KC_PLAIN_k1_bias_cols_accumulate
  general gemm_kernel 16x64.shallow.ring KC.KC.PLAIN k1 bias_cols pre_add <- general_16x64_shallow_ring_KC_KC_PLAIN_k1_bias_cols_pre_add
  general gemm_kernel 16x64.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering <- general_16x64_shallow_ring_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_covering
  general gemm_kernel 16x64.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap <- general_16x64_shallow_ring_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_gap
  general gemm_kernel 16x64.shallow.ring KC.KC.PLAIN kN bias_cols <- general_16x64_shallow_ring_KC_KC_PLAIN_kN_bias_cols
  general gemm_kernel 16x64.shallow.ring KC.RC.PLAIN z1 <- general_16x64_shallow_ring_KC_RC_PLAIN_z1
  general gemm_kernel 16x64.shallow.ring KC.RC.PLAIN z1 accumulate <- general_16x64_shallow_ring_KC_RC_PLAIN_z1_accumulate
  general gemm_kernel 16x64.shallow.ring KC.RC.PLAIN zN accumulate <- general_16x64_shallow_ring_KC_RC_PLAIN_zN_accumulate
  general gemm_kernel 64x16.deep.ring KC.KC.PLAIN k1 bias_cols <- general_64x16_deep_ring_KC_KC_PLAIN_k1_bias_cols
  general gemm_kernel 64x16.deep.ring KC.KC.PLAIN k1 relu bias_cols <- wl_cases.dense_17x36_k128_eight_steps
  general gemm_kernel 64x16.deep.ring KC.RC.PLAIN z1 <- general_64x16_deep_ring_KC_RC_PLAIN_z1
  general gemm_kernel 64x16.deep.ring KC.RC.PLAIN z1 accumulate <- general_64x16_deep_ring_KC_RC_PLAIN_z1_accumulate
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ k1 <- general_64x16_deep_ring_KC_TOKR_TOKJ_k1
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ k1 bias_rows <- general_64x16_deep_ring_KC_TOKR_TOKJ_k1_bias_rows
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ k1 bias_rows mask_rows <- general_64x16_deep_ring_KC_TOKR_TOKJ_k1_bias_rows_mask_rows
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ k1 relu bias_rows <- general_64x16_deep_ring_KC_TOKR_TOKJ_k1_relu_bias_rows
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ k1 silu bias_rows mask_rows save_z <- general_64x16_deep_ring_KC_TOKR_TOKJ_k1_silu_bias_rows_mask_rows_save_z
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ kN <- general_64x16_deep_ring_KC_TOKR_TOKJ_kN
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ kN bias_rows <- general_64x16_deep_ring_KC_TOKR_TOKJ_kN_bias_rows
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ kN bias_rows mask_rows <- general_64x16_deep_ring_KC_TOKR_TOKJ_kN_bias_rows_mask_rows
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ kN relu bias_rows <- wl_cases.token_fwd_17x64_tok5_16_33
  general gemm_kernel 64x16.deep.ring KC.TOKR.TOKJ kN silu bias_rows mask_rows save_z <- general_64x16_deep_ring_KC_TOKR_TOKJ_kN_silu_bias_rows_mask_rows_save_z
  general gemm_kernel 64x16.deep.ring RC.RC.PLAIN z1 split <- general_64x16_deep_ring_RC_RC_PLAIN_z1_split
  general gemm_kernel 64x16.deep.ring RC.RC.PLAIN z1 split accumulate <- general_64x16_deep_ring_RC_RC_PLAIN_z1_split_accumulate
  general gemm_kernel 64x16.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum <- general_64x16_deep_ring_RC_RC_PLAIN_z1_split_ones_own_rowsum
  general gemm_kernel 64x16.deep.ring RC.RC.PLAIN z1 split_deferred ones_own_rowsum <- general_64x16_deep_ring_RC_RC_PLAIN_z1_split_deferred_ones_own_rowsum
  general gemm_kernel 64x16.deep.ring RC.RC.PLAIN zN split ones_own_rowsum <- general_64x16_deep_ring_RC_RC_PLAIN_zN_split_ones_own_rowsum
  general gemm_kernel 64x16.deep.ring RC.TOKR.TOKJ k1 accumulate <- general_64x16_deep_ring_RC_TOKR_TOKJ_k1_accumulate
  general gemm_kernel 64x16.deep.ring RC.TOKR.TOKJ kN <- wl_cases.t64x16_rcrc_plain_k65
  general gemm_kernel 64x16.deep.ring RC.TOKR.TOKJ z1 accumulate <- general_64x16_deep_ring_RC_TOKR_TOKJ_z1_accumulate
  general gemm_kernel 64x16.deep.ring TOKK.TOKK.PLAIN z1 split ones_own_rowsum <- general_64x16_deep_ring_TOKK_TOKK_PLAIN_z1_split_ones_own_rowsum
  general gemm_kernel 64x16.deep.ring TOKK.TOKK.PLAIN zN split ones_own_rowsum <- general_64x16_deep_ring_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  general gemm_kernel 64x16.deep.ring_aux KC.RC.PLAIN z1 accumulate aux_A <- general_64x16_deep_ring_aux_KC_RC_PLAIN_z1_accumulate_aux_A
  general gemm_kernel 64x16.deep.ring_aux KC.RC.PLAIN zN acc_mixed aux_A <- general_64x16_deep_ring_aux_KC_RC_PLAIN_zN_acc_mixed_aux_A
  general gemm_kernel 64x16.deep.ring_aux KC.RC.PLAIN zN aux_A <- general_64x16_deep_ring_aux_KC_RC_PLAIN_zN_aux_A
  general gemm_kernel 64x16.deep.ring_aux RC.RC.PLAIN z1 split ones_own_rowsum aux_A <- general_64x16_deep_ring_aux_RC_RC_PLAIN_z1_split_ones_own_rowsum_aux_A
  general gemm_kernel 64x16.deep.ring_aux RC.RC.PLAIN zN split ones_own_rowsum aux_A <- general_64x16_deep_ring_aux_RC_RC_PLAIN_zN_split_ones_own_rowsum_aux_A
  general gemm_kernel 64x16.deep.ring_aux RC.TOKR.TOKJ z1 accumulate aux_B <- general_64x16_deep_ring_aux_RC_TOKR_TOKJ_z1_accumulate_aux_B
  general gemm_kernel 64x16.deep.ring_aux RC.TOKR.TOKJ z1 aux_B <- general_64x16_deep_ring_aux_RC_TOKR_TOKJ_z1_aux_B
  general gemm_kernel 64x16.deep.ring_aux TOKK.TOKK.PLAIN z1 split aux_A <- general_64x16_deep_ring_aux_TOKK_TOKK_PLAIN_z1_split_aux_A
  general gemm_kernel 64x16.deep.ring_aux TOKK.TOKK.PLAIN z1 split ones_own_rowsum aux_A <- general_64x16_deep_ring_aux_TOKK_TOKK_PLAIN_z1_split_ones_own_rowsum_aux_A
  general gemm_kernel 64x16.deep.ring_aux TOKK.TOKK.PLAIN zN split ones_own_rowsum aux_A <- general_64x16_deep_ring_aux_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum_aux_A
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 <- general_64x16_shallow_ring_KC_KC_PLAIN_k1
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 bias_cols <- wl_cases.dense_3x13_k16
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 bias_cols accumulate <- general_64x16_shallow_ring_KC_KC_PLAIN_k1_bias_cols_accumulate
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 bias_cols mask_cols accumulate <- general_64x16_shallow_ring_KC_KC_PLAIN_k1_bias_cols_mask_cols_accumulate
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 bias_cols pre_add <- general_64x16_shallow_ring_KC_KC_PLAIN_k1_bias_cols_pre_add
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 relu bias_cols <- general_64x16_shallow_ring_KC_KC_PLAIN_k1_relu_bias_cols
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering <- general_64x16_shallow_ring_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_covering
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap <- general_64x16_shallow_ring_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_gap
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN k1 silu bias_cols mask_cols save_z <- general_64x16_shallow_ring_KC_KC_PLAIN_k1_silu_bias_cols_mask_cols_save_z
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN kN <- general_64x16_shallow_ring_KC_KC_PLAIN_kN
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN kN bias_cols <- general_64x16_shallow_ring_KC_KC_PLAIN_kN_bias_cols
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN kN bias_cols mask_cols <- general_64x16_shallow_ring_KC_KC_PLAIN_kN_bias_cols_mask_cols
  general gemm_kernel 64x16.shallow.ring KC.KC.PLAIN kN bias_cols mask_cols accumulate <- general_64x16_shallow_ring_KC_KC_PLAIN_kN_bias_cols_mask_cols_accumulate
  general gemm_kernel 64x16.shallow.ring KC.RC.PLAIN z1 <- general_64x16_shallow_ring_KC_RC_PLAIN_z1
  general gemm_kernel 64x16.shallow.ring KC.RC.PLAIN z1 accumulate <- general_64x16_shallow_ring_KC_RC_PLAIN_z1_accumulate
  general gemm_kernel 64x16.shallow.ring KC.RC.PLAIN zN acc_mixed <- general_64x16_shallow_ring_KC_RC_PLAIN_zN_acc_mixed
  general gemm_kernel 64x16.shallow.ring KC.RC.PLAIN zN accumulate <- general_64x16_shallow_ring_KC_RC_PLAIN_zN_accumulate
  general gemm_kernel 64x16.shallow.ring KC.TOKR.TOKJ k1 <- general_64x16_shallow_ring_KC_TOKR_TOKJ_k1
  general gemm_kernel 64x16.shallow.ring KC.TOKR.TOKJ k1 bias_rows <- general_64x16_shallow_ring_KC_TOKR_TOKJ_k1_bias_rows
  general gemm_kernel 64x16.shallow.ring KC.TOKR.TOKJ k1 bias_rows mask_rows <- general_64x16_shallow_ring_KC_TOKR_TOKJ_k1_bias_rows_mask_rows
  general gemm_kernel 64x16.shallow.ring KC.TOKR.TOKJ k1 relu bias_rows <- general_64x16_shallow_ring_KC_TOKR_TOKJ_k1_relu_bias_rows
  general gemm_kernel 64x16.shallow.ring KC.TOKR.TOKJ k1 silu bias_rows mask_rows save_z <- general_64x16_shallow_ring_KC_TOKR_TOKJ_k1_silu_bias_rows_mask_rows_save_z
  general gemm_kernel 64x16.shallow.ring KC.TOKR.TOKJ kN bias_rows <- general_64x16_shallow_ring_KC_TOKR_TOKJ_kN_bias_rows
  general gemm_kernel 64x16.shallow.ring KC.TOKR.TOKJ kN relu bias_rows <- general_64x16_shallow_ring_KC_TOKR_TOKJ_kN_relu_bias_rows
  general gemm_kernel 64x16.shallow.ring RC.TOKR.TOKJ z1 accumulate <- general_64x16_shallow_ring_RC_TOKR_TOKJ_z1_accumulate
  general gemm_kernel 64x16.shallow.ring_aux KC.RC.PLAIN z1 accumulate aux_A <- general_64x16_shallow_ring_aux_KC_RC_PLAIN_z1_accumulate_aux_A
  general gemm_kernel 64x16.shallow.ring_aux RC.TOKR.TOKJ z1 accumulate aux_B <- general_64x16_shallow_ring_aux_RC_TOKR_TOKJ_z1_accumulate_aux_B
  general gemm_kernel big64x64.plain_template RC.TOKR.TOKJ z1 accumulate aux_B <- general_big64x64_plain_template_RC_TOKR_TOKJ_z1_accumulate_aux_B
  general gemm_kernel big64x64.plain_template RC.TOKR.TOKJ z1 aux_B <- general_big64x64_plain_template_RC_TOKR_TOKJ_z1_aux_B
  general gemm_kernel big64x64.plain_template RC.TOKR.TOKJ zN acc_mixed aux_B <- general_big64x64_plain_template_RC_TOKR_TOKJ_zN_acc_mixed_aux_B
  general gemm_kernel big64x64.plain_template RC.TOKR.TOKJ zN accumulate <- general_big64x64_plain_template_RC_TOKR_TOKJ_zN_accumulate
  general gemm_kernel big64x64.plain_template RC.TOKR.TOKJ zN accumulate aux_B <- general_big64x64_plain_template_RC_TOKR_TOKJ_zN_accumulate_aux_B
  general gemm_kernel big64x64.plain_template RC.TOKR.TOKJ zN aux_B <- general_big64x64_plain_template_RC_TOKR_TOKJ_zN_aux_B
  general gemm_kernel mid64x64.deep.plain_template RC.TOKR.TOKJ kN disagree aux_B <- general_mid64x64_deep_plain_template_RC_TOKR_TOKJ_kN_disagree_aux_B
  general gemm_kernel mid64x64.deep.ring KC.KC.PLAIN k1 bias_cols <- general_mid64x64_deep_ring_KC_KC_PLAIN_k1_bias_cols
  general gemm_kernel mid64x64.deep.ring KC.KC.PLAIN k1 relu bias_cols <- general_mid64x64_deep_ring_KC_KC_PLAIN_k1_relu_bias_cols
  general gemm_kernel mid64x64.deep.ring KC.KC.PLAIN k1 split <- general_mid64x64_deep_ring_KC_KC_PLAIN_k1_split
  general gemm_kernel mid64x64.deep.ring KC.KC.PLAIN k1 split bias_cols <- general_mid64x64_deep_ring_KC_KC_PLAIN_k1_split_bias_cols
  general gemm_kernel mid64x64.deep.ring KC.KC.PLAIN kN split <- general_mid64x64_deep_ring_KC_KC_PLAIN_kN_split
  general gemm_kernel mid64x64.deep.ring KC.KC.PLAIN kN split bias_cols <- general_mid64x64_deep_ring_KC_KC_PLAIN_kN_split_bias_cols
  general gemm_kernel mid64x64.deep.ring KC.KC.PLAIN kN split relu bias_cols <- general_mid64x64_deep_ring_KC_KC_PLAIN_kN_split_relu_bias_cols
  general gemm_kernel mid64x64.deep.ring KC.RC.PLAIN z1 <- general_mid64x64_deep_ring_KC_RC_PLAIN_z1
  general gemm_kernel mid64x64.deep.ring KC.RC.PLAIN z1 accumulate <- general_mid64x64_deep_ring_KC_RC_PLAIN_z1_accumulate
  general gemm_kernel mid64x64.deep.ring KC.RC.PLAIN z1 split <- general_mid64x64_deep_ring_KC_RC_PLAIN_z1_split
  general gemm_kernel mid64x64.deep.ring KC.RC.PLAIN z1 split accumulate <- general_mid64x64_deep_ring_KC_RC_PLAIN_z1_split_accumulate
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN bias_rows mask_rows <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN_bias_rows_mask_rows
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN silu bias_rows mask_rows save_z <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN_silu_bias_rows_mask_rows_save_z
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN split <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN_split
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN split bias_rows <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN_split_bias_rows
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN split bias_rows mask_rows <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN_split_bias_rows_mask_rows
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN split relu bias_rows <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN_split_relu_bias_rows
  general gemm_kernel mid64x64.deep.ring KC.TOKR.TOKJ kN split silu bias_rows mask_rows save_z <- general_mid64x64_deep_ring_KC_TOKR_TOKJ_kN_split_silu_bias_rows_mask_rows_save_z
  general gemm_kernel mid64x64.deep.ring RC.RC.PLAIN z1 ones_own_rowsum <- general_mid64x64_deep_ring_RC_RC_PLAIN_z1_ones_own_rowsum
  general gemm_kernel mid64x64.deep.ring RC.RC.PLAIN z1 split <- general_mid64x64_deep_ring_RC_RC_PLAIN_z1_split
  general gemm_kernel mid64x64.deep.ring RC.RC.PLAIN z1 split accumulate <- general_mid64x64_deep_ring_RC_RC_PLAIN_z1_split_accumulate
  general gemm_kernel mid64x64.deep.ring RC.RC.PLAIN z1 split accumulate mvalid<M <- general_mid64x64_deep_ring_RC_RC_PLAIN_z1_split_accumulate_mvalid_lt_M
  general gemm_kernel mid64x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum <- general_mid64x64_deep_ring_RC_RC_PLAIN_z1_split_ones_own_rowsum
  general gemm_kernel mid64x64.deep.ring RC.RC.PLAIN z1 split ones_own_rowsum mvalid<M <- general_mid64x64_deep_ring_RC_RC_PLAIN_z1_split_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel mid64x64.deep.ring RC.TOKR.TOKJ kN split <- general_mid64x64_deep_ring_RC_TOKR_TOKJ_kN_split
  general gemm_kernel mid64x64.deep.ring RC.TOKR.TOKJ kN split accumulate <- general_mid64x64_deep_ring_RC_TOKR_TOKJ_kN_split_accumulate
  general gemm_kernel mid64x64.deep.ring RC.TOKR.TOKJ z1 <- general_mid64x64_deep_ring_RC_TOKR_TOKJ_z1
  general gemm_kernel mid64x64.deep.ring RC.TOKR.TOKJ z1 accumulate <- general_mid64x64_deep_ring_RC_TOKR_TOKJ_z1_accumulate
  general gemm_kernel mid64x64.deep.ring_aux KC.RC.PLAIN z1 accumulate aux_A <- general_mid64x64_deep_ring_aux_KC_RC_PLAIN_z1_accumulate_aux_A
  general gemm_kernel mid64x64.deep.ring_aux KC.RC.PLAIN z1 aux_A <- general_mid64x64_deep_ring_aux_KC_RC_PLAIN_z1_aux_A
  general gemm_kernel mid64x64.deep.ring_aux KC.RC.PLAIN z1 split accumulate aux_A <- general_mid64x64_deep_ring_aux_KC_RC_PLAIN_z1_split_accumulate_aux_A
  general gemm_kernel mid64x64.deep.ring_aux RC.TOKR.TOKJ k1 accumulate aux_B <- general_mid64x64_deep_ring_aux_RC_TOKR_TOKJ_k1_accumulate_aux_B
  general gemm_kernel mid64x64.deep.ring_aux RC.TOKR.TOKJ z1 accumulate aux_B <- general_mid64x64_deep_ring_aux_RC_TOKR_TOKJ_z1_accumulate_aux_B
  general gemm_kernel mid64x64.deep.ring_aux RC.TOKR.TOKJ z1 aux_B <- general_mid64x64_deep_ring_aux_RC_TOKR_TOKJ_z1_aux_B
  general gemm_kernel mid64x64.shallow.ring KC.KC.PLAIN k1 bias_cols <- general_mid64x64_shallow_ring_KC_KC_PLAIN_k1_bias_cols
  general gemm_kernel mid64x64.shallow.ring KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap <- general_mid64x64_shallow_ring_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_gap
  general gemm_kernel mid64x64.shallow.ring KC.KC.PLAIN kN bias_cols <- general_mid64x64_shallow_ring_KC_KC_PLAIN_kN_bias_cols
  general gemm_kernel mid64x64.shallow.ring KC.RC.PLAIN z1 <- general_mid64x64_shallow_ring_KC_RC_PLAIN_z1
  general gemm_kernel mid64x64.shallow.ring KC.RC.PLAIN z1 accumulate <- general_mid64x64_shallow_ring_KC_RC_PLAIN_z1_accumulate
  general gemm_kernel mid64x64.shallow.ring KC.RC.PLAIN zN <- general_mid64x64_shallow_ring_KC_RC_PLAIN_zN
  general gemm_kernel mid64x64.shallow.ring KC.RC.PLAIN zN acc_mixed <- general_mid64x64_shallow_ring_KC_RC_PLAIN_zN_acc_mixed
  general gemm_kernel mid64x64.shallow.ring KC.RC.PLAIN zN accumulate <- general_mid64x64_shallow_ring_KC_RC_PLAIN_zN_accumulate
  general gemm_kernel mid64x64.shallow.ring RC.TOKR.TOKJ z1 <- general_mid64x64_shallow_ring_RC_TOKR_TOKJ_z1
  general gemm_kernel mid64x64.shallow.ring RC.TOKR.TOKJ z1 accumulate <- general_mid64x64_shallow_ring_RC_TOKR_TOKJ_z1_accumulate
  general gemm_kernel mid64x64.shallow.ring RC.TOKR.TOKJ zN <- general_mid64x64_shallow_ring_RC_TOKR_TOKJ_zN
  general gemm_kernel mid64x64.shallow.ring RC.TOKR.TOKJ zN acc_mixed <- general_mid64x64_shallow_ring_RC_TOKR_TOKJ_zN_acc_mixed
  general gemm_kernel mid64x64.shallow.ring RC.TOKR.TOKJ zN accumulate <- general_mid64x64_shallow_ring_RC_TOKR_TOKJ_zN_accumulate
  general gemm_kernel mid64x64.shallow.ring_aux KC.RC.PLAIN z1 accumulate aux_A <- general_mid64x64_shallow_ring_aux_KC_RC_PLAIN_z1_accumulate_aux_A
  general gemm_kernel mid64x64.shallow.ring_aux RC.TOKR.TOKJ z1 aux_B <- general_mid64x64_shallow_ring_aux_RC_TOKR_TOKJ_z1_aux_B
  general gemm_kernel mid64x64.shallow.ring_aux RC.TOKR.TOKJ zN acc_mixed aux_B <- general_mid64x64_shallow_ring_aux_RC_TOKR_TOKJ_zN_acc_mixed_aux_B
  general gemm_kernel mid64x64.shallow.ring_aux RC.TOKR.TOKJ zN accumulate aux_B <- general_mid64x64_shallow_ring_aux_RC_TOKR_TOKJ_zN_accumulate_aux_B
  general gemm_kernel mid64x64.shallow.ring_aux RC.TOKR.TOKJ zN aux_B <- general_mid64x64_shallow_ring_aux_RC_TOKR_TOKJ_zN_aux_B
  general gemm_kernel z32x32.deep.ring KC.RC.PLAIN zN accumulate <- general_z32x32_deep_ring_KC_RC_PLAIN_zN_accumulate
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN <- general_z32x32_deep_ring_RC_RC_PLAIN_zN
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN ones_own_rowsum <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_ones_own_rowsum
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN ones_own_rowsum mvalid<M <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN split <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_split
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN split accumulate <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_split_accumulate
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN split ones_own_rowsum <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_split_ones_own_rowsum
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN split ones_own_rowsum mvalid<M <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_split_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN split_deferred <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_split_deferred
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN split_deferred ones_own_rowsum <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_split_deferred_ones_own_rowsum
  general gemm_kernel z32x32.deep.ring RC.RC.PLAIN zN split_deferred ones_own_rowsum mvalid<M <- general_z32x32_deep_ring_RC_RC_PLAIN_zN_split_deferred_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel z32x32.deep.ring RC.TOKR.TOKJ zN <- general_z32x32_deep_ring_RC_TOKR_TOKJ_zN
  general gemm_kernel z32x32.deep.ring RC.TOKR.TOKJ zN acc_mixed <- general_z32x32_deep_ring_RC_TOKR_TOKJ_zN_acc_mixed
  general gemm_kernel z32x32.deep.ring RC.TOKR.TOKJ zN accumulate <- general_z32x32_deep_ring_RC_TOKR_TOKJ_zN_accumulate
  general gemm_kernel z32x32.deep.ring TOKK.TOKK.PLAIN zN split ones_own_rowsum <- general_z32x32_deep_ring_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  general gemm_kernel z32x32.deep.ring TOKK.TOKK.PLAIN zN split_deferred <- general_z32x32_deep_ring_TOKK_TOKK_PLAIN_zN_split_deferred
  general gemm_kernel z32x32.deep.ring TOKK.TOKK.PLAIN zN split_deferred ones_own_rowsum <- general_z32x32_deep_ring_TOKK_TOKK_PLAIN_zN_split_deferred_ones_own_rowsum
  general gemm_kernel z32x32.deep.ring TOKK.TOKK.PLAIN zN split_deferred ones_own_rowsum mvalid<M <- general_z32x32_deep_ring_TOKK_TOKK_PLAIN_zN_split_deferred_ones_own_rowsum_mvalid_lt_M
  general gemm_kernel z32x32.deep.ring_aux KC.RC.PLAIN zN acc_mixed aux_A <- general_z32x32_deep_ring_aux_KC_RC_PLAIN_zN_acc_mixed_aux_A
  general gemm_kernel z32x32.deep.ring_aux KC.RC.PLAIN zN accumulate aux_A <- general_z32x32_deep_ring_aux_KC_RC_PLAIN_zN_accumulate_aux_A
  general gemm_kernel z32x32.deep.ring_aux KC.RC.PLAIN zN aux_A <- general_z32x32_deep_ring_aux_KC_RC_PLAIN_zN_aux_A
  general gemm_kernel z32x32.deep.ring_aux KC.RC.PLAIN zN split acc_mixed aux_A <- general_z32x32_deep_ring_aux_KC_RC_PLAIN_zN_split_acc_mixed_aux_A
  general gemm_kernel z32x32.deep.ring_aux KC.RC.PLAIN zN split accumulate aux_A <- general_z32x32_deep_ring_aux_KC_RC_PLAIN_zN_split_accumulate_aux_A
  general gemm_kernel z32x32.deep.ring_aux RC.RC.PLAIN zN aux_A <- general_z32x32_deep_ring_aux_RC_RC_PLAIN_zN_aux_A
  general gemm_kernel z32x32.deep.ring_aux RC.RC.PLAIN zN ones_own_rowsum aux_A <- general_z32x32_deep_ring_aux_RC_RC_PLAIN_zN_ones_own_rowsum_aux_A
  general gemm_kernel z32x32.deep.ring_aux RC.RC.PLAIN zN split ones_own_rowsum aux_A <- general_z32x32_deep_ring_aux_RC_RC_PLAIN_zN_split_ones_own_rowsum_aux_A
  general gemm_kernel z32x32.deep.ring_aux RC.TOKR.TOKJ zN acc_mixed aux_B <- general_z32x32_deep_ring_aux_RC_TOKR_TOKJ_zN_acc_mixed_aux_B
  general gemm_kernel z32x32.deep.ring_aux RC.TOKR.TOKJ zN accumulate aux_B <- general_z32x32_deep_ring_aux_RC_TOKR_TOKJ_zN_accumulate_aux_B
  general gemm_kernel z32x32.deep.ring_aux RC.TOKR.TOKJ zN aux_B <- general_z32x32_deep_ring_aux_RC_TOKR_TOKJ_zN_aux_B
  general gemm_kernel z32x32.deep.ring_aux TOKK.TOKK.PLAIN zN split aux_A <- general_z32x32_deep_ring_aux_TOKK_TOKK_PLAIN_zN_split_aux_A
  general gemm_kernel z32x32.deep.ring_aux TOKK.TOKK.PLAIN zN split ones_own_rowsum aux_A <- general_z32x32_deep_ring_aux_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum_aux_A
  kslice gemm_kslice_kernel - KC.KC.PLAIN k1 <- kslice_-_KC_KC_PLAIN_k1
  kslice gemm_kslice_kernel - KC.KC.PLAIN k1 bias_cols <- kslice_-_KC_KC_PLAIN_k1_bias_cols
  kslice gemm_kslice_kernel - KC.KC.PLAIN k1 bias_cols mask_cols <- kslice_-_KC_KC_PLAIN_k1_bias_cols_mask_cols
  kslice gemm_kslice_kernel - KC.KC.PLAIN k1 bias_cols mask_cols accumulate <- kslice_-_KC_KC_PLAIN_k1_bias_cols_mask_cols_accumulate
  kslice gemm_kslice_kernel - KC.KC.PLAIN k1 silu bias_cols mask_cols save_z <- kslice_-_KC_KC_PLAIN_k1_silu_bias_cols_mask_cols_save_z
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN <- kslice_-_KC_KC_PLAIN_kN
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN accumulate <- kslice_-_KC_KC_PLAIN_kN_accumulate
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN bias_cols mask_cols <- kslice_-_KC_KC_PLAIN_kN_bias_cols_mask_cols
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN bias_cols mask_cols accumulate <- kslice_-_KC_KC_PLAIN_kN_bias_cols_mask_cols_accumulate
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN mask_cols accumulate <- kslice_-_KC_KC_PLAIN_kN_mask_cols_accumulate
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN relu bias_cols <- kslice_-_KC_KC_PLAIN_kN_relu_bias_cols
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN sigmoid bias_cols save_act gate_covering <- kslice_-_KC_KC_PLAIN_kN_sigmoid_bias_cols_save_act_gate_covering
  kslice gemm_kslice_kernel - KC.KC.PLAIN kN silu bias_cols mask_cols save_z <- kslice_-_KC_KC_PLAIN_kN_silu_bias_cols_mask_cols_save_z
  skinny_n gemm_skinny_n_kernel 8waves KC.KC.PLAIN k1 <- skinny_n_8waves_KC_KC_PLAIN_k1
  skinny_n gemm_skinny_n_kernel 8waves KC.KC.PLAIN k1 bias_cols <- skinny_n_8waves_KC_KC_PLAIN_k1_bias_cols
  skinny_n gemm_skinny_n_kernel 8waves KC.KC.PLAIN k1 relu bias_cols <- skinny_n_8waves_KC_KC_PLAIN_k1_relu_bias_cols
  skinny_n gemm_skinny_n_kernel 8waves KC.KC.PLAIN kN <- skinny_n_8waves_KC_KC_PLAIN_kN
  skinny_n gemm_skinny_n_kernel 8waves KC.KC.PLAIN kN bias_cols <- skinny_n_8waves_KC_KC_PLAIN_kN_bias_cols
  skinny_n gemm_skinny_n_kernel 8waves KC.KC.PLAIN kN relu bias_cols <- skinny_n_8waves_KC_KC_PLAIN_kN_relu_bias_cols
  skinny_n gemm_skinny_n_kernel 8waves KC.RC.PLAIN z1 <- skinny_n_8waves_KC_RC_PLAIN_z1
  tinyk gemm_tinyk_kernel col4 KC.KC.PLAIN k1 bias_cols accumulate <- tinyk_col4_KC_KC_PLAIN_k1_bias_cols_accumulate
  tinyk gemm_tinyk_kernel col4 KC.KC.PLAIN k1 bias_cols mask_cols accumulate <- tinyk_col4_KC_KC_PLAIN_k1_bias_cols_mask_cols_accumulate
  tinyk gemm_tinyk_kernel col4 KC.KC.PLAIN k1 bias_cols pre_add <- tinyk_col4_KC_KC_PLAIN_k1_bias_cols_pre_add
  tinyk gemm_tinyk_kernel col4 KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_covering <- tinyk_col4_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_covering
  tinyk gemm_tinyk_kernel col4 KC.KC.PLAIN k1 sigmoid bias_cols save_act gate_gap <- tinyk_col4_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_gap
  tinyk gemm_tinyk_kernel col4 KC.KC.PLAIN k1 silu bias_cols mask_cols save_z <- tinyk_col4_KC_KC_PLAIN_k1_silu_bias_cols_mask_cols_save_z
  tinyk gemm_tinyk_kernel simple KC.KC.PLAIN k1 <- tinyk_simple_KC_KC_PLAIN_k1
  tinyk gemm_tinyk_kernel simple KC.KC.PLAIN k1 bias_cols <- tinyk_simple_KC_KC_PLAIN_k1_bias_cols
  tinyk gemm_tinyk_kernel simple KC.KC.PLAIN k1 relu bias_cols <- tinyk_simple_KC_KC_PLAIN_k1_relu_bias_cols
  token_dw token_dw_kernel rb1.cb4 TOKK.TOKK.PLAIN zN split ones_own_rowsum <- token_dw_rb1_cb4_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  token_dw token_dw_kernel rb1.cb5 TOKK.TOKK.PLAIN z1 split ones_own_rowsum <- token_dw_rb1_cb5_TOKK_TOKK_PLAIN_z1_split_ones_own_rowsum
  token_dw token_dw_kernel rb3.cb2 TOKK.TOKK.PLAIN z1 split <- token_dw_rb3_cb2_TOKK_TOKK_PLAIN_z1_split
  token_dw token_dw_kernel rb3.cb2 TOKK.TOKK.PLAIN z1 split ones_own_rowsum <- token_dw_rb3_cb2_TOKK_TOKK_PLAIN_z1_split_ones_own_rowsum
  token_dw token_dw_kernel rb3.cb2 TOKK.TOKK.PLAIN zN split <- token_dw_rb3_cb2_TOKK_TOKK_PLAIN_zN_split
  token_dw token_dw_kernel rb3.cb2 TOKK.TOKK.PLAIN zN split ones_own_rowsum <- token_dw_rb3_cb2_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  token_dw token_dw_kernel rb3.cb4 TOKK.TOKK.PLAIN zN split ones_own_rowsum <- token_dw_rb3_cb4_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  token_dw token_dw_kernel rb3.cb5 TOKK.TOKK.PLAIN z1 split <- token_dw_rb3_cb5_TOKK_TOKK_PLAIN_z1_split
  token_dw token_dw_kernel rb3.cb5 TOKK.TOKK.PLAIN zN split <- token_dw_rb3_cb5_TOKK_TOKK_PLAIN_zN_split
  token_dw token_dw_kernel rb3.cb5 TOKK.TOKK.PLAIN zN split ones_own_rowsum <- token_dw_rb3_cb5_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  token_dw token_dw_kernel rb4.cb2 TOKK.TOKK.PLAIN z1 split <- token_dw_rb4_cb2_TOKK_TOKK_PLAIN_z1_split
  token_dw token_dw_kernel rb4.cb2 TOKK.TOKK.PLAIN zN split <- token_dw_rb4_cb2_TOKK_TOKK_PLAIN_zN_split
  token_dw token_dw_kernel rb4.cb2 TOKK.TOKK.PLAIN zN split ones_own_rowsum <- token_dw_rb4_cb2_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum
  token_dw token_dw_kernel rb4.cb2 TOKK.TOKK.PLAIN zN split ones_own_rowsum mvalid<M <- token_dw_rb4_cb2_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum_mvalid_lt_M
  token_dw token_dw_kernel rb4.cb4 TOKK.TOKK.PLAIN z1 split ones_own_rowsum <- token_dw_rb4_cb4_TOKK_TOKK_PLAIN_z1_split_ones_own_rowsum
  token_dw token_dw_kernel rb4.cb5 TOKK.TOKK.PLAIN z1 split <- token_dw_rb4_cb5_TOKK_TOKK_PLAIN_z1_split
  token_dw token_dw_kernel rb4.cb5 TOKK.TOKK.PLAIN zN split <- token_dw_rb4_cb5_TOKK_TOKK_PLAIN_zN_split
  token_dw token_dw_kernel rb4.cb5 TOKK.TOKK.PLAIN zN split mvalid<M <- token_dw_rb4_cb5_TOKK_TOKK_PLAIN_zN_split_mvalid_lt_M
  token_dw token_dw_kernel rb4.cb5 TOKK.TOKK.PLAIN zN split ones_own_rowsum mvalid<M <- token_dw_rb4_cb5_TOKK_TOKK_PLAIN_zN_split_ones_own_rowsum_mvalid_lt_M
  token_linear token_linear_kernel rb1.one_problem KC.TOKR.TOKJ k1 bias_rows <- token_linear_rb1_one_problem_KC_TOKR_TOKJ_k1_bias_rows
  token_linear token_linear_kernel rb1.one_problem KC.TOKR.TOKJ k1 relu bias_rows <- token_linear_rb1_one_problem_KC_TOKR_TOKJ_k1_relu_bias_rows
  token_linear token_linear_kernel rb1.one_problem KC.TOKR.TOKJ kN bias_rows <- token_linear_rb1_one_problem_KC_TOKR_TOKJ_kN_bias_rows
  token_linear token_linear_kernel rb1.one_problem KC.TOKR.TOKJ kN relu bias_rows <- token_linear_rb1_one_problem_KC_TOKR_TOKJ_kN_relu_bias_rows
  token_linear token_linear_kernel rb1.one_problem RC.TOKR.TOKJ z1 accumulate <- token_linear_rb1_one_problem_RC_TOKR_TOKJ_z1_accumulate
  token_linear token_linear_kernel rb2.one_problem KC.TOKR.TOKJ k1 bias_rows <- token_linear_rb2_one_problem_KC_TOKR_TOKJ_k1_bias_rows
  token_linear token_linear_kernel rb2.one_problem KC.TOKR.TOKJ kN relu bias_rows <- token_linear_rb2_one_problem_KC_TOKR_TOKJ_kN_relu_bias_rows
  token_linear token_linear_kernel rb2.one_problem RC.TOKR.TOKJ k1 accumulate <- token_linear_rb2_one_problem_RC_TOKR_TOKJ_k1_accumulate
  token_linear token_linear_kernel rb2.one_problem RC.TOKR.TOKJ kN <- token_linear_rb2_one_problem_RC_TOKR_TOKJ_kN
  token_linear token_linear_kernel rb2.one_problem RC.TOKR.TOKJ kN accumulate <- token_linear_rb2_one_problem_RC_TOKR_TOKJ_kN_accumulate
  token_linear token_linear_kernel rb2.one_problem RC.TOKR.TOKJ z1 <- token_linear_rb2_one_problem_RC_TOKR_TOKJ_z1
  token_linear token_linear_kernel rb3.one_problem KC.TOKR.TOKJ k1 <- token_linear_rb3_one_problem_KC_TOKR_TOKJ_k1
  token_linear token_linear_kernel rb3.one_problem KC.TOKR.TOKJ k1 bias_rows <- token_linear_rb3_one_problem_KC_TOKR_TOKJ_k1_bias_rows
  token_linear token_linear_kernel rb3.one_problem KC.TOKR.TOKJ k1 relu bias_rows <- token_linear_rb3_one_problem_KC_TOKR_TOKJ_k1_relu_bias_rows
  token_linear token_linear_kernel rb3.one_problem KC.TOKR.TOKJ kN <- token_linear_rb3_one_problem_KC_TOKR_TOKJ_kN
  token_linear token_linear_kernel rb3.one_problem KC.TOKR.TOKJ kN bias_rows <- token_linear_rb3_one_problem_KC_TOKR_TOKJ_kN_bias_rows
  token_linear token_linear_kernel rb3.one_problem KC.TOKR.TOKJ kN relu bias_rows <- token_linear_rb3_one_problem_KC_TOKR_TOKJ_kN_relu_bias_rows
  token_linear token_linear_kernel rb4.batch RC.TOKR.TOKJ zN acc_mixed <- token_linear_rb4_batch_RC_TOKR_TOKJ_zN_acc_mixed
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ k1 <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_k1
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ k1 bias_rows <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_k1_bias_rows
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ k1 bias_rows mask_rows <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_k1_bias_rows_mask_rows
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ k1 relu bias_rows <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_k1_relu_bias_rows
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ k1 silu bias_rows mask_rows save_z <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_k1_silu_bias_rows_mask_rows_save_z
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ kN <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_kN
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ kN bias_rows mask_rows <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_kN_bias_rows_mask_rows
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ kN relu bias_rows <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_kN_relu_bias_rows
  token_linear token_linear_kernel rb4.one_problem KC.TOKR.TOKJ kN silu bias_rows mask_rows save_z <- token_linear_rb4_one_problem_KC_TOKR_TOKJ_kN_silu_bias_rows_mask_rows_save_z
  token_linear token_linear_kernel rb4.one_problem RC.TOKR.TOKJ z1 <- token_linear_rb4_one_problem_RC_TOKR_TOKJ_z1
  token_linear token_linear_kernel rb4.one_problem RC.TOKR.TOKJ z1 accumulate <- token_linear_rb4_one_problem_RC_TOKR_TOKJ_z1_accumulate
  token_linear token_linear_kernel rb5.batch RC.TOKR.TOKJ zN <- token_linear_rb5_batch_RC_TOKR_TOKJ_zN
  token_linear token_linear_kernel rb5.batch RC.TOKR.TOKJ zN acc_mixed <- token_linear_rb5_batch_RC_TOKR_TOKJ_zN_acc_mixed
  token_linear token_linear_kernel rb5.batch RC.TOKR.TOKJ zN accumulate <- token_linear_rb5_batch_RC_TOKR_TOKJ_zN_accumulate
  token_linear token_linear_kernel rb5.one_problem RC.TOKR.TOKJ z1 <- token_linear_rb5_one_problem_RC_TOKR_TOKJ_z1
  token_linear token_linear_kernel rb5.one_problem RC.TOKR.TOKJ z1 accumulate <- token_linear_rb5_one_problem_RC_TOKR_TOKJ_z1_accumulate
"""
import contextlib
import io

import pytest
import torch

import gemm_cases as G
import op_forms as F
import wl_cases as W
from nasrec_amd import _lib as L

DEFAULTS = set(G.DEFAULTS) | {"highest"}
KERNEL = {"general": "gemm_kernel", "kslice": "gemm_kslice_kernel", "skinny_n": "gemm_skinny_n_kernel", "tinyk": "gemm_tinyk_kernel",
          "token_linear": "token_linear_kernel", "token_dw": "token_dw_kernel", "fast": "gemm_fast_kernel"}


@pytest.fixture(scope="module")
def harvested():
    forms, _ = F.harvest()
    return {f: d for f, d in forms.items() if f[0] == "gemm"}


def case_forms():
    """form -> name of the first case that sets it (built on the host: no pointer is dereferenced)"""
    out = {}
    for c in G.CASES:
        out.setdefault(c.form(), c.name)
    for c in W.CASES:
        if c.gemm:
            d = c.build("cpu").desc
            out.setdefault(F.form_of(d), "wl_cases." + c.name)
    return out


@pytest.fixture(scope="module")
def covered():
    return case_forms()


def show(form):
    return " ".join(w for w in form[1:] if w not in DEFAULTS)


def test_every_harvested_gemm_form_is_the_form_of_a_case(harvested, covered):
    uncovered = sorted(show(f) for f in harvested if f not in covered)
    assert not uncovered, "GEMM forms the planner emits and no kernel case sets:\n  " + "\n  ".join(uncovered)


def test_the_harvest_contains_the_forms_the_planner_is_known_to_emit(harvested):
    """... so that an empty or a crippled harvest does not pass for full coverage"""
    fs = list(harvested)
    assert len(fs) >= 300
    assert {f[1] for f in fs} == set(F.GEMM_FAMILY.values())
    configs = {f[3] for f in fs if f[1] == "general"}
    for cfg in ("16x64.deep.ring", "16x64.deep.ring_aux", "16x64.shallow.ring", "64x16.deep.ring", "64x16.deep.ring_aux", "64x16.shallow.ring",
                "64x16.shallow.ring_aux", "big64x64.plain_template", "mid64x64.deep.ring", "mid64x64.deep.ring_aux", "mid64x64.shallow.ring",
                "mid64x64.shallow.ring_aux", "mid64x64.deep.plain_template", "z32x32.deep.ring", "z32x32.deep.ring_aux"):
        assert cfg in configs, cfg
    for cfg in configs:
        tile, body = cfg.rsplit(".", 1)
        assert tile in F.GENERAL_CONFIGS and body in F.GENERAL_BODIES, cfg

    def some(*props):
        return any(all(p in f for p in props) for f in fs)
    assert some("fast", "split") and some("fast", "s1") and not some("balanced")
    assert some("token_dw", "ones_own_rowsum") and some("token_linear", "bias_rows", "mask_rows", "save_z")
    assert some("disagree", "aux_B") and some("split_deferred") and some("pre_add") and some("gate_gap") and some("gate_covering")
    assert some("silu", "save_z") and some("sigmoid", "save_act") and some("acc_mixed") and some("mvalid<M")
    assert not some("null_A") and not some("gate_gap_null") and not some("gate_covering_null")
    assert {f[-1] for f in fs} == {"highest"}  # (the bf16 bodies: tests/test_gemm_bf16_gpu.py, tests/test_token_linear_bf16_gpu.py)


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_a_case_has_the_form_its_words_claim(case):
    """family, configuration, binding, segments and every non-default property: exactly the words of the case (a word that starts with @
    is an option of the case, no property of the form)"""
    f = case.form()
    claimed = [w for w in case.words.split() if not w.startswith("@")]
    assert f[0] == "gemm" and f[1] == case.family and f[2] == KERNEL[case.family]
    assert [f[1], f[3], f[4], f[5]] == claimed[:4]
    assert sorted(w for w in f[6:] if w not in DEFAULTS) == sorted(claimed[4:])


def test_the_cases_the_issue_of_this_table_asked_for_have_their_forms(covered):
    """forms no plan emits today and a kernel has code for: the balanced schedule with a non-trivial epilogue; a NULL A segment in every
    family that takes several k-segments; the acc_in_tile start of the throughput kernel and its neighbour with a bias; a NULL gating
    pointer; the 4-wave skinny_n instantiation; ft_epilogue's full path.  (NASREC_SPLITK_BALANCED on a plain product stays with
    tests/test_gemm_fast_gpu.py; a precision other than HIGHEST with the bf16 test files.)"""
    fs = list(covered)

    def some(*props):
        return any(all(p in f for p in props) for f in fs)
    assert some("fast", "balanced", "sigmoid", "gate_gap", "save_act") and some("fast", "balanced", "pre_add", "save_z", "accumulate", "mask_cols")
    for family in ("general", "kslice", "skinny_n", "token_linear", "fast"):
        assert some(family, "kN", "null_A"), family
    assert some("general", "split", "null_A")
    assert some("fast", "no_ones_template.acc_in_tile", "k1", "accumulate", "no_bias")
    assert some("fast", "no_ones_template.nread1", "k1", "accumulate", "bias_cols", "act_none")
    assert some("fast", "gate_gap_null") and some("general", "gate_covering_null")
    assert some("skinny_n", "4waves") and some("fast", "no_ones_template.full_nread2+", "s1")
    assert some("general", "big64x64.plain_template", "KC.KC.PLAIN")


CHECKED = ["general_64x16_deep_ring_KC_KC_PLAIN_kN_relu_bias_cols_null_A", "fast_no_ones_template_nread1_KC_KC_PLAIN_k1_sigmoid_bias_cols_save_act_gate_gap_null",
           "general_64x16_deep_ring_KC_TOKR_TOKJ_kN_relu_bias_rows_mask_rows_dims0", "skinny_n_8waves_KC_KC_PLAIN_kN_bias_cols_null_A"]


@pytest.mark.parametrize("name", CHECKED)
def test_a_cases_check_accepts_its_reference_and_notices_one_wrong_element(name):
    """the checker itself, on the host: the fp64 reference rounded to fp32 and laid out in the output buffers passes; the same with one
    element of C off by 1e-2 of the scale, with a pad column written, or with save_act holding the gated value, fails"""
    b = G.BY_NAME[name].build("cpu")
    ref = b.reference(torch.float64)
    got = {}
    for k, v in b.outs.items():
        g = v.clone()
        if k.startswith("rowsum"):
            g[:ref[k].numel()] = ref[k].float()
        elif k != "workspace":
            g = torch.where(b.planes[k].inside, b.planes[k].image(ref[k].float(), 0.0), g)
        got[k] = g

    def passes(g):
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                b.check(g)
                return True
            except AssertionError:
                return False
    assert passes(got)
    plane = b.planes["C0"]
    last, pad = int(plane.inside.nonzero()[-1]), int((~plane.inside).nonzero()[0])
    wrong = got["C0"].clone()
    wrong[last] += 1e-2 * max(1.0, float(ref["C0"].abs().max()))
    assert not passes(dict(got, C0=wrong))
    wrong = got["C0"].clone()
    wrong[pad] = 0.0
    assert not passes(dict(got, C0=wrong))
    if "save_act" in got:
        assert not passes(dict(got, save_act=torch.where(plane.inside, plane.image(ref["C0"].float(), 0.0), got["save_act"])))


def coverage_table(forms, covered):
    return ["  %s <- %s" % (show(f), covered[f]) for f in sorted(forms, key=show)]


def test_the_table_in_this_modules_docstring_is_the_harvest(harvested, covered):
    rows = [line.rstrip() for line in __doc__.splitlines() if " <- " in line]
    assert rows == [r.rstrip() for r in coverage_table(harvested, covered)]
    assert ("The harvest holds %d GEMM forms." % len(harvested)) in __doc__
    assert ("%d forms in the harvest" % len(harvested)) in F.__doc__
