"""Every GEMM kernel at every descriptor form the plan compiler emits, against plain fp64 math of the same descriptor.

The cases are the table of tests/gemm_cases.py (tests/test_gemm_forms_cpu.py holds it against the harvest of tests/op_forms.py and
carries the form -> case table): one case per form — kernel family, tile configuration or launcher branch, operand binding, k-segments or
z-problems, split-K class, and every predicate the five copies of the epilogue are written in — at the smallest shapes the routing rule
accepts for the form, ragged against every tile, with NaN in the pad columns of the inputs and a sentinel in the pad columns and behind
the tail of every output (C, save_z, save_act, the row sums, the split-K workspace).  Each case asserts, before it launches, that
nasrec_gemm_route still names the family it was written for, goes through nasrec_launch (a deferred second pass is finished by one
NASREC_OP_SPLITK_EPILOGUES launch in the same case), synchronises once and runs its check.  save_z and save_act are outputs in their
own right; a masked element must be exactly 0 (exactly the accumulation target's value where the launch accumulates); a problem that
does not accumulate starts as NaN, so a kernel that read it fails; the ones-column's sums go to the row-sum buffer and column N - 1 of
C, its first pad column, keeps the sentinel.

Tolerances, compared as wl_cases.close compares (max error against tol x max(1, |ref|max)): 2e-5 for forward and input-gradient
products (tests/test_ops_gpu.py, tests/test_gemm_fast_gpu.py), 5e-5 for the weight-gradient products with K = 16 B at large batch
(token_dw and the throughput kernel's weight-gradient binding: the figure tests/test_gemm_fast_gpu.py uses).  A case with SiLU or a
sigmoid in its epilogue has no established figure: its bound is ACT_FLOOR_MULTIPLE = 8 x the floor, the maximum absolute error of
torch's fp32 evaluation of the same reference against the fp64 one on the case's own inputs (the rule of tests/test_op_forms_gpu.py
for the activation backward), per output.  No bound comes from a kernel's output.  Every case prints, per output, its error, its
bound and their ratio.

Measured on an MI355X when the table was added (355 cases, 3 s in all, the slowest 0.3 s): under the tolerance rule the largest
error / bound ratio of an output is 0.023 (general z32x32.deep.ring KC.RC.PLAIN zN accumulate, C of the first problem: 5.7e-6 against
2.5e-4); under the floor rule the largest kernel / floor ratio is 1.35 of the 8 allowed (general 64x16.shallow.ring KC.KC.PLAIN k1 sigmoid
bias_cols save_act gate_gap, save_act: 1.91e-7 against a floor of 1.42e-7).  A library built with ft_epilogue's `plain` widened to ignore
the activation fails the two throughput-kernel cases whose only epilogue term is an activation (errors of 9 and 10); one built with the
gating product moved in front of save_act in epilogue_store_col4 fails save_act (errors of 4 .. 5) in the ten gated cases of the general
template and of gemm_tinyk_kernel."""
import ctypes as C

import pytest
import torch

import gemm_cases as G
import op_forms as F
from nasrec_amd import _lib as L
from nasrec_amd import plan as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_gemm_form_against_fp64(lib, case):
    b = case.build("cuda")
    assert F.GEMM_FAMILY.get(P.gemm_route(b.desc)[0]) == case.family, "the routing rule no longer sends this case to %s" % case.family
    init = {k: v.clone() for k, v in b.outs.items() if k != "workspace"}
    for d in b.descs:
        L.check(lib.nasrec_launch(None, C.addressof(d)))
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in b.outs.items()}
    assert any(not torch.equal(init[k], got[k]) for k in init), "a launch that leaves every buffer as it was compares nothing"
    print(case.name)
    b.check(got)
