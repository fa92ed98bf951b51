"""Matmul precision on the large-batch token-axis launches (DESIGN.md "Matmul precision"), the host side: routing that does not
depend on the precision, the kernel names of the two bf16 bodies (csrc/token_linear_bf16.hip: token_dw at "high" and "medium",
token_linear at "medium" — its "high" body did not pay on every measured launch and stays fp32), the two launch counters, and a plan
compiled on the host reporting both.  No device needed."""
import pytest

from nasrec_amd import _lib as L
from nasrec_amd import plan as P

from test_matmul_precision_cpu import CASES, _desc

KC, RC, TOKR, TOKK, PLAIN, TOKJ = L.AM_KC, L.AM_RC, L.AM_TOKR, L.AM_TOKK, L.CM_PLAIN, L.CM_TOKJ
PRECISIONS = (L.PRECISION_HIGHEST, L.PRECISION_HIGH, L.PRECISION_MEDIUM)
B = 1024


def _tok(binding, segs, zmode=0, splitk=1, precision=None):
    """a token-axis descriptor: (M, N, K) per segment with the leading dimensions of [B, tokens, 16] slabs"""
    d = _desc(binding, segs, zmode, splitk, precision=precision)
    for q, (m, n, k) in enumerate(segs):
        s = d.seg[q]
        if binding[2] == TOKJ:
            s.lda, s.ldb, s.ldc = (k if binding[0] == KC else m), k * 16, m * 16
        else:
            s.lda, s.ldb, s.ldc = m * 16, n * 16, n
    if splitk > 1:
        d.workspace = 0x4000  # (a dummy: nothing is launched)
    return d


BOTH, MEDIUM_ONLY = (L.PRECISION_HIGH, L.PRECISION_MEDIUM), (L.PRECISION_MEDIUM,)
# (name, builder, family, fp32 kernel, bf16 kernel, precisions at which the launcher takes the bf16 kernel)
TOKEN_CASES = [
    ("forward", lambda p: _tok((KC, TOKR, TOKJ), [(45, B * 16, 26), (45, B * 16, 72), (45, B * 16, 9)], precision=p),
     L.GEMM_ROUTE_TOKEN_LINEAR, "token_linear_kernel", "token_linear_bf16_kernel", MEDIUM_ONLY),
    ("input gradient", lambda p: _tok((RC, TOKR, TOKJ), [(72, B * 16, 64), (66, B * 16, 64)], zmode=1, precision=p),
     L.GEMM_ROUTE_TOKEN_LINEAR, "token_linear_kernel", "token_linear_bf16_kernel", MEDIUM_ONLY),
    ("weight gradient", lambda p: _tok((TOKK, TOKK, PLAIN), [(45, 72, B * 16), (45, 9, B * 16)], zmode=1, splitk=4, precision=p),
     L.GEMM_ROUTE_TOKEN_DW, "token_dw_kernel", "token_dw_bf16_kernel", BOTH),
]


@pytest.mark.parametrize("case", range(len(TOKEN_CASES)))
def test_route_and_mask_of_token_launches_do_not_depend_on_the_precision(case):
    _, build, family, _, _, _ = TOKEN_CASES[case]
    routes = [P.gemm_route(build(p)) for p in PRECISIONS]
    assert routes[0][0] == family, "the case must be sized for its family"
    assert routes[0] == routes[1] == routes[2] == P.gemm_route(build(None))
    assert routes[0][1] & (1 << family)


@pytest.mark.parametrize("case", range(len(TOKEN_CASES)))
def test_kernel_name_of_a_token_launch_is_its_bf16_body_at_reduced_precision(case):
    _, build, _, fp32, bf16, takes = TOKEN_CASES[case]
    assert P.gemm_kernel_name(build(None)) == fp32
    assert P.gemm_kernel_name(build(L.PRECISION_HIGHEST)) == fp32
    assert P.gemm_kernel_name(build(L.PRECISION_HIGH)) == (bf16 if L.PRECISION_HIGH in takes else fp32)
    assert P.gemm_kernel_name(build(L.PRECISION_MEDIUM)) == bf16


def test_kernel_names_of_the_other_families_are_what_they_were():
    for binding, segs, zmode, splitk, family in CASES:
        base = P.gemm_kernel_name(_desc(binding, segs, zmode, splitk))
        assert not base.startswith("token_")
        for p in PRECISIONS:
            name = P.gemm_kernel_name(_desc(binding, segs, zmode, splitk, precision=p))
            assert name == ("gemm_fast_bf16_kernel" if (family == L.GEMM_ROUTE_FAST and p != L.PRECISION_HIGHEST) else base)


def test_each_counter_counts_its_own_families_only():
    for p in (L.PRECISION_HIGH, L.PRECISION_MEDIUM):
        mixed = [_desc(b, s, z, k, precision=p) for b, s, z, k, _ in CASES] + [c[1](p) for c in TOKEN_CASES]
        assert P.bf16_launches(mixed) == sum(1 for c in CASES if c[4] == L.GEMM_ROUTE_FAST)
        assert P.bf16_token_launches(mixed) == sum(1 for c in TOKEN_CASES if p in c[5])
    for p in (None, L.PRECISION_HIGHEST):
        mixed = [_desc(b, s, z, k, precision=p) for b, s, z, k, _ in CASES] + [c[1](p) for c in TOKEN_CASES]
        assert P.bf16_launches(mixed) == 0 and P.bf16_token_launches(mixed) == 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_plan_compiled_on_the_host_reports_both_counters(precision):
    """a one-block supernet's full path at batch 1024 through the plan compiler, with host tensors standing in for the device's (the
    compiler only takes their addresses; nothing is launched)"""
    import torch
    from nasrec_amd.search_space import ops_config_lib
    cfg = P.NetConfig(1, ops_config_lib["autoctr"], False)
    choice = P.full_path_choice(cfg)
    Fd, Fs, E = 13, 26, 16
    shapes = P.infer_param_shapes(cfg, choice, Fd, Fs, [11] * Fs)
    params = {n: torch.zeros(s) for n, s in shapes.items() if not n.startswith("_embedding.")}
    ctx = P.Ctx(B, torch.device("cpu"), params, {n: torch.zeros_like(t) for n, t in params.items()}, shape_only=False, train=True)
    ctx.matmul_precision = precision
    d_last, s_last = P.network_walk(ctx, cfg, choice, P.DV(P.Buf(ctx, B * Fd, False), 0, Fd, Fd), P.SV(ctx.buf(B * Fs * E), 0, Fs, Fs * E))
    for v in d_last + s_last:
        v.buf.grad_tensor()
        v.buf.mark(*v.cols())
    ctx.build_backward()
    descs = list(ctx.fwd) + list(ctx.bwd)
    gemms = [d for d in descs if isinstance(d, L.GemmDesc)]
    families = [P.gemm_route(d)[0] for d in gemms]
    fast = families.count(L.GEMM_ROUTE_FAST)
    tok_lin, tok_dw = families.count(L.GEMM_ROUTE_TOKEN_LINEAR), families.count(L.GEMM_ROUTE_TOKEN_DW)
    assert tok_lin > 0 and tok_dw > 0, "a batch-1024 supernet plan has large-batch token-axis launches of both families"
    lin_bf16 = tok_lin if precision == L.PRECISION_MEDIUM else 0  # (token_linear has a "medium" body only)
    dw_bf16 = tok_dw if precision else 0
    assert P.bf16_launches(descs) == (fast if precision else 0)
    assert P.bf16_token_launches(descs) == lin_bf16 + dw_bf16
    names = [P.gemm_kernel_name(d) for d in gemms]
    assert names.count("token_linear_bf16_kernel") == lin_bf16 and names.count("token_linear_kernel") == tok_lin - lin_bf16
    assert names.count("token_dw_bf16_kernel") == dw_bf16 and names.count("token_dw_kernel") == tok_dw - dw_bf16
