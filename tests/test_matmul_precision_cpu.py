"""Matmul precision (DESIGN.md "Matmul precision"), the host side: the descriptor field and its layout check, routing that does not
depend on it, the kernel name, rejection of unknown values, the public argument / environment variable / CLI flag, and a plan compiled
on the host carrying the value on every GEMM descriptor.  No device needed."""
import ctypes as C

import pytest

from nasrec_amd import _lib as L
from nasrec_amd import plan as P

KC, RC, TOKR, TOKK, PLAIN, TOKJ = L.AM_KC, L.AM_RC, L.AM_TOKR, L.AM_TOKK, L.CM_PLAIN, L.CM_TOKJ
PRECISIONS = (L.PRECISION_HIGHEST, L.PRECISION_HIGH, L.PRECISION_MEDIUM)


def _desc(binding, segs, zmode=0, splitk=1, precision=None, **kw):
    d = L.GemmDesc()
    d.kind = L.OP_GEMM
    d.amode, d.bmode, d.cmode = binding
    d.nseg, d.zmode, d.splitk, d.dims_in_use = len(segs), zmode, splitk, -1
    for k, v in kw.items():
        setattr(d, k, v)
    for q, (m, n, k) in enumerate(segs):
        s = d.seg[q]
        s.A, s.B, s.C, s.M, s.N, s.K, s.Mvalid = 0x1000, 0x2000, 0x3000, m, n, k, m
        s.lda, s.ldb, s.ldc = (k if binding[0] == KC else m), (k if binding[1] == KC else n), n
    if precision is not None:
        d.precision = precision
    return d


# (binding, segments, zmode, splitk, family): throughput launches of the three bindings and launches of every other family
CASES = [
    ((KC, KC, PLAIN), [(2048, 1035, 300)], 0, 1, L.GEMM_ROUTE_FAST),
    ((KC, KC, PLAIN), [(2048, 1035, 13), (2048, 1035, 200)], 0, 2, L.GEMM_ROUTE_FAST),
    ((KC, RC, PLAIN), [(2048, 1035, 512), (2048, 1024, 512)], 1, 1, L.GEMM_ROUTE_FAST),
    ((RC, RC, PLAIN), [(1024, 1024, 2048)] * 8, 1, 1, L.GEMM_ROUTE_FAST),
    ((KC, KC, PLAIN), [(64, 64, 64)], 0, 1, L.GEMM_ROUTE_GENERAL),
    ((KC, KC, PLAIN), [(256, 1024, 5133)], 0, 1, L.GEMM_ROUTE_KSLICE),
    ((KC, KC, PLAIN), [(4096, 8, 1024)], 0, 1, L.GEMM_ROUTE_SKINNY_N),
    ((KC, KC, PLAIN), [(4096, 1024, 13)], 0, 1, L.GEMM_ROUTE_TINYK),
]


def test_descriptor_carries_the_precision_and_the_layout_check_sees_it():
    lib = L.load()
    assert [n for n, _ in L.GemmDesc._fields_][-2:] == ["precision", "_pad_precision"]
    assert L.GemmDesc.precision.offset == L.GemmDesc.seg.offset + C.sizeof(L.GemmSeg) * L.MAX_SEGS  # appended: the head did not move
    assert L.GemmDesc().precision == L.PRECISION_HIGHEST == 0  # a zero-initialised descriptor is fp32
    sizes = (C.c_int32 * 43)()
    n = lib.nasrec_desc_sizes(sizes, 43)
    assert n > L.OP_SPLITK_EPILOGUES
    assert sizes[L.OP_GEMM] == C.sizeof(L.GemmDesc)
    assert sizes[L.OP_SPLITK_EPILOGUES] == C.sizeof(L.SplitkEpiloguesDesc)  # the container that embeds descriptors grew with them
    assert sizes[L.OP_WORKLIST] == C.sizeof(L.WorklistDesc)
    assert lib.nasrec_abi_version() == 17
    assert (L.PRECISION_HIGHEST, L.PRECISION_HIGH, L.PRECISION_MEDIUM) == (0, 1, 2)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_route_and_mask_do_not_depend_on_the_precision(case):
    binding, segs, zmode, splitk, family = CASES[case]
    routes = [P.gemm_route(_desc(binding, segs, zmode, splitk, precision=p)) for p in PRECISIONS]
    assert routes[0][0] == family, "the case must be sized for its family"
    assert routes[0] == routes[1] == routes[2] == P.gemm_route(_desc(binding, segs, zmode, splitk))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernel_name_is_the_bf16_body_exactly_for_throughput_launches_with_reduced_precision(case):
    binding, segs, zmode, splitk, family = CASES[case]
    base = P.gemm_kernel_name(_desc(binding, segs, zmode, splitk))
    assert base != "gemm_fast_bf16_kernel" and (base == "gemm_fast_kernel") == (family == L.GEMM_ROUTE_FAST)
    for p in PRECISIONS:
        name = P.gemm_kernel_name(_desc(binding, segs, zmode, splitk, precision=p))
        assert name == ("gemm_fast_bf16_kernel" if (family == L.GEMM_ROUTE_FAST and p != L.PRECISION_HIGHEST) else base)


def test_bf16_launch_count_counts_throughput_launches_only():
    descs = [_desc(b, s, z, k, precision=L.PRECISION_MEDIUM) for b, s, z, k, _ in CASES]
    assert P.bf16_launches(descs) == sum(1 for c in CASES if c[4] == L.GEMM_ROUTE_FAST)
    assert P.bf16_launches([_desc(b, s, z, k) for b, s, z, k, _ in CASES]) == 0


@pytest.mark.parametrize("bad", [7, -1, 3])
def test_unknown_precision_is_rejected_with_a_message(bad):
    lib = L.load()
    for binding, segs, zmode, splitk, _ in (CASES[0], CASES[4]):
        d = _desc(binding, segs, zmode, splitk, precision=bad)
        assert P.gemm_route(d) == (L.GEMM_ROUTE_BAD_PRECISION, 0)
        with pytest.raises(ValueError):
            P.gemm_kernel_name(d)
        # the launcher refuses the descriptor before it touches a device
        assert lib.nasrec_launch(None, C.addressof(d)) != 0
        msg = lib.nasrec_last_error().decode()
        assert "precision" in msg and str(bad) in msg
        with pytest.raises(L.EngineError):
            L.check(lib.nasrec_gemm(None, C.addressof(d)))


def _tiny_supernet(**kw):
    from nasrec_amd.search_space import ops_config_lib
    from nasrec_amd.supernet.supernet import SuperNet
    return SuperNet(num_blocks=1, ops_config=ops_config_lib["autoctr"], use_layernorm=False, num_embeddings=[11] * 26, **kw)


def test_supernet_argument_is_validated(monkeypatch):
    monkeypatch.delenv(L.MATMUL_PRECISION_ENV, raising=False)
    with pytest.raises(ValueError):
        _tiny_supernet(matmul_precision="fast")
    assert _tiny_supernet()._matmul_precision == "highest"
    for name in ("highest", "high", "medium"):
        m = _tiny_supernet(matmul_precision=name)
        assert m._matmul_precision == name
        # operators run on their own (opexec.run) take their owner's precision
        assert all(sub.__dict__["_matmul_precision"] == name for sub in m.modules())


def test_environment_default_is_honoured(monkeypatch):
    monkeypatch.setenv(L.MATMUL_PRECISION_ENV, "medium")
    assert L.matmul_precision_name(None) == "medium"
    assert _tiny_supernet()._matmul_precision == "medium"
    assert _tiny_supernet(matmul_precision="high")._matmul_precision == "high"  # the argument wins
    monkeypatch.setenv(L.MATMUL_PRECISION_ENV, "fast")
    with pytest.raises(ValueError):
        _tiny_supernet()  # a typo must not silently run fp32
    monkeypatch.delenv(L.MATMUL_PRECISION_ENV)
    assert L.matmul_precision_name(None) == "highest"
    monkeypatch.setenv(L.MATMUL_PRECISION_ENV, "")
    assert L.matmul_precision_name(None) == "highest"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_plan_compiled_on_the_host_carries_the_precision_on_every_gemm_descriptor(precision):
    """the supernet's full path at batch 2048 through the plan compiler, with host tensors standing in for the device's (the compiler
    only takes their addresses; nothing is launched): forward and backward programs"""
    import torch
    from nasrec_amd.search_space import ops_config_lib
    cfg = P.NetConfig(2, ops_config_lib["xlarge"], True)
    choice = P.full_path_choice(cfg)
    B, Fd, Fs, E = 2048, 13, 26, 16
    shapes = P.infer_param_shapes(cfg, choice, Fd, Fs, [11] * Fs)
    params = {n: torch.zeros(s) for n, s in shapes.items() if not n.startswith("_embedding.")}
    ctx = P.Ctx(B, torch.device("cpu"), params, {n: torch.zeros_like(t) for n, t in params.items()}, shape_only=False, train=True)
    assert ctx.matmul_precision == L.PRECISION_HIGHEST
    ctx.matmul_precision = precision
    d_last, s_last = P.network_walk(ctx, cfg, choice, P.DV(P.Buf(ctx, B * Fd, False), 0, Fd, Fd), P.SV(ctx.buf(B * Fs * E), 0, Fs, Fs * E))
    for v in d_last + s_last:
        v.buf.grad_tensor()
        v.buf.mark(*v.cols())
    ctx.build_backward()
    gemms = [d for d in list(ctx.fwd) + list(ctx.bwd) if isinstance(d, L.GemmDesc)]
    assert len(gemms) > 20 and any(isinstance(d, L.GemmDesc) for d in ctx.bwd)
    assert all(d.precision == precision for d in gemms)
    fast = [d for d in gemms if P.gemm_route(d)[0] == L.GEMM_ROUTE_FAST]
    assert fast, "a batch-2048 supernet plan has throughput launches"
    assert P.bf16_launches(gemms) == (len(fast) if precision else 0)
    assert {P.gemm_kernel_name(d) for d in fast} == {"gemm_fast_bf16_kernel" if precision else "gemm_fast_kernel"}


@pytest.mark.parametrize("module", ["main_train", "train_supernet", "eval_subnet_from_supernet", "eval_subnet_from_scratch"])
def test_every_cli_parser_accepts_the_flag(module):
    import importlib
    mod = importlib.import_module("nasrec_amd." + module)
    p = mod.build_parser()
    assert p.parse_args([]).matmul_precision == "highest"
    for name in ("highest", "high", "medium"):
        assert p.parse_args(["--matmul-precision", name]).matmul_precision == name
    with pytest.raises(SystemExit):
        p.parse_args(["--matmul-precision", "fast"])
