"""Matmul precision on the large-batch token-axis launches, end to end (DESIGN.md "Matmul precision"): one ElasticLinear3D through its
single-operator plan, and one supernet through the engine at batch 1024 — the smallest batch at which its token-axis Linears and their
weight gradients are token_linear / token_dw launches.  Which launches take the bf16 bodies (csrc/token_linear_bf16.hip: token_dw
at "high" and "medium", token_linear at "medium" — its "high" body did not pay on every measured launch and stays fp32), that
"highest" is bit for bit the engine without the argument, what the modes do to the logits against the fp64 oracle, and that a few
fused training steps in "medium" stay sane."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_golden, oracle_cfg, oracle_params
from nasrec_amd import _lib as L
from nasrec_amd import plan as P
from nasrec_amd.engine import SupernetEngine
from nasrec_amd.search_space import ops_config_lib
from oracle import nasrec_oracle as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -23


def _bf(t):
    return t.bfloat16().double()


def _within(got, want, bound, what):
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max err %.3e, max err / bound %.3f" % (what, float(err.max()), ratio))
    assert torch.isfinite(got).all(), what
    assert bool((err <= bound).all()), "%s: max err / bound = %.3f" % (what, ratio)


def test_one_token_axis_operator_in_medium_through_its_single_operator_plan():
    """ElasticLinear3D forward + autograd backward at B = 1024, 26 -> 45 tokens: y[b] = W x[b] + bias (token_linear), dx[b] = W^T dy[b]
    (token_linear, the input-gradient binding) and dW = sum_b dy[b] x[b]^T with the bias gradient as its ones column (token_dw, split-K
    by the planner), each against fp64 torch on the bf16-rounded operands with the MEDIUM bound (Kt + 8) u S, Kt = the contraction
    length (+ 8 u |bias| where the bias is added)."""
    from nasrec_amd.supernet.modules import ElasticLinear3D
    torch.manual_seed(41)
    B, nin, nout, E = 1024, 26, 45, 16
    lin = ElasticLinear3D(fixed=True, use_layernorm=False, max_dims_or_dims=nout, activation="identity").cuda()
    lin._matmul_precision = "medium"
    x = torch.randn(B, nin, E, device="cuda", requires_grad=True)
    with torch.no_grad():
        lin(x.detach(), nout)  # materialises the lazy Linear
        lin._linear.weight.copy_(torch.randn(nout, nin, device="cuda") * 0.2)
        lin._linear.bias.copy_(torch.randn(nout, device="cuda"))
    W, b = lin._linear.weight, lin._linear.bias
    dy = torch.randn(B, nout, E, device="cuda")
    y = lin(x, nout)
    (y * dy).sum().backward()
    plans = [p for p in lin.__dict__["_op_plans"].values() if p.train]
    assert len(plans) == 1 and plans[0].matmul_precision == "medium"
    names = [P.gemm_kernel_name(d) for d in plans[0].ctx.fwd + plans[0].ctx.bwd if isinstance(d, L.GemmDesc)]
    print("launches:", names)
    assert names.count("token_linear_bf16_kernel") == 2 and names.count("token_dw_bf16_kernel") == 1
    assert "token_linear_kernel" not in names and "token_dw_kernel" not in names
    assert plans[0].bf16_token_launches == 3 and plans[0].bf16_launches == 0
    xx, ww, gg, bb = _bf(x.detach()), _bf(W.detach()), _bf(dy), b.detach().double()
    _within(y.detach(), torch.einsum("on,bne->boe", ww, xx) + bb[None, :, None],
            (nin + 8) * U * torch.einsum("on,bne->boe", ww.abs(), xx.abs()) + 8 * U * bb.abs()[None, :, None], "y")
    _within(x.grad, torch.einsum("on,boe->bne", ww, gg), (nout + 8) * U * torch.einsum("on,boe->bne", ww.abs(), gg.abs()), "dx")
    Kt = B * E
    _within(W.grad, torch.einsum("boe,bne->on", gg, xx), (Kt + 8) * U * torch.einsum("boe,bne->on", gg.abs(), xx.abs()), "dW")
    _within(b.grad, gg.sum((0, 2)), (Kt + 8) * U * gg.abs().sum((0, 2)), "db (the ones column of the dW launch: 1.0 is a bf16 value)")


CASE = "supernet_autoctr_single"  # the smallest supernet fixture of tests/test_parity_gpu.py
B = 1024


@pytest.fixture(scope="module")
def net():
    """the fixture's network at batch 1024: inputs, the fp64 oracle's logits (computed once), and one engine per precision with the
    same name-seeded weights"""
    z, meta = load_golden(os.path.join(GOLDEN, CASE + ".npz"))
    cfg = P.NetConfig(meta["num_blocks"], ops_config_lib[meta["config"]], meta["use_layernorm"], meta["activation"], fixed=False,
                      last_n_blocks_out=meta.get("last_n_blocks_out", 1))
    Fd, Fs = z["int_x"].shape[1], z["cat_x"].shape[1]
    int_x, cat_x, y = O.synthetic_batch(B, Fd, meta["tables"], seed=78)
    with torch.no_grad():
        ref = O.supernet_forward(oracle_params(meta), oracle_cfg(meta), int_x.double(), cat_x, meta["choice"], num_embeddings=meta["tables"]).view(-1)
    weights = {k: O.seeded_param(k, shp) for k, shp in meta["param_shapes"].items()}
    old = os.environ.pop(L.MATMUL_PRECISION_ENV, None)
    try:
        engines = {}
        for name in (None, "highest", "high", "medium"):
            kw = {} if name is None else {"matmul_precision": name}
            eng = SupernetEngine(cfg, Fd, Fs, meta["tables"], **kw)
            assert eng.load_params(weights) == []
            engines[name] = eng
    finally:
        if old is not None:
            os.environ[L.MATMUL_PRECISION_ENV] = old
    return dict(meta=meta, weights=weights, int_x=int_x.cuda(), cat_x=cat_x.cuda(), y=y.cuda(), ref=ref.numpy(), engines=engines)


def _families(descs):
    return [P.gemm_route(d)[0] for d in descs if isinstance(d, L.GemmDesc)]


def test_which_launches_of_a_network_take_the_token_bf16_bodies(net):
    choice = net["meta"]["choice"]
    assert net["engines"][None].matmul_precision == "highest"
    cp = net["engines"]["highest"].compile(choice, B, train=True)
    descs = cp.fwd.descs + cp.bwd.descs
    fam = _families(descs)
    n_lin, n_dw = fam.count(L.GEMM_ROUTE_TOKEN_LINEAR), fam.count(L.GEMM_ROUTE_TOKEN_DW)
    assert n_lin >= 1 and n_dw >= 1, "the fixture's plan at this batch must hold launches of both token-axis families"
    assert cp.bf16_token_launches == 0 and cp.bf16_launches == 0
    for train in (False, True):
        cp = net["engines"]["highest"].compile(choice, B, train=train)
        descs = cp.fwd.descs + (cp.bwd.descs if train else [])
        fam = _families(descs)
        lin, dw = fam.count(L.GEMM_ROUTE_TOKEN_LINEAR), fam.count(L.GEMM_ROUTE_TOKEN_DW)
        for name in ("high", "medium"):
            cq = net["engines"][name].compile(choice, B, train=train)
            qd = cq.fwd.descs + (cq.bwd.descs if train else [])
            lin_bf16 = lin if name == "medium" else 0  # (token_linear has a "medium" body only)
            assert cq.bf16_token_launches == lin_bf16 + dw
            names = [P.gemm_kernel_name(d) for d in qd if isinstance(d, L.GemmDesc)]
            assert names.count("token_linear_bf16_kernel") == lin_bf16 and names.count("token_linear_kernel") == lin - lin_bf16
            assert names.count("token_dw_bf16_kernel") == dw and "token_dw_kernel" not in names
            # the precision changes no routing decision: same launches, same split-K, in the same order
            assert [(type(d).__name__, getattr(d, "splitk", None)) for d in qd] == [(type(d).__name__, getattr(d, "splitk", None)) for d in descs]
            assert _families(qd) == fam
    print("token-axis launches of %s at B = %d, forward + backward: %d token_linear, %d token_dw" % (CASE, B, n_lin, n_dw))


def test_logits_of_the_three_modes_against_the_fp64_oracle(net):
    choice, ref = net["meta"]["choice"], net["ref"]
    out = {}
    for name, eng in net["engines"].items():
        out[name] = eng.forward(net["int_x"], net["cat_x"], choice).view(-1).clone()
        eng.check_indices()
        assert torch.isfinite(out[name]).all(), name
    assert torch.equal(out["highest"], out[None]), "'highest' must be bit for bit the engine built without the argument"
    err = {name: float(np.abs(o.cpu().numpy().astype(np.float64) - ref).max()) for name, o in out.items() if name is not None}
    print("max |logit - fp64 oracle| of %s at B = %d (max |logit| %.3f): highest %.3e, high %.3e, medium %.3e"
          % (CASE, B, float(np.abs(ref).max()), err["highest"], err["high"], err["medium"]))
    assert err["high"] < err["medium"]
    assert not torch.equal(out["medium"], out["highest"])


def test_three_fused_training_steps_in_medium_stay_close_to_highest(net):
    """a sanity rail, not a parity bar (no end-to-end tolerance can be derived): finite, and within the step-0 loss of what fp32
    products give"""
    choice = net["meta"]["choice"]
    losses = {}
    for name in ("highest", "medium"):
        eng = net["engines"][name]
        losses[name] = []
        for _ in range(3):
            loss = eng.train_step(net["int_x"], net["cat_x"], net["y"].view(-1), lr=1e-3, choice=choice)
            torch.cuda.synchronize()
            losses[name].append(float(loss.item()))
        assert eng.load_params(net["weights"]) == []  # (the other tests of this module read the engines' logits)
    print("fused-step losses: highest %s, medium %s" % (losses["highest"], losses["medium"]))
    assert all(np.isfinite(v) for v in losses["medium"] + losses["highest"])
    assert abs(losses["medium"][-1] - losses["highest"][-1]) < losses["highest"][0]
