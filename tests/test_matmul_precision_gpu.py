"""Matmul precision end to end (DESIGN.md "Matmul precision"): one operator through its single-operator plan, and one supernet through
the engine at a batch size where some of its products are throughput launches — which launches take the bf16 body, what it does to
the logits against the fp64 oracle, that "highest" is bit for bit the engine without the argument, and that a few fused training
steps in "medium" stay sane."""
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


def test_one_operator_in_medium_through_its_single_operator_plan():
    """ElasticLinear forward + autograd backward at B = 2048, in = 1035, out = 1024.  The three throughput launches are y = x W^T + b
    (16 x 8 tiles) and the first 1024 columns of dx = dy W (16 x 8) and of dW = dy^T x (8 x 8, split-K by the planner): each against
    fp64 torch on the bf16-rounded operands with the MEDIUM bound (Kt + 8) u S, Kt = the contraction length (+ 8 u |b| where the bias
    is added).  The planner cuts the 11 remainder columns of dx and dW (1035 = 8 x 128 + 11), with the bias gradient's ones column,
    into problems of their own for the small-tile kernel (plan._split_column_remainder), at every precision: those columns are fp32
    products — the precision is a permission only throughput launches take up — and are held to the same (Kt + 8) u S on the
    UNROUNDED operands, the bound of an fp32 FMA chain in any order."""
    from nasrec_amd.supernet.modules import ElasticLinear
    torch.manual_seed(31)
    B, nin, nout, nmain = 2048, 1035, 1024, 1024
    lin = ElasticLinear(fixed=True, use_layernorm=False, max_dims_or_dims=nout, activation="identity").cuda()
    lin._matmul_precision = "medium"
    x = torch.randn(B, nin, device="cuda", requires_grad=True)
    with torch.no_grad():
        lin(x.detach(), nout)  # materialises the lazy Linear
        lin._linear.weight.copy_(torch.randn(nout, nin, device="cuda") * 0.05)
        lin._linear.bias.copy_(torch.randn(nout, device="cuda"))
    W, b = lin._linear.weight, lin._linear.bias
    dy = torch.randn(B, nout, device="cuda")
    y = lin(x, nout)
    (y * dy).sum().backward()
    plans = [p for p in lin.__dict__["_op_plans"].values() if p.train]
    assert len(plans) == 1 and plans[0].matmul_precision == "medium"
    assert plans[0].bf16_launches == 3
    names = [P.gemm_kernel_name(d) for d in plans[0].ctx.fwd + plans[0].ctx.bwd if isinstance(d, L.GemmDesc)]
    assert names.count("gemm_fast_bf16_kernel") == 3 and "gemm_fast_kernel" not in names
    x32, w32, g32 = x.detach().double(), W.detach().double(), dy.double()
    xx, ww, gg = _bf(x.detach()), _bf(W.detach()), _bf(dy)
    _within(y.detach(), xx @ ww.t() + b.detach().double(), (nin + 8) * U * (xx.abs() @ ww.abs().t()) + 8 * U * b.detach().double().abs(), "y")
    _within(x.grad[:, :nmain], gg @ ww[:, :nmain], (nout + 8) * U * (gg.abs() @ ww[:, :nmain].abs()), "dx (bf16 body)")
    _within(x.grad[:, nmain:], g32 @ w32[:, nmain:], (nout + 8) * U * (g32.abs() @ w32[:, nmain:].abs()), "dx (fp32 remainder columns)")
    _within(W.grad[:, :nmain], gg.t() @ xx[:, :nmain], (B + 8) * U * (gg.abs().t() @ xx[:, :nmain].abs()), "dW (bf16 body)")
    _within(W.grad[:, nmain:], g32.t() @ x32[:, nmain:], (B + 8) * U * (g32.abs().t() @ x32[:, nmain:].abs()), "dW (fp32 remainder columns)")
    _within(b.grad, g32.sum(0), (B + 8) * U * g32.abs().sum(0), "db (fp32: the ones column rides on the remainder problem)")


CASE = "supernet_autoctr_single"  # the smallest supernet fixture of tests/test_parity_gpu.py
B = 2048


@pytest.fixture(scope="module")
def net():
    """the fixture's network at batch 2048: inputs, the fp64 oracle's logits (computed once), and one engine per precision with the
    same name-seeded weights"""
    z, meta = load_golden(os.path.join(GOLDEN, CASE + ".npz"))
    cfg = P.NetConfig(meta["num_blocks"], ops_config_lib[meta["config"]], meta["use_layernorm"], meta["activation"], fixed=False,
                      last_n_blocks_out=meta.get("last_n_blocks_out", 1))
    Fd, Fs = z["int_x"].shape[1], z["cat_x"].shape[1]
    int_x, cat_x, y = O.synthetic_batch(B, Fd, meta["tables"], seed=77)
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


def test_which_launches_of_a_network_take_the_bf16_body(net):
    choice = net["meta"]["choice"]
    assert net["engines"][None].matmul_precision == "highest"
    counts = {}
    for train in (False, True):
        cp = net["engines"]["highest"].compile(choice, B, train=train)
        descs = cp.fwd.descs + (cp.bwd.descs if train else [])
        fast = sum(1 for d in descs if isinstance(d, L.GemmDesc) and P.gemm_kernel_name(d) == "gemm_fast_kernel")
        assert cp.bf16_launches == 0 and fast > 0
        for name in ("high", "medium"):
            eng = net["engines"][name]
            assert eng.matmul_precision == name
            cq = eng.compile(choice, B, train=train)
            assert cq.bf16_launches == fast
            qd = cq.fwd.descs + (cq.bwd.descs if train else [])
            assert sum(1 for d in qd if isinstance(d, L.GemmDesc) and P.gemm_kernel_name(d) == "gemm_fast_bf16_kernel") == fast
            # the precision changes no routing decision: same launches, same split-K, in the same order
            assert [(type(d).__name__, getattr(d, "splitk", None)) for d in qd] == [(type(d).__name__, getattr(d, "splitk", None)) for d in descs]
        counts[train] = fast
    print("throughput launches of %s at B = %d: forward %d, forward + backward %d" % (CASE, B, counts[False], counts[True]))


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
    """a sanity rail, not a parity bar: finite, and within the step-0 loss of what fp32 products give"""
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
