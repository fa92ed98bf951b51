"""`--decoupled-wd LAMBDA` without a GPU: utils/optim.DecoupledWeightDecay against an fp64 restatement of its rule and against
torch.optim.AdamW; the error bar of the lazily paid decay (`decay_bar`, the bar of the GPU tests); the harness's choice of route; the
spec's field; the descriptor's layout; the parsers.

The bar (derived from the rule, not measured; DESIGN.md "Lazy decoupled weight decay").  Against the fp64 product of the same factors
over the same fp32 history, with u = 2^-24 (one round-to-nearest, relative) and M the largest |w| of the element's history:
  * one dense statement p = fl(p * fl(1 - lr lambda)) rounds twice — the factor (1 - lr lambda lies in (1/2, 1]: at most u relative)
    and the product: 2 u M.  Every factor is <= 1, so earlier error does not grow.
  * whatever moves the weights behind the decay (the optimizer; in the kernel test one fp32 addition per step) rounds once more: u M.
  * a row that rests is not walked: it pays exp(L - stamp) in fp64, rounded once (u M), where the stamp is the fp32 value of a level
    |L| <= 1 (u |L| <= u relative): 2 u M for what would have been 2 u M per rested step.  A row in every batch never catches up.
So T steps cost at most 3 T u M on either route; (3 T + 2) u M leaves two roundings for the second-order terms and for the fp64 sum of
logs.  (The form the issue expected, (2 T + 2) u M, counts the factor's own rounding as none.)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd import train_supernet as TS
from nasrec_amd.optim_spec import OptimSpec, regularises_tables
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import DecoupledWeightDecay, WeightEMA


def decay_bar(T, M):
    """the derived bound on |fp32 weights - fp64 weights| after T steps of decay + update, per element (M: array or scalar)"""
    return (3 * T + 2) * 2.0 ** -24 * M


def cosine_lrs(T, hi=1e-2, lo=1e-3):
    """T learning rates from a cosine between hi and lo, rounded to fp32 (what the device scalar holds), as Python floats"""
    return [float(np.float32(lo + 0.5 * (hi - lo) * (1.0 + math.cos(math.pi * t / max(1, T - 1))))) for t in range(T)]


class _Toy(torch.nn.Module):
    """one table and parameters of 1, 2 and 3 dimensions"""

    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16)])
        self.lin = torch.nn.Linear(4, 3)        # lin.weight 2-D, lin.bias 1-D
        self.cube = torch.nn.Parameter(torch.randn(2, 3, 4))
        self.skipped = torch.nn.Parameter(torch.randn(3, 3))  # (never gets a gradient)


class _Tiny(torch.nn.Module):
    """test_weight_ema_cpu.py's stand-in for a SuperNet in the routing questions"""

    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self.ln = torch.nn.LayerNorm(3)
        self._final = torch.nn.Linear(3, 1)

    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


def _give_grads(m, g, skip=("skipped",)):
    for n, p in m.named_parameters():
        p.grad = None if n in skip else torch.randn(p.shape, generator=g)


@pytest.mark.parametrize("no_reg", [None, "_embedding", "lin"])
def test_apply_against_an_fp64_restatement(no_reg):
    lam, T = 0.1, 5
    g = torch.Generator().manual_seed(3)
    m = _Toy()
    dec = DecoupledWeightDecay(m, lam, no_reg)
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    want = {n: p.detach().double().numpy().copy() for n, p in m.named_parameters()}
    chosen = {n for n, p in m.named_parameters() if p.dim() >= 2 and not (no_reg is not None and n.startswith(no_reg))}
    assert [n for n, _ in dec.selected()] == [n for n, _ in m.named_parameters() if n in chosen]
    assert ("_embedding.0.weight" in chosen) == (no_reg != "_embedding") == regularises_tables(lam, no_reg)
    assert ("lin.weight" in chosen) == (no_reg != "lin") and "lin.bias" not in chosen and "cube" in chosen
    lrs = cosine_lrs(T)
    for lr in lrs:
        _give_grads(m, g)
        dec.apply(lr)
        for n in chosen - {"skipped"}:
            want[n] = want[n] * (1.0 - lr * lam)
    for n, p in m.named_parameters():
        if n in chosen and n != "skipped":
            err = np.abs(p.detach().double().numpy() - want[n])
            assert (err <= decay_bar(T, np.abs(start[n].double().numpy()))).all(), n
            assert not torch.equal(p, start[n]), n
        else:  # 1-D, left out by the prefix, or grad is None: the bits stay
            assert torch.equal(p, start[n]), n
    # a table whose backward stopped short of the stem (grad None) does not decay; lambda = 0 is no helper; the bounds
    _give_grads(m, g, skip=("skipped", "_embedding.0.weight"))
    before = m._embedding[0].weight.detach().clone()
    dec.apply(1e-2)
    assert torch.equal(m._embedding[0].weight, before)
    snap = {n: p.detach().clone() for n, p in m.named_parameters()}
    _give_grads(m, g)
    DecoupledWeightDecay(m, 0.0).apply(1e-2)
    assert all(torch.equal(p, snap[n]) for n, p in m.named_parameters())
    with pytest.raises(ValueError):
        DecoupledWeightDecay(m, -0.1)
    with pytest.raises(ValueError):
        dec.apply(10.0)  # lr lambda >= 1
    assert not hasattr(dec, "state_dict")  # (no state: nothing for a checkpoint)


def test_a_bound_helper_flushes_first():
    m = _Toy()
    dec = DecoupledWeightDecay(m, 0.1)
    calls = []
    dec._flush = lambda: calls.append([p.detach().clone() for p in m.parameters()])
    _give_grads(m, torch.Generator().manual_seed(4))
    before = [p.detach().clone() for p in m.parameters()]
    dec.apply(1e-2)
    assert len(calls) == 1 and all(torch.equal(a, b) for a, b in zip(calls[0], before))  # (the hook saw the weights untouched)


class _AllSelected(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.randn(5, 4))
        self.b = torch.nn.Parameter(torch.randn(2, 3, 4))
        self.c = torch.nn.Parameter(torch.randn(9, 16))


def test_apply_and_adam_are_adamw():
    """apply(lr) in front of torch.optim.Adam.step() is torch.optim.AdamW(weight_decay=lambda): five steps, a changing lr.  Both
    multiply by the Python float 1 - lr * lambda; they come out bit for bit, which is what is asserted (rtol 1e-6 is the issue's bar)."""
    lam, T = 0.1, 5
    torch.manual_seed(11)
    m1 = _AllSelected()
    m2 = _AllSelected()
    m2.load_state_dict(m1.state_dict())
    adam, adamw = torch.optim.Adam(m1.parameters(), lr=1e-2), torch.optim.AdamW(m2.parameters(), lr=1e-2, weight_decay=lam)
    dec = DecoupledWeightDecay(m1, lam)
    assert len(dec.selected()) == 3
    g = torch.Generator().manual_seed(12)
    for lr in cosine_lrs(T):
        for opt in (adam, adamw):
            opt.param_groups[0]["lr"] = lr
        for p1, p2 in zip(m1.parameters(), m2.parameters()):
            p1.grad = torch.randn(p1.shape, generator=g)
            p2.grad = p1.grad.clone()
        dec.apply(lr)
        adam.step()
        adamw.step()
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        torch.testing.assert_close(p1, p2, rtol=1e-6, atol=0.0)
        assert torch.equal(p1, p2), n


def test_the_dense_fp32_statement_stays_within_the_bar():
    lam, T = 0.1, 6
    g = torch.Generator().manual_seed(21)
    p = torch.randn(4096, generator=g) * torch.logspace(-3, 3, 4096)
    want = p.double().numpy().copy()
    M = np.abs(want)
    for lr in cosine_lrs(T):
        u = 0.05 * torch.randn(4096, generator=g) * p.abs()
        p.mul_(1 - lr * lam)
        want = want * (1.0 - lr * lam)
        M = np.maximum(M, np.abs(want))
        p.add_(u)  # (the optimizer's stand-in: one fp32 addition)
        want = want + u.double().numpy()
        M = np.maximum(M, np.abs(want))
    err = np.abs(p.double().numpy() - want)
    frac = float((err / decay_bar(T, M)).max())
    print("largest error as a fraction of the bar: %.3f" % frac)
    assert frac <= 1.0
    # the closed form a resting row pays: exp of the fp64 sum of logs is the product, far inside one rounding
    lrs = cosine_lrs(T)
    level = sum(math.log1p(-lr * lam) for lr in lrs)
    assert abs(math.exp(level) / np.prod([1.0 - lr * lam for lr in lrs]) - 1.0) < 1e-14
    assert abs(float(np.float32(level)) - level) <= 2.0 ** -24 * abs(level)


def test_routing_with_a_decay():
    m = _Tiny()
    dec, dense_dec = DecoupledWeightDecay(m, 0.1), DecoupledWeightDecay(m, 0.1, "_embedding")
    ema = WeightEMA(m, 0.9)
    no_wd, dense_wd, table_wd = TU.L2Loss(0.0), TU.L2Loss(1e-8, "_embedding"), TU.L2Loss(1e-8)
    for name in ("adagrad", "row-sparse-adam", "rmsprop"):
        opt = MT.build_optimizer(name, m, 0.05)
        plain = TU._fused_step_spec(m, opt, no_wd, False)
        got = TU._fused_step_spec(m, opt, no_wd, False, decay=dec)
        assert plain is not None and plain.dwd == 0.0 and got == plain._replace(dwd=0.1), name
        assert TU._fused_step_applies(m, opt, no_wd, False, decay=dec) is True
        assert TU._fused_step_spec(m, opt, no_wd, False, decay=dense_dec) == plain._replace(dwd=0.1, no_reg="_embedding"), name
        assert TU._fused_step_spec(m, opt, table_wd, False, decay=dec) is None, name        # an L2 term on the tables
        assert TU._fused_step_spec(m, opt, no_wd, True, decay=dec) is None, name            # AMP
        assert TU._fused_step_spec(m, opt, no_wd, False, ema=ema, decay=dec) is None, name  # a weight EMA, the decay on the tables
        both = TU._fused_step_spec(m, opt, no_wd, False, ema=ema, decay=dense_dec)          # ... and with the tables left out
        assert both == plain._replace(dwd=0.1, no_reg="_embedding", ema=0.9), name
        l2_too = TU._fused_step_spec(m, opt, dense_wd, False, decay=dense_dec)              # L2 and decay, both off the tables
        assert l2_too is not None and l2_too.wd == 1e-8 and l2_too.dwd == 0.1 and l2_too.no_reg == "_embedding", name
        assert "EMA" in TU._decay_route(m, plain, no_wd, dec, ema)
    for name in ("adam", "sgd"):
        opt = MT.build_optimizer(name, m, 0.05)
        assert TU._fused_step_spec(m, opt, no_wd, False) is not None
        assert TU._fused_step_spec(m, opt, no_wd, False, decay=dec) is None, name
        assert TU._fused_step_spec(m, opt, no_wd, False, decay=dense_dec) is None, name
    opt = MT.build_optimizer("adagrad", m, 0.05)
    assert TU._fused_step_spec(m, opt, no_wd, False, decay=dec) is not None
    m._place_embedding_on_cpu = True
    assert TU._fused_step_spec(m, opt, no_wd, False, decay=dec) is None   # tables on the host
    m._place_embedding_on_cpu = False
    m._table_sharding = "row"
    assert TU._fused_step_spec(m, opt, no_wd, False) is not None
    assert TU._fused_step_spec(m, opt, no_wd, False, decay=dec) is None   # row-sharded tables
    m._table_sharding = None
    for p in m.lin.parameters():
        p.requires_grad_(False)
    assert TU._fused_step_spec(m, opt, no_wd, False, decay=dec) is None   # last-layer mode: frozen parameters
    for p in m.lin.parameters():
        p.requires_grad_(True)
    assert TU._fused_step_spec(m, opt, no_wd, False, decay=dec) is not None
    # decay=None: every answer is the one the earlier form gives
    for name in ("adagrad", "adam", "sgd", "row-sparse-adam", "rmsprop"):
        o = MT.build_optimizer(name, m, 0.05)
        for l2 in (no_wd, dense_wd, table_wd):
            for amp in (False, True):
                for e in (None, ema):
                    assert TU._fused_step_spec(m, o, l2, amp, e, decay=None) == TU._fused_step_spec(m, o, l2, amp, e), (name, amp)


def test_a_data_parallel_run_keeps_the_torch_route(monkeypatch):
    from nasrec_amd.utils import dist
    m = _Tiny()
    dec = DecoupledWeightDecay(m, 0.1)
    opt = MT.build_optimizer("adagrad", m, 0.05)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, decay=dec) is not None
    monkeypatch.setattr(dist, "world_info", lambda: (0, 2))
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, decay=dec) is None
    assert TU._decay_route(m, OptimSpec.of(1e-2), TU.L2Loss(0.0), dec) == "data-parallel run"


def test_spec_field():
    assert OptimSpec._field_defaults["dwd"] == 0.0 and OptimSpec("adagrad").dwd == 0.0
    assert OptimSpec("adam") == OptimSpec("adam", 0.9, 0.999, 1e-8, 0.0, False, 0.0, None, False, 0.99)  # (positional uses hold)
    assert OptimSpec.of(1e-2) == OptimSpec("adagrad", eps=1e-2) and OptimSpec.of(1e-2).dwd == 0.0
    assert OptimSpec.of(1e-2, decoupled_wd=0.1) == OptimSpec("adagrad", eps=1e-2, dwd=0.1) != OptimSpec.of(1e-2)
    assert OptimSpec.of(1e-2, no_reg_param_name="_embedding").no_reg is None          # (no_reg counts with wd or dwd only)
    assert OptimSpec.of(1e-2, 1e-8, "_embedding").no_reg == "_embedding"
    assert OptimSpec.of(1e-2, 0.0, "_embedding", decoupled_wd=0.1).no_reg == "_embedding"
    rms = OptimSpec("rmsprop", alpha=0.9)
    assert OptimSpec.of(optim=rms, decoupled_wd=0.5) == rms._replace(dwd=0.5)
    assert OptimSpec.of(optim=rms._replace(dwd=0.5)).dwd == 0.5
    with pytest.raises(ValueError):
        OptimSpec.of(1e-2, decoupled_wd=-0.1)


def test_descriptor_layout_matches_the_header():
    lib = L.load()
    assert lib.nasrec_abi_version() == 17
    sizes = (C.c_int32 * 45)()
    n = lib.nasrec_desc_sizes(sizes, 45)
    assert n == 45 and L.OP_DECOUPLED_DECAY == 44 and sizes[44] == C.sizeof(L.DecoupledDecayDesc)
    assert L.DESC_BY_KIND[L.OP_DECOUPLED_DECAY] is L.DecoupledDecayDesc and hasattr(lib, "nasrec_decoupled_decay")
    D = L.DecoupledDecayDesc
    assert D.mask.offset == 24 and D.n_chunks.offset == 28 and D.lambda_.offset == 32 and D.lr_max.offset == 40 and D.idx.offset == 48
    assert D.table.offset == 64 and D.stamp.offset == D.table.offset + 8 * L.MAX_TABLES
    assert D.tile_off.offset == D.rows.offset + 8 * L.MAX_TABLES and D.bitmap.offset == D.tile_off.offset + 8 * (L.MAX_TABLES + 1)
    assert C.sizeof(D) == D.counter.offset + 8


@pytest.mark.parametrize("mod", [MT, TS])
def test_parsers(mod):
    p = mod.build_parser()
    assert p.parse_args([]).decoupled_wd == 0.0 and p.parse_args(["--decoupled-wd", "0.1"]).decoupled_wd == 0.1
    a = p.parse_args(["--decoupled-wd", "1e-5", "--wd", "1e-8", "--no-reg-param-name", "_embedding"])
    assert (a.decoupled_wd, a.wd, a.no_reg_param_name) == (1e-5, 1e-8, "_embedding")  # (independent of --wd)
    with pytest.raises(SystemExit):
        p.parse_args(["--decoupled-wd", "-0.1"])
