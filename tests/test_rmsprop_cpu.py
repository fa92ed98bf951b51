"""`--optimizer rmsprop` without a GPU: build_optimizer's LazyRMSprop and its OptimSpec, the harness's choice of route (weight decay on
the dense parameters alone is fused, a regularised table, AMP, row sharding and every torch option the fused step does not reproduce
keep the torch route), LazyRMSprop.step() without an engine against torch.optim.RMSprop bit for bit, the descriptor's layout, and the
lazy rule itself: `lazy_rmsprop_reference`, an fp64 NumPy restatement of the kernel's row arithmetic with the flush — the reference of
the GPU kernel test — against dense RMSprop in fp64."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import LazyRMSprop


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self.ln = torch.nn.LayerNorm(3)
        self._final = torch.nn.Linear(3, 1)

    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


def test_build_optimizer_returns_a_lazy_rmsprop_with_its_spec():
    m = _Tiny()
    opt = MT.build_optimizer("rmsprop", m, 0.05)
    assert type(opt) is LazyRMSprop and isinstance(opt, torch.optim.RMSprop)
    g = opt.param_groups[0]
    assert g["lr"] == 0.05 and g["alpha"] == 0.99 and g["eps"] == 1e-8 and g["momentum"] == 0 and not g["centered"]
    spec = OptimSpec.from_optimizer(opt)
    assert spec == OptimSpec("rmsprop", alpha=0.99, eps=1e-8)
    assert spec.moments and spec.state_keys == ("square_avg",)
    assert OptimSpec.for_step(opt) == spec
    assert OptimSpec.for_step(opt, 1e-8, "_embedding") == spec._replace(wd=1e-8, no_reg="_embedding")
    assert OptimSpec.for_step(opt, 1e-8, None) is None and OptimSpec.for_step(opt, 1e-8, "lin") is None
    assert OptimSpec("adam") == OptimSpec("adam", alpha=0.99)  # (the appended field keeps existing equalities)
    with pytest.raises(KeyError):
        MT.build_optimizer("ds-optimizer", m, 0.05)


def test_routing():
    m = _Tiny()
    opt = MT.build_optimizer("rmsprop", m, 0.05)
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8, "_embedding"), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), False) is False   # the tables are regularised
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), True) is False     # AMP
    m._table_sharding = "row"
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False
    m._table_sharding = None
    # a hand-built torch.optim.RMSprop keeps the torch route
    assert TU._fused_step_applies(m, torch.optim.RMSprop(m.parameters(), lr=0.05), TU.L2Loss(0.0), False) is False


@pytest.mark.parametrize("kw", [dict(momentum=0.9), dict(centered=True), dict(weight_decay=1e-4), dict(maximize=True), dict(capturable=True),
                                dict(differentiable=True)], ids=lambda kw: next(iter(kw)))
def test_options_the_fused_step_does_not_reproduce(kw):
    m = _Tiny()
    opt = LazyRMSprop(m.parameters(), lr=0.05, **kw)
    assert OptimSpec.from_optimizer(opt) is None
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False


def test_two_parameter_groups_keep_the_torch_route():
    m = _Tiny()
    opt = LazyRMSprop([{"params": list(m._embedding.parameters())}, {"params": [p for n, p in m.named_parameters() if not n.startswith("_embedding.")]}],
                      lr=0.05)
    assert OptimSpec.from_optimizer(opt) is None
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False


def test_the_last_layer_step_keeps_the_torch_route():
    class _LL(_Tiny):
        def engine_last_layer_step(self, *a, **k):
            raise AssertionError("not called here")

        def _last_layer_only(self):
            return True
    m = _LL()
    assert TU._last_layer_step_applies(m, MT.build_optimizer("adam", m, 0.05), TU.L2Loss(0.0), False) is True
    assert TU._last_layer_step_applies(m, MT.build_optimizer("rmsprop", m, 0.05), TU.L2Loss(0.0), False) is False


def test_step_without_an_engine_is_torch_rmsprop_bit_for_bit():
    torch.manual_seed(2)
    a, b = _Tiny(), _Tiny()
    b.load_state_dict(a.state_dict())
    oa, ob = MT.build_optimizer("rmsprop", a, 0.05), torch.optim.RMSprop(b.parameters(), lr=0.05)
    for k in range(4):
        x, ids = torch.randn(6, 4), torch.randint(0, 5, (6,))
        for m in (a, b):
            for p in m.parameters():
                p.grad = None
            out = m._final(m.ln(m.lin(x))).view(-1) + m._embedding[0](ids).sum(1)  # (table 1 never has a gradient)
            out.square().mean().backward()
        oa.step()
        ob.step()
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        assert torch.equal(p, pb[n]), n
        assert (p in oa.state) == (pb[n] in ob.state), n
        if p not in oa.state:
            continue
        assert set(oa.state[p]) == set(ob.state[pb[n]]), n
        for k, v in oa.state[p].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(ob.state[pb[n]][k])), (n, k)
    assert set(oa.state[a._final.weight]) == {"step", "square_avg"} and a._embedding[1].weight not in oa.state
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and set(sa["state"]) == set(sb["state"])
    # the flush hook runs first in step() and state_dict(), and is no part of a checkpoint
    calls = []
    oa._lazy_flush = lambda: calls.append(1)
    oa.step()
    assert calls == [1]
    assert "_lazy_flush" not in str(oa.state_dict()["param_groups"]) and calls == [1, 1]


def test_descriptor_layout_matches_the_header():
    """the stamps travel in the slots of `tm` (a union in the header): the structure keeps its size, and the binding's own check
    (load) compares it with the library's"""
    lib = L.load()
    assert lib.nasrec_abi_version() == 17
    sizes = (C.c_int32 * 43)()
    n = lib.nasrec_desc_sizes(sizes, 43)
    assert n > L.OP_OPT_MOMENTS and sizes[L.OP_OPT_MOMENTS] == C.sizeof(L.OptMomentsDesc)
    assert L.OptMomentsDesc.tv.offset == L.OptMomentsDesc.tm.offset + 8 * L.MAX_TABLES
    assert L.OPTIM_RMSPROP == 3


# ---------------------------------------------------------------------------------------------------------------------------------
def lazy_rmsprop_reference(p, v, stamp, step, touched, alpha, eps, lr):
    """One fused RMSprop step on one table, fp64, as the kernel does it (include/nasrec_hip.h): `touched` = {row: clipped summed
    gradient [16]}; p, v [rows, 16] float64 and stamp [rows] int64 are updated in place; step = the table's count before this step.
    A touched row pays alpha^n for the n steps it rested, takes RMSprop's update and is stamped; every other row is left alone."""
    t = step + 1
    for row, g in touched.items():
        n = t - 1 - int(stamp[row])
        if n > 0:
            v[row] *= alpha ** n
        v[row] = v[row] * alpha + (1 - alpha) * g * g
        p[row] = p[row] - lr * g / (np.sqrt(v[row]) + eps)
        stamp[row] = t
    return t


def lazy_rmsprop_flush(v, stamp, step, alpha):
    n = step - stamp
    owed = n > 0
    v[owed] *= (alpha ** n[owed].astype(np.float64))[:, None]
    stamp[owed] = step


def test_the_lazy_rule_with_the_flush_is_dense_rmsprop():
    """97 rows, 40 steps, 5 random rows per step (gaps up to 6 and more) and every 7th step all rows; in fp64 the lazy rule with the
    flush and dense RMSprop differ by rounding alone.  The bar |v - v_dense| <= (3 T + 2) 2^-24 v_dense is the one the fp32 kernel
    has to meet (at most three roundings per step — the decay, the multiply, the fused add —, all terms positive); fp64 sits far
    below it, and a wrong power, a stamp off by one or a missed flush sit far above (1 - alpha = 1e-2 per step)."""
    R, T, alpha, eps, lr = 97, 40, 0.99, 1e-8, 0.01
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal((R, 16))
    pl, vl, stamp = p0.copy(), np.zeros((R, 16)), np.zeros(R, np.int64)
    pd, vd = p0.copy(), np.zeros((R, 16))
    step, gaps = 0, 0
    for t in range(1, T + 1):
        rows = np.arange(R) if t % 7 == 0 else rng.permutation(R)[:5]
        g = np.zeros((R, 16))
        g[rows] = rng.standard_normal((len(rows), 16))
        vd = alpha * vd + (1 - alpha) * g * g
        pd = pd - lr * g / (np.sqrt(vd) + eps)
        gaps = max(gaps, int((t - 1 - stamp[rows]).max()))
        before = (pl.copy(), vl.copy(), stamp.copy())
        step = lazy_rmsprop_reference(pl, vl, stamp, step, {int(r): g[r] for r in rows}, alpha, eps, lr)
        rest = np.ones(R, bool)
        rest[rows] = False
        assert all(np.array_equal(x[rest], y[rest]) for x, y in zip(before, (pl, vl, stamp)))
    assert gaps >= 6 and step == T
    assert np.abs(vl - vd).max() > 1e-3  # (before the flush the resting rows are behind)
    lazy_rmsprop_flush(vl, stamp, step, alpha)
    assert (stamp == T).all()
    bar = (3 * T + 2) * 2.0 ** -24
    assert (np.abs(vl - vd) <= bar * vd).all(), float((np.abs(vl - vd) / np.maximum(vd, 1e-300)).max())
    assert np.abs(pl - pd).max() <= 1e-12
    again = vl.copy()
    lazy_rmsprop_flush(vl, stamp, step, alpha)
    assert np.array_equal(again, vl)
