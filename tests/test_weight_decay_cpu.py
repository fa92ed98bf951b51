"""The L2 weight-decay spec of the harness (train_utils.L2Loss), the regularised parameter set the fused step decays
(plan.regularised) and the harness's choice of route for it — without a GPU."""
import torch

from nasrec_amd import plan as P
from nasrec_amd.utils import train_utils as TU


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self.ln = torch.nn.LayerNorm(3)
        self._final = torch.nn.Linear(3, 1)


def test_l2_spec_returns_what_get_l2_loss_returns():
    torch.manual_seed(0)
    m = _Tiny()
    for wd, prefix in [(1e-8, None), (1e-3, None), (1e-3, "_embedding"), (0.5, "lin"), (0.0, None)]:
        spec = TU.L2Loss(wd, prefix)
        assert spec.wd == wd and spec.no_reg_param_name == prefix
        assert torch.equal(spec(m), TU.get_l2_loss(m, wd, prefix))
    ref = sum(float((p.detach().double() ** 2).sum()) for n, p in m.named_parameters() if p.dim() > 1)
    assert abs(float(TU.L2Loss(1e-3)(m).detach()) - 1e-3 * ref) <= 1e-6 * 1e-3 * ref


def test_regularised_set_is_what_get_l2_loss_walks():
    """dim-1 parameters excluded, the name prefix excluded, tables included — the same set as named_parameters()"""
    m = _Tiny()
    shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
    for prefix in (None, "_embedding", "_embedding.1", "lin", "_final"):
        dense, tables = P.regularised(shapes, prefix)
        want = [n for n, p in m.named_parameters() if p.dim() > 1 and not (prefix is not None and n.startswith(prefix))]
        assert dense + ["_embedding.%d.weight" % f for f in tables] == [n for n in want if not n.startswith("_embedding.")] + \
            [n for n in want if n.startswith("_embedding.")]
    assert P.regularised(shapes, None) == (["lin.weight", "_final.weight"], [0, 1])
    assert P.regularised(shapes, "_embedding.1") == (["lin.weight", "_final.weight"], [0])


def test_regularised_set_of_an_engine_parameter_layout():
    """the engine's parameter names and shapes (plan.infer_param_shapes) of a supernet: every 2-D weight of every block — on a
    sampled path or off it — and every table; no bias, no LayerNorm"""
    from nasrec_amd.search_space import ops_config_lib
    cfg = P.NetConfig(2, ops_config_lib["xlarge"], True)
    shapes = P.infer_param_shapes(cfg, P.full_path_choice(cfg), 13, 26, [11] * 26)
    dense, tables = P.regularised(shapes)
    assert tables == list(range(26))
    assert dense and all(len(shapes[n]) >= 2 for n in dense)
    assert {n for n, s in shapes.items() if len(s) >= 2 and not n.startswith("_embedding.")} == set(dense)


class _FakeEngineModel(_Tiny):
    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


def test_fused_step_route_for_weight_decay(monkeypatch):
    m = _FakeEngineModel()
    opt = torch.optim.Adagrad(m.parameters(), lr=0.1, eps=1e-2)
    from nasrec_amd.utils import dist as D
    monkeypatch.setattr(D, "world_info", lambda: (0, 1))
    # an opaque callable: only a zero L2 term takes the fused step (unchanged behaviour)
    assert TU._fused_step_applies(m, opt, lambda mm: TU.get_l2_loss(mm, 0.0, None), False) is True
    assert TU._fused_step_applies(m, opt, lambda mm: TU.get_l2_loss(mm, 1e-8, None), False) is False
    # the spec: any wd
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-3, "_embedding"), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is True
    # AMP, torch's own weight decay: torch route as before
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), True) is False
    assert TU._fused_step_applies(m, torch.optim.Adagrad(m.parameters(), lr=0.1, weight_decay=1e-4), TU.L2Loss(1e-8), False) is False
    # row-sharded tables and more than one process keep the torch route with weight decay
    m._table_sharding = "row"
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), False) is False
    m._table_sharding = None
    monkeypatch.setattr(D, "world_info", lambda: (0, 2))
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), False) is False
