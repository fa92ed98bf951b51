"""Which torch optimizers the fused engine step stands in for (train_utils._fused_step_applies, optim_spec.OptimSpec): the reference's
Adam and Nesterov-momentum SGD (main_train.py:150-160) are accepted; every configuration the fused Adam / SGD does not reproduce keeps
the torch route; Adagrad's answers are unchanged — without a GPU."""
import pytest
import torch

from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self.ln = torch.nn.LayerNorm(3)
        self._final = torch.nn.Linear(3, 1)

    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


@pytest.fixture
def one_process(monkeypatch):
    from nasrec_amd.utils import dist as D
    monkeypatch.setattr(D, "world_info", lambda: (0, 1))
    return D


def _zero_l2(m):
    return TU.get_l2_loss(m, 0.0, None)


def test_reference_optimizers_take_the_fused_step(one_process):
    m = _Tiny()
    adam, sgd = MT.build_optimizer("adam", m, 1e-3), MT.build_optimizer("sgd", m, 0.05)
    assert OptimSpec.from_optimizer(adam) == OptimSpec("adam", beta1=0.9, beta2=0.999, eps=1e-8)
    assert OptimSpec.from_optimizer(sgd) == OptimSpec("sgd", momentum=0.9, nesterov=True)
    for opt in (adam, sgd):
        assert TU._fused_step_applies(m, opt, _zero_l2, False) is True
        assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), False) is True
        assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), True) is False  # AMP
    # other betas / eps / momentum, plain (non-Nesterov) momentum: carried in the spec
    spec = OptimSpec.from_optimizer(torch.optim.Adam(m.parameters(), lr=1e-2, betas=(0.8, 0.99), eps=1e-6))
    assert spec == OptimSpec("adam", beta1=0.8, beta2=0.99, eps=1e-6)
    assert OptimSpec.from_optimizer(torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.5)) == OptimSpec("sgd", momentum=0.5, nesterov=False)
    assert spec.state_keys == ("exp_avg", "exp_avg_sq") and OptimSpec("sgd", momentum=0.9).state_keys == ("momentum_buffer",)


@pytest.mark.parametrize("make", [
    lambda ps: torch.optim.Adam(ps, lr=1e-3, amsgrad=True),
    lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-4),
    lambda ps: torch.optim.Adam(ps, lr=1e-3, maximize=True),
    lambda ps: torch.optim.Adam(ps, lr=1e-3, capturable=True),
    lambda ps: torch.optim.Adam(ps, lr=1e-3, differentiable=True),
    lambda ps: torch.optim.AdamW(ps, lr=1e-3),
    lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9, dampening=0.1),
    lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4),
    lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9, maximize=True),
    lambda ps: torch.optim.SGD(ps, lr=0.1),  # plain SGD (momentum 0): torch route
    lambda ps: torch.optim.RMSprop(ps, lr=0.1),
], ids=["amsgrad", "adam-wd", "adam-maximize", "capturable", "differentiable", "adamw", "dampening", "sgd-wd", "sgd-maximize",
        "plain-sgd", "rmsprop"])
def test_configurations_the_fused_step_does_not_reproduce_keep_the_torch_route(one_process, make):
    m = _Tiny()
    opt = make(m.parameters())
    assert OptimSpec.from_optimizer(opt) is None
    assert TU._fused_step_applies(m, opt, _zero_l2, False) is False


def test_groups_subsets_and_placement_keep_the_torch_route(one_process, monkeypatch):
    m = _Tiny()
    for cls, kw in ((torch.optim.Adam, {"eps": 1e-8}), (torch.optim.SGD, {"momentum": 0.9, "nesterov": True})):
        two = cls([{"params": list(m._embedding.parameters())}, {"params": [p for n, p in m.named_parameters() if not n.startswith("_emb")]}],
                  lr=1e-2, **kw)
        assert TU._fused_step_applies(m, two, _zero_l2, False) is False
        subset = cls(list(m._final.parameters()), lr=1e-2, **kw)
        assert TU._fused_step_applies(m, subset, _zero_l2, False) is False
        whole = cls(m.parameters(), lr=1e-2, **kw)
        assert TU._fused_step_applies(m, whole, _zero_l2, False) is True
        m._embedding[0].weight.requires_grad_(False)
        assert TU._fused_step_applies(m, whole, _zero_l2, False) is False
        m._embedding[0].weight.requires_grad_(True)
        m._table_sharding = "row"
        assert TU._fused_step_applies(m, whole, _zero_l2, False) is False
        m._table_sharding = None
        m._place_embedding_on_cpu = True
        assert TU._fused_step_applies(m, whole, _zero_l2, False) is False
        m._place_embedding_on_cpu = False
        monkeypatch.setattr(one_process, "world_info", lambda: (0, 2))
        assert TU._fused_step_applies(m, whole, _zero_l2, False) is False
        monkeypatch.setattr(one_process, "world_info", lambda: (0, 1))
        # an opaque L2 callable with a non-zero value: torch route, as for Adagrad
        assert TU._fused_step_applies(m, whole, lambda mm: TU.get_l2_loss(mm, 1e-8, None), False) is False


def test_adagrad_answers_are_unchanged(one_process):
    m = _Tiny()
    opt = MT.build_optimizer("adagrad", m, 0.05)
    assert OptimSpec.from_optimizer(opt) is None  # (Adagrad is not a moments optimizer: it keeps its own checks)
    assert TU._fused_step_applies(m, opt, _zero_l2, False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-8), False) is True
    assert TU._fused_step_applies(m, opt, lambda mm: TU.get_l2_loss(mm, 1e-8, None), False) is False
    assert TU._fused_step_applies(m, torch.optim.Adagrad(m.parameters(), lr=0.1, lr_decay=0.1), _zero_l2, False) is False
    assert TU._fused_step_applies(m, torch.optim.Adagrad(m.parameters(), lr=0.1, initial_accumulator_value=0.1), _zero_l2, False) is False
    assert TU._fused_step_applies(m, torch.optim.Adagrad(m.parameters(), lr=0.1, weight_decay=1e-4), _zero_l2, False) is False
    assert TU._fused_step_applies(m, opt, _zero_l2, True) is False
