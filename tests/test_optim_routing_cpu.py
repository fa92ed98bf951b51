"""Which route the training harness takes for an optimizer (train_utils: the fused step, the fused last-layer step or the torch route), and
what SuperNet.engine_bind_optimizer leaves in optimizer.state, for a table of optimizers x weight decay x model mode — without a GPU (the
engine's state arrays live on the host here)."""
import contextlib
import types

import pytest
import torch

from nasrec_amd.engine import SupernetEngine
from nasrec_amd.supernet.supernet import SuperNet
from nasrec_amd.utils import train_utils as TU

OPTIMIZERS = {
    "adagrad": lambda ps: torch.optim.Adagrad(ps, lr=0.05, eps=1e-2),
    "adagrad-lr_decay": lambda ps: torch.optim.Adagrad(ps, lr=0.05, lr_decay=0.1),
    "adagrad-differentiable": lambda ps: torch.optim.Adagrad(ps, lr=0.05, differentiable=True),
    "adam": lambda ps: torch.optim.Adam(ps, lr=1e-3),
    "adam-amsgrad": lambda ps: torch.optim.Adam(ps, lr=1e-3, amsgrad=True),
    "sgd": lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9, nesterov=True),
    "sgd-plain": lambda ps: torch.optim.SGD(ps, lr=0.05),
}

# (optimizer, wd, mode) -> route, as train_and_test_one_epoch(last_layer_step=True) chooses it
ROUTES = {
    ("adagrad", 0.0, "full"): "fused", ("adagrad", 1e-4, "full"): "fused",
    ("adagrad", 0.0, "last"): "last", ("adagrad", 1e-4, "last"): "last",
    ("adagrad-lr_decay", 0.0, "full"): "torch", ("adagrad-lr_decay", 1e-4, "full"): "torch",
    ("adagrad-lr_decay", 0.0, "last"): "torch", ("adagrad-lr_decay", 1e-4, "last"): "torch",
    ("adagrad-differentiable", 0.0, "full"): "fused", ("adagrad-differentiable", 1e-4, "full"): "fused",
    ("adagrad-differentiable", 0.0, "last"): "torch", ("adagrad-differentiable", 1e-4, "last"): "torch",
    ("adam", 0.0, "full"): "fused", ("adam", 1e-4, "full"): "fused",
    ("adam", 0.0, "last"): "last", ("adam", 1e-4, "last"): "last",
    ("adam-amsgrad", 0.0, "full"): "torch", ("adam-amsgrad", 1e-4, "full"): "torch",
    ("adam-amsgrad", 0.0, "last"): "torch", ("adam-amsgrad", 1e-4, "last"): "torch",
    ("sgd", 0.0, "full"): "fused", ("sgd", 1e-4, "full"): "fused",
    ("sgd", 0.0, "last"): "last", ("sgd", 1e-4, "last"): "last",
    ("sgd-plain", 0.0, "full"): "torch", ("sgd-plain", 1e-4, "full"): "torch",
    ("sgd-plain", 0.0, "last"): "torch", ("sgd-plain", 1e-4, "last"): "torch",
}


def _model():
    m = SuperNet.__new__(SuperNet)
    torch.nn.Module.__init__(m)
    m._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
    m.lin = torch.nn.Linear(4, 3)
    m._final = torch.nn.Linear(3, 1)
    m.__dict__.update(_table_sharding=None, _place_embedding_on_cpu=False, _engine=None)
    return m


def _last_layer_mode(m):
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("_final."))


@pytest.fixture
def one_process(monkeypatch):
    from nasrec_amd.utils import dist as D
    monkeypatch.setattr(D, "world_info", lambda: (0, 1))


@pytest.mark.parametrize("name,wd,mode", sorted(ROUTES))
def test_route(one_process, name, wd, mode):
    m = _model()
    if mode == "last":
        _last_layer_mode(m)
    opt = OPTIMIZERS[name](m.parameters())
    l2 = TU.L2Loss(wd)
    if TU._fused_step_applies(m, opt, l2, False):
        route = "fused"
    elif TU._last_layer_step_applies(m, opt, l2, False):
        route = "last"
    else:
        route = "torch"
    assert route == ROUTES[(name, wd, mode)]


class _HostEngine(SupernetEngine):
    """the engine's optimizer-state bookkeeping (SupernetEngine's own methods) over host arrays"""

    def __init__(self, m):
        params = dict(m.named_parameters())
        self.device, self.stream = torch.device("cpu"), types.SimpleNamespace(synchronize=lambda: None)
        self.dense_names = [n for n in params if not n.startswith("_embedding.")]
        self.offsets, off = {}, 0
        for n in self.dense_names:
            self.offsets[n] = off
            off += params[n].numel()
        self.flat_numel = off
        self.flat_s = torch.zeros(off)
        self.params = {n: p.data for n, p in params.items()}
        self.state = {n: self.flat_s[self.offsets[n]:self.offsets[n] + p.numel()].view(p.shape) for n, p in params.items()
                      if n in self.offsets}
        self.tables = [e.weight.data for e in m._embedding]
        self.Fs = len(self.tables)
        self.table_state = None


def _engine_arrays(eng):
    arrays = [eng.flat_s] + list(eng.table_state or [])
    for flat, tabs in getattr(eng, "moments", {}).values():
        arrays += [flat] + list(tabs)
    for pair in getattr(eng, "ll_moments", {}).values():
        arrays += list(pair)
    return arrays


def _aliases(t, arrays):
    return any(a.data_ptr() <= t.data_ptr() < a.data_ptr() + a.numel() * a.element_size() for a in arrays)


# (optimizer, mode) -> {parameter: sorted (state key, aliases engine storage, value of "step" or None)} after one bind of a fresh
# optimizer and a sync after two fused steps
STATE = {
    ("adagrad", "full"): {n: [("step", False, 2.0), ("sum", True, None)] for n in
                          ("_embedding.0.weight", "_embedding.1.weight", "lin.weight", "lin.bias", "_final.weight", "_final.bias")},
    # (torch.optim.Adagrad creates its state in the constructor: the frozen parameters keep theirs, untouched)
    ("adagrad", "last"): dict({n: [("step", False, 0.0), ("sum", False, None)] for n in
                               ("_embedding.0.weight", "_embedding.1.weight", "lin.weight", "lin.bias")},
                              **{n: [("step", False, 2.0), ("sum", True, None)] for n in ("_final.weight", "_final.bias")}),
    ("adam", "full"): {n: [("exp_avg", True, None), ("exp_avg_sq", True, None), ("step", False, 2.0)] for n in
                       ("_embedding.0.weight", "_embedding.1.weight", "lin.weight", "lin.bias", "_final.weight", "_final.bias")},
    ("adam", "last"): {n: [("exp_avg", True, None), ("exp_avg_sq", True, None), ("step", False, 2.0)] for n in ("_final.weight", "_final.bias")},
    ("sgd", "full"): {n: [("momentum_buffer", True, None)] for n in
                      ("_embedding.0.weight", "_embedding.1.weight", "lin.weight", "lin.bias", "_final.weight", "_final.bias")},
    ("sgd", "last"): {n: [("momentum_buffer", True, None)] for n in ("_final.weight", "_final.bias")},
}


@pytest.mark.parametrize("name,mode", sorted(STATE))
def test_bound_state(monkeypatch, name, mode):
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    m = _model()
    last = mode == "last"
    if last:
        _last_layer_mode(m)
    opt = OPTIMIZERS[name](m.parameters())
    eng = m.__dict__["_engine"] = _HostEngine(m)
    m.engine_bind_optimizer(opt, last_layer=last)
    # two fused steps: the engine's counters move (Adam / SGD), the harness's step counts move (Adagrad)
    m.__dict__["_last_layer_steps" if last else "_engine_steps"] = 2
    if name != "adagrad":
        steps = eng.ll_steps if last else eng.opt_steps
        steps.fill_(2.0)
    m.engine_sync_optimizer_steps(opt)
    arrays = _engine_arrays(eng)
    got = {}
    for n, p in m.named_parameters():
        st = opt.state.get(p)
        if st:
            got[n] = sorted((k, _aliases(v, arrays) if k != "step" else False, float(v) if k == "step" else None) for k, v in st.items())
    assert got == STATE[(name, mode)]
