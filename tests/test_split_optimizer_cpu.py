"""`--optimizer adam-adagrad-tables` without a GPU: utils/optim.AdamAdagradTables.step() against torch itself — torch.optim.Adam on the
dense parameters plus torch.optim.Adagrad(lr * table_lr_scale, eps=table_eps) on the tables, bit for bit —, its checkpoint, the two
schedulers over its one param group, its OptimSpec (fields, pinned positions, refusals, the regularised-table rule), the harness's
choice of route, the three CLIs, what engine_bind_optimizer leaves in optimizer.state, and the descriptor's layout."""
import contextlib
import copy
import ctypes as C

import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.lr_schedule import ConstantWithWarmup, CosineAnnealingWarmupRestarts
from nasrec_amd.utils.optim import AdamAdagradTables
from test_optim_routing_cpu import _HostEngine, _aliases, _engine_arrays, _last_layer_mode, _model, one_process  # noqa: F401

LR, TABLE_EPS = 1e-3, 1e-2


class _Net(torch.nn.Module):
    """two tables, two Linears, and one parameter no gradient ever reaches"""

    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(50, 16), torch.nn.Embedding(50, 16)])
        self.lin = torch.nn.Linear(32, 8)
        self._final = torch.nn.Linear(8, 1)
        self.unused = torch.nn.Parameter(torch.randn(5))

    def forward(self, ids):
        x = torch.cat([self._embedding[f](ids[:, f]) for f in range(2)], 1)
        return self._final(torch.relu(self.lin(x))).view(-1)


def _pair(seed=3):
    torch.manual_seed(seed)
    a, b = _Net(), _Net()
    b.load_state_dict(a.state_dict())
    return a, b


def _split(m, scale, lr=LR):
    return AdamAdagradTables(m.parameters(), list(m._embedding.parameters()), lr=lr, table_lr_scale=scale, table_eps=TABLE_EPS)


def _torch_pair(m, scale, lr=LR):
    tables = list(m._embedding.parameters())
    dense = [p for n, p in m.named_parameters() if not n.startswith("_embedding.")]
    return torch.optim.Adam(dense, lr=lr), torch.optim.Adagrad(tables, lr=lr * scale, eps=TABLE_EPS)


def _backward(m, ids, y):
    for p in m.parameters():
        p.grad = None
    (m(ids) - y).square().mean().backward()


def _batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 30, (6, 2), generator=g), torch.randn(6, generator=g)) for _ in range(n)]  # (rows 30.. are never in a batch)


@pytest.mark.parametrize("scale", [1.0, 50.0])
def test_step_is_adam_on_the_network_and_adagrad_on_the_tables_bit_for_bit(scale):
    a, b = _pair()
    start = {n: p.detach().clone() for n, p in a.named_parameters()}
    oa = _split(a, scale)
    adam, adagrad = _torch_pair(b, scale)
    for ids, y in _batches(4):
        _backward(a, ids, y)
        _backward(b, ids, y)
        oa.step()
        adam.step()
        adagrad.step()
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        ref = adagrad if n.startswith("_embedding.") else adam
        assert torch.equal(p, pb[n]), n
        if n == "unused":  # no gradient: no state (torch.optim.Adam creates none either)
            assert p not in oa.state and pb[n] not in ref.state and torch.equal(p, start[n])
            continue
        sa, sb = oa.state[p], ref.state[pb[n]]
        assert set(sa) == set(sb) == ({"step", "sum"} if n.startswith("_embedding.") else {"step", "exp_avg", "exp_avg_sq"}), n
        for k in sa:
            assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), (n, k)
        assert float(sa["step"]) == 4.0 and sa["step"].dtype == sb["step"].dtype
    for f in range(2):  # a row outside every batch: a zero gradient leaves W and sum alone
        w = a._embedding[f].weight
        assert torch.equal(w[30:], start["_embedding.%d.weight" % f][30:]) and not torch.equal(w[:30], start["_embedding.%d.weight" % f][:30])
        assert int(oa.state[w]["sum"][30:].count_nonzero()) == 0 and int(oa.state[w]["sum"][:30].count_nonzero()) > 0


def test_the_scale_moves_the_tables_only():
    a, b = _pair()
    oa, ob = _split(a, 1.0), _split(b, 50.0)
    for ids, y in _batches(1):
        _backward(a, ids, y)
        _backward(b, ids, y)
        oa.step()
        ob.step()
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        assert torch.equal(p, pb[n]) == (not n.startswith("_embedding.")), n


def test_checkpoint_round_trip_gives_the_same_next_step():
    a, b = _pair()
    oa = _split(a, 50.0)
    data = _batches(4)
    for ids, y in data[:3]:
        _backward(a, ids, y)
        oa.step()
    b.load_state_dict(a.state_dict())
    ob = _split(b, 1.0, lr=0.5)  # (the checkpoint's group carries lr, table_lr_scale and table_eps)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))  # (as a checkpoint file would hold it: torch's load keeps the tensors it is given)
    g = ob.param_groups[0]
    assert g["lr"] == LR and g["table_lr_scale"] == 50.0 and g["table_eps"] == TABLE_EPS
    ids, y = data[3]
    for m, o in ((a, oa), (b, ob)):
        _backward(m, ids, y)
        o.step()
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        assert torch.equal(p, pb[n]), n
        if p in oa.state:
            for k, v in oa.state[p].items():
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(ob.state[pb[n]][k])), (n, k)
    assert a.unused not in oa.state and b.unused not in ob.state


def test_constructor_checks_and_sparse_gradients():
    m = _Net()
    for kw in (dict(table_eps=0.0), dict(table_eps=-1e-2), dict(table_lr_scale=0.0), dict(table_lr_scale=-1.0)):
        with pytest.raises(ValueError):
            AdamAdagradTables(m.parameters(), list(m._embedding.parameters()), **kw)
    with pytest.raises(ValueError):
        AdamAdagradTables(m.lin.parameters(), list(m._embedding.parameters()))  # a table that is not one of params
    with pytest.raises(ValueError):
        AdamAdagradTables([{"params": list(m._embedding.parameters())}, {"params": list(m.lin.parameters())}], list(m._embedding.parameters()))
    w = torch.nn.Parameter(torch.randn(6, 16))
    opt = AdamAdagradTables([w], [w])
    w.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.randn(1, 16), (6, 16))
    with pytest.raises(RuntimeError, match="dense gradients"):
        opt.step()
    assert not hasattr(opt, "touch")  # (the harness calls touch() where it exists: this optimizer needs no ids)


def test_schedulers_move_lr_and_leave_the_table_keys_alone():
    m = _Net()
    opt = _split(m, 160.0)
    sched = ConstantWithWarmup(opt, num_warmup_steps=4)
    seen = [opt.param_groups[0]["lr"]]
    for _ in range(5):
        sched.step()
        seen.append(opt.param_groups[0]["lr"])
    assert seen[0] == LR / 4 and seen[-1] == LR and len(set(seen)) == 4
    g = opt.param_groups[0]
    assert len(opt.param_groups) == 1 and g["table_lr_scale"] == 160.0 and g["table_eps"] == TABLE_EPS
    opt = _split(m, 160.0)
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=10, warmup_steps=2, max_lr=LR, min_lr=1e-8)
    seen = [opt.param_groups[0]["lr"]]
    for _ in range(6):
        sched.step()
        seen.append(opt.param_groups[0]["lr"])
    assert seen[0] == 1e-8 and max(seen) == LR and len(set(seen)) > 4
    g = opt.param_groups[0]
    assert g["table_lr_scale"] == 160.0 and g["table_eps"] == TABLE_EPS and g["lr"] == sched.get_lr()


# ------------------------------------------------------------------------------------------------------------------------- spec
def test_spec_fields_and_pinned_positions():
    m = _model()
    opt = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, 160.0, 1e-6)
    assert type(opt) is AdamAdagradTables
    g = opt.param_groups[0]
    assert g["lr"] == 1e-3 and g["eps"] == 1e-8 and g["table_lr_scale"] == 160.0 and g["table_eps"] == 1e-6
    d = MT.build_optimizer("adam-adagrad-tables", m, 1e-3).param_groups[0]
    assert d["table_lr_scale"] == 1.0 and d["table_eps"] == 1e-2
    spec = OptimSpec.from_optimizer(opt)
    assert spec == OptimSpec("adam", beta1=0.9, beta2=0.999, eps=1e-8, table_kind="adagrad", table_eps=1e-6, table_lr_scale=160.0)
    assert spec.moments and spec.rows_only and not spec.sparse_rows and spec.state_keys == ("exp_avg", "exp_avg_sq")
    # the positional prefix up to alpha, the new fields behind it, dwd and ema last
    assert OptimSpec._fields[:10] == ("kind", "beta1", "beta2", "eps", "momentum", "nesterov", "wd", "no_reg", "sparse_rows", "alpha")
    assert OptimSpec._fields[10:] == ("table_kind", "table_eps", "table_lr_scale", "dwd", "ema") and OptimSpec._fields[-1] == "ema"
    assert OptimSpec("adam") == OptimSpec("adam", 0.9, 0.999, 1e-8, 0.0, False, 0.0, None, False, 0.99)
    assert OptimSpec("adam").table_kind == "" and OptimSpec("adam").table_eps == 1e-2 and OptimSpec("adam").table_lr_scale == 1.0
    assert OptimSpec.from_optimizer(torch.optim.Adam(m.parameters(), lr=1e-3)).table_kind == ""
    # rows_only: Adagrad, row-sparse Adam, RMSprop and the split; not dense Adam / SGD
    assert [OptimSpec(k).rows_only for k in ("adagrad", "rmsprop", "adam", "sgd")] == [True, True, False, False]
    assert OptimSpec("adam", sparse_rows=True).rows_only
    # `of` carries the fields through
    full = OptimSpec.of(optim=spec, weight_decay=1e-3, no_reg_param_name="_embedding", ema=0.99)
    assert (full.table_kind, full.table_eps, full.table_lr_scale, full.wd, full.ema) == ("adagrad", 1e-6, 160.0, 1e-3, 0.99)
    assert OptimSpec.of(optim=spec) != OptimSpec.of(optim=spec._replace(table_lr_scale=1.0))  # (plan-cache keys hold the spec)


def test_spec_refusals():
    m = _model()
    tables = list(m._embedding.parameters())
    assert OptimSpec.from_optimizer(AdamAdagradTables(m.parameters(), tables)) is not None
    opt = AdamAdagradTables(m.parameters(), tables)
    opt.param_groups[0]["amsgrad"] = True
    assert OptimSpec.from_optimizer(opt) is None
    for key, val in (("table_eps", torch.tensor(1e-2)), ("table_lr_scale", torch.tensor(50.0)), ("betas", (torch.tensor(0.9), 0.999))):
        opt = AdamAdagradTables(m.parameters(), tables)
        opt.param_groups[0][key] = val
        assert OptimSpec.from_optimizer(opt) is None, key
    opt = AdamAdagradTables(m.parameters(), tables)
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})
    assert OptimSpec.from_optimizer(opt) is None and OptimSpec.for_step(opt) is None
    for kw in ("weight_decay", "maximize"):
        opt = AdamAdagradTables(m.parameters(), tables)
        opt.param_groups[0][kw] = 1
        assert OptimSpec.from_optimizer(opt) is None, kw


def test_for_step_and_the_regularised_table_rule():
    m = _model()
    opt = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, 50.0)
    spec = OptimSpec.from_optimizer(opt)
    assert OptimSpec.for_step(opt) == spec
    assert OptimSpec.for_step(opt, 1e-3, None) is None and OptimSpec.for_step(opt, 1e-3, "lin") is None
    assert OptimSpec.for_step(opt, 1e-3, "_embedding") == spec._replace(wd=1e-3, no_reg="_embedding")


# ---------------------------------------------------------------------------------------------------------------------- routing
def test_routing(one_process):  # noqa: F811
    m = _model()
    m.engine_train_step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("not called here"))
    opt = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, 50.0)
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-3, "_embedding"), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-3), False) is False  # the tables are regularised
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), True) is False    # AMP
    spec = TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False)
    assert spec.table_kind == "adagrad" and spec.table_lr_scale == 50.0
    # the weight average and the decoupled decay ride in the fused step, as with Adagrad
    from nasrec_amd.utils.optim import DecoupledWeightDecay, WeightEMA
    assert TU._ema_route(m, spec, TU.L2Loss(0.0)) is None
    assert TU._ema_route(m, OptimSpec("adam"), TU.L2Loss(0.0)) is not None
    decay = DecoupledWeightDecay(m, 0.1)
    assert TU._decay_route(m, spec, TU.L2Loss(0.0), decay) is None
    assert TU._decay_route(m, spec, TU.L2Loss(0.0), decay, ema=WeightEMA(m, 0.99)) is not None  # (decay reaches the tables beside an EMA)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, WeightEMA(m, 0.99)).ema == 0.99
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, None, decay).dwd == 0.1
    # row-sharded tables and tables on the host keep the torch route (the optimizer itself runs there: it needs no ids)
    m.__dict__["_table_sharding"] = "row"
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False
    m.__dict__.update(_table_sharding=None, _place_embedding_on_cpu=True)
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False
    m.__dict__["_place_embedding_on_cpu"] = False
    # a parameter that does not train: torch route
    m.lin.bias.requires_grad_(False)
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False


def test_the_last_layer_step_keeps_the_torch_route(one_process):  # noqa: F811
    m = _model()
    _last_layer_mode(m)
    assert TU._last_layer_step_applies(m, MT.build_optimizer("adam", m, 1e-3), TU.L2Loss(0.0), False) is True
    assert TU._last_layer_step_applies(m, MT.build_optimizer("adam-adagrad-tables", m, 1e-3), TU.L2Loss(0.0), False) is False


def test_the_run_says_which_route_it_took(capsys):
    m = _model()
    opt = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, 160.0)
    TU._announce_split_route(opt, TU.L2Loss(0.0), True)
    TU._announce_split_route(opt, TU.L2Loss(0.0), True)  # once per run
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "fused step" in out and "160.0" in out
    opt = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, 160.0)
    TU._announce_split_route(opt, TU.L2Loss(1e-3), False)
    out = capsys.readouterr().out
    assert "torch route" in out and "weight decay reaches the embedding tables" in out
    TU._announce_split_route(MT.build_optimizer("adam", m, 1e-3), TU.L2Loss(0.0), True)
    assert capsys.readouterr().out == ""


def test_the_three_clis_take_the_flags():
    from nasrec_amd import eval_subnet_from_scratch, train_supernet
    for mod in (MT, train_supernet, eval_subnet_from_scratch):
        parser = mod.build_parser()
        opts = [a for a in parser._actions if "--optimizer" in a.option_strings]
        assert len(opts) == 1 and "adam-adagrad-tables" in opts[0].choices, mod.__name__
        by_flag = {s: a for a in parser._actions for s in a.option_strings}
        assert by_flag["--table-lr-scale"].default == 1.0 and by_flag["--table-lr-scale"].type is float, mod.__name__
        assert by_flag["--table-eps"].default == 1e-2 and by_flag["--table-eps"].type is float, mod.__name__
        assert by_flag["--table-lr-scale"].dest == "table_lr_scale" and by_flag["--table-eps"].dest == "table_eps"


# ------------------------------------------------------------------------------------------------------------------ bound state
def test_bound_state_shares_adams_moments_and_the_tables_sum(monkeypatch):
    """engine_bind_optimizer / engine_sync_optimizer_steps over host arrays: a dense parameter aliases Adam's moments, a table aliases
    table_state as `sum`; the engine allocates no table moments; a table the engine never stepped gets no state; an existing `sum` (a
    resumed checkpoint) is copied in"""
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    m = _model()
    opt = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, 50.0)
    w0 = m._embedding[0].weight
    opt.state[w0]["step"] = torch.tensor(3.0)
    opt.state[w0]["sum"] = torch.full_like(w0, 0.25)
    eng = m.__dict__["_engine"] = _HostEngine(m)
    m.engine_bind_optimizer(opt)
    assert all(tabs == [] for _, tabs in eng.moments.values()) and set(eng.moments) == {"exp_avg", "exp_avg_sq"}
    assert eng.table_state is not None and torch.equal(eng.table_state[0], torch.full_like(w0, 0.25))
    assert int(eng.table_state[1].count_nonzero()) == 0
    k0 = eng.param_index["_embedding.0.weight"]
    assert float(eng.opt_steps[k0]) == 3.0
    with pytest.raises(L.EngineError, match="table_state"):
        eng.moments_view("exp_avg", "_embedding.0.weight")
    # two fused steps that reached the dense parameters and table 0 only
    eng.opt_steps.add_(2.0)
    eng.opt_steps[eng.param_index["_embedding.1.weight"]] = 0.0
    m.__dict__["_engine_steps"] = 2
    m.engine_sync_optimizer_steps(opt)
    arrays = _engine_arrays(eng)
    got = {}
    for n, p in m.named_parameters():
        st = opt.state.get(p)
        if st:
            got[n] = sorted((k, _aliases(v, arrays) if k != "step" else False, float(v) if k == "step" else None) for k, v in st.items())
    dense = [("exp_avg", True, None), ("exp_avg_sq", True, None), ("step", False, 2.0)]
    assert got == {"_embedding.0.weight": [("step", False, 5.0), ("sum", True, None)],
                   "lin.weight": dense, "lin.bias": dense, "_final.weight": dense, "_final.bias": dense}
    assert opt.state[w0]["sum"].data_ptr() == eng.table_state[0].data_ptr()
    sd = opt.state_dict()  # what the torch route would have written: Adagrad's keys on the table, Adam's on the rest
    assert sorted(sd["state"][0]) == ["step", "sum"] and 1 not in sd["state"] and sorted(sd["state"][2]) == ["exp_avg", "exp_avg_sq", "step"]


# ------------------------------------------------------------------------------------------------------------------- descriptor
def test_descriptor_carries_the_new_fields_in_its_padding_words():
    """table_algo sits where _pad3 was and is the structure's last field; table_eps and table_lr_scale sit where _pad and _pad2 were:
    the structure keeps its size (test_row_sparse_adam_cpu.py pins its end 8 bytes behind sparse_rows), a caller of the earlier layout
    wrote zeros there = NASREC_TABLE_ALGO_SAME, and the binding's load-time check compares the size with the library's"""
    names = [f[0] for f in L.OptMomentsDesc._fields_]
    assert names[-2:] == ["sparse_rows", "table_algo"] and not any(n.startswith("_pad") for n in names)
    D = L.OptMomentsDesc
    assert D.table_algo.offset == D.sparse_rows.offset + 4 and C.sizeof(D) == D.table_algo.offset + 4   # where _pad3 was
    assert D.table_eps.offset == D.wd.offset + 4 and D.beta1.offset == D.table_eps.offset + 4            # where _pad was
    assert D.table_lr_scale.offset == D.rank_B.offset + 4 and D.rank_stride.offset == D.table_lr_scale.offset + 4  # where _pad2 was
    assert all(dict(D._fields_)[k] is C.c_float for k in ("table_eps", "table_lr_scale")) and dict(D._fields_)["table_algo"] is C.c_int32
    assert (L.TABLE_ALGO_SAME, L.TABLE_ALGO_ADAGRAD) == (0, 1)
    lib = L.load()  # (load compares every structure's size with the library's)
    assert lib.nasrec_abi_version() == 17
    sizes = (C.c_int32 * 45)()
    n = lib.nasrec_desc_sizes(sizes, 45)
    assert n > L.OP_OPT_MOMENTS and sizes[L.OP_OPT_MOMENTS] == C.sizeof(D)


# ------------------------------------------------------------------------------------------------------------ row-sharded checkpoint
def test_a_row_sharded_checkpoint_gathers_the_optimizers_own_sum():
    """row-sharded tables train with this optimizer on the torch route, so a table's `sum` is the optimizer's own tensor: the checkpoint
    gathers that shard, not the engine's Adagrad accumulator (which torch.optim.Adagrad's state aliases and which stays the source there)"""
    from nasrec_amd.utils.io_utils import optimizer_state_for_checkpoint
    calls = []

    class _Sharded:
        world = 2

        def whole_table(self, f, which="tables", shard=None):
            calls.append((f, which, shard))
            return torch.cat([shard, shard]) if shard is not None else torch.zeros(1)
    m = _model()
    opt = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, 50.0)
    w0 = m._embedding[0].weight
    w0.grad = torch.randn_like(w0)
    opt.step()
    m.__dict__.update(_table_sharding="row", _sharded=_Sharded())
    sd = optimizer_state_for_checkpoint(m, opt)
    assert [(f, which) for f, which, _ in calls] == [(0, "state")] and calls[0][2] is opt.state[w0]["sum"]
    assert torch.equal(sd["state"][0]["sum"], torch.cat([opt.state[w0]["sum"]] * 2)) and 1 not in sd["state"]
    del calls[:]
    ada = torch.optim.Adagrad(m.parameters(), lr=0.05)
    optimizer_state_for_checkpoint(m, ada)
    assert calls and all(shard is None for _, _, shard in calls)
