"""`--optimizer adam-adagrad-tables --table-rowwise` without a GPU: utils/optim.AdamAdagradTables(table_rowwise=True).step() against an
fp64 NumPy restatement of row-wise Adagrad (sum += mean(g^2) per row; W -= tlr * g / (sqrt(sum) + eps)) with the dense half bit-identical
to torch.optim.Adam; the [rows] accumulator, its checkpoint and the refusal of the other rule's state; the OptimSpec (table_kind
"rowwise_adagrad", no new field), the binding's constant, the harness's choice of route, the three CLIs, what engine_bind_optimizer
leaves in optimizer.state and in the engine (table_row_state, never table_state), the replicas' rule encoding, and the row-sharded
checkpoint's gather of a 1-D shard.  Helpers from test_split_optimizer_cpu.py."""
import contextlib
import copy
import types

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import AdamAdagradTables
from test_optim_routing_cpu import _HostEngine, _aliases, _engine_arrays, _last_layer_mode, _model, one_process  # noqa: F401
from test_split_optimizer_cpu import LR, TABLE_EPS, _Net, _backward, _batches, _pair

NAME = "adam-adagrad-tables"


def _rowwise(m, scale, lr=LR, rowwise=True):
    return AdamAdagradTables(m.parameters(), list(m._embedding.parameters()), lr=lr, table_lr_scale=scale, table_eps=TABLE_EPS,
                             table_rowwise=rowwise)


def _close(a, b, what):
    """the kernel tests' bar: one step from fp32 inputs, in fp32 against fp64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.allclose(a, b, rtol=2e-6, atol=2e-7), (what, float(np.abs(a - b).max()))


@pytest.mark.parametrize("scale", [1.0, 50.0])
def test_step_against_fp64_with_adam_on_the_network_bit_for_bit(scale):
    """3 steps; every step's table update is restated in fp64 from the fp32 state it started from; the twin model takes torch.optim.Adam
    on the dense parameters and the first model's tables, so both see the same gradients"""
    a, b = _pair()
    start = {n: p.detach().clone() for n, p in a.named_parameters()}
    oa = _rowwise(a, scale)
    adam = torch.optim.Adam([p for n, p in b.named_parameters() if not n.startswith("_embedding.")], lr=LR)
    tlr = LR * scale
    for step, (ids, y) in enumerate(_batches(3)):
        _backward(a, ids, y)
        _backward(b, ids, y)
        want = []
        for f in range(2):
            w = a._embedding[f].weight
            g = w.grad.double().numpy()
            s = oa.state[w]["sum"].double().numpy() if w in oa.state and "sum" in oa.state[w] else np.zeros(50)
            s = s + (g * g).mean(axis=1)
            want.append((s, w.detach().double().numpy() - tlr * g / (np.sqrt(s) + TABLE_EPS)[:, None]))
        oa.step()
        adam.step()
        for f in range(2):
            w = a._embedding[f].weight
            assert oa.state[w]["sum"].shape == (50,) and oa.state[w]["sum"].dtype == torch.float32
            assert float(oa.state[w]["step"]) == step + 1.0
            _close(oa.state[w]["sum"], want[f][0], ("sum", f, step))
            _close(w.detach(), want[f][1], ("table", f, step))
            with torch.no_grad():
                b._embedding[f].weight.copy_(w)
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        if n.startswith("_embedding."):
            continue
        assert torch.equal(p, pb[n]), n
        if n == "unused":
            assert p not in oa.state and torch.equal(p, start[n])
            continue
        sa, sb = oa.state[p], adam.state[pb[n]]
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}, n
        for k in sa:
            assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), (n, k)
    for f in range(2):  # rows 30.. are in no batch: an all-zero gradient keeps the bits of W and sum
        w = a._embedding[f].weight
        k = "_embedding.%d.weight" % f
        assert torch.equal(w[30:], start[k][30:]) and not torch.equal(w[:30], start[k][:30])
        assert int(oa.state[w]["sum"][30:].count_nonzero()) == 0 and int(oa.state[w]["sum"][:30].count_nonzero()) > 0


def test_a_zero_gradient_row_keeps_its_bits_with_a_non_zero_accumulator():
    w = torch.nn.Parameter(torch.randn(6, 16))
    opt = AdamAdagradTables([w], [w], table_lr_scale=50.0, table_rowwise=True)
    w.grad = torch.randn(6, 16)
    opt.step()
    w0, s0 = w.detach().clone(), opt.state[w]["sum"].clone()
    assert s0.shape == (6,) and bool((s0 > 0).all())
    w.grad = torch.randn(6, 16)
    w.grad[2] = 0.0
    w.grad[5] = 0.0
    opt.step()
    moved = torch.tensor([True, True, False, True, True, False])
    assert torch.equal(w.detach()[~moved], w0[~moved]) and torch.equal(opt.state[w]["sum"][~moved], s0[~moved])
    assert not (w.detach()[moved] == w0[moved]).all(1).any() and bool((opt.state[w]["sum"][moved] > s0[moved]).all())


def test_the_rule_differs_from_the_elementwise_one_on_the_tables_only():
    a, b = _pair()
    oa, ob = _rowwise(a, 50.0), _rowwise(b, 50.0, rowwise=False)
    for ids, y in _batches(1):
        _backward(a, ids, y)
        _backward(b, ids, y)
        oa.step()
        ob.step()
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        assert torch.equal(p, pb[n]) == (not n.startswith("_embedding.")), n
    assert ob.state[b._embedding[0].weight]["sum"].shape == (50, 16) and oa.state[a._embedding[0].weight]["sum"].shape == (50,)


def test_checkpoint_round_trip_gives_the_same_next_step():
    a, b = _pair()
    oa = _rowwise(a, 50.0)
    data = _batches(4)
    for ids, y in data[:3]:
        _backward(a, ids, y)
        oa.step()
    b.load_state_dict(a.state_dict())
    ob = _rowwise(b, 1.0, lr=0.5)  # (the checkpoint's group carries lr, table_lr_scale, table_eps and table_rowwise)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    g = ob.param_groups[0]
    assert g["lr"] == LR and g["table_lr_scale"] == 50.0 and g["table_eps"] == TABLE_EPS and g["table_rowwise"] is True
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
    assert ob.state[b._embedding[1].weight]["sum"].shape == (50,)


def test_the_other_rules_state_is_refused():
    """an element-wise checkpoint into a row-wise optimizer and the reverse: ValueError, nothing loaded, nothing broadcast"""
    a, b = _pair()
    rowwise, elementwise = _rowwise(a, 50.0), _rowwise(b, 50.0, rowwise=False)
    ids, y = _batches(1)[0]
    for m, o in ((a, rowwise), (b, elementwise)):
        _backward(m, ids, y)
        o.step()
    sd_row, sd_elem = copy.deepcopy(rowwise.state_dict()), copy.deepcopy(elementwise.state_dict())
    for opt, other in ((rowwise, sd_elem), (elementwise, sd_row)):
        before = copy.deepcopy(opt.state_dict())
        with pytest.raises(ValueError, match="table_rowwise"):
            opt.load_state_dict(copy.deepcopy(other))
        after = opt.state_dict()
        assert after["param_groups"] == before["param_groups"]
        assert all(torch.equal(torch.as_tensor(v), torch.as_tensor(after["state"][i][k])) for i, st in before["state"].items() for k, v in st.items())
    # a checkpoint from before the flag (no table_rowwise in its group) is an element-wise one
    old = copy.deepcopy(sd_elem)
    del old["param_groups"][0]["table_rowwise"]
    with pytest.raises(ValueError, match="table_rowwise"):
        rowwise.load_state_dict(copy.deepcopy(old))
    elementwise.load_state_dict(old)
    assert elementwise.param_groups[0].get("table_rowwise", False) is False
    # the group says row-wise but a sum has the table's shape (or the reverse): the shape check names both shapes
    forged = copy.deepcopy(sd_elem)
    forged["param_groups"][0]["table_rowwise"] = True
    with pytest.raises(ValueError, match=r"\(50, 16\)"):
        rowwise.load_state_dict(forged)
    # and a state put there by hand is caught by step() before anything broadcasts: [16] against a [16, 16] table would
    w = torch.nn.Parameter(torch.randn(16, 16))
    opt = AdamAdagradTables([w], [w], table_rowwise=False)
    opt.state[w]["step"], opt.state[w]["sum"] = torch.tensor(1.0), torch.ones(16)
    w.grad = torch.randn(16, 16)
    w0 = w.detach().clone()
    with pytest.raises(ValueError, match=r"\(16,\)"):
        opt.step()
    assert torch.equal(w.detach(), w0)
    opt = AdamAdagradTables([w], [w], table_rowwise=True)
    opt.state[w]["step"], opt.state[w]["sum"] = torch.tensor(1.0), torch.ones(16, 16)
    with pytest.raises(ValueError, match=r"\(16, 16\)"):
        opt.step()
    assert torch.equal(w.detach(), w0)


def test_a_table_that_is_not_2d_is_refused():
    v = torch.nn.Parameter(torch.randn(6))
    with pytest.raises(ValueError, match=r"\(6,\)"):
        AdamAdagradTables([v], [v], table_rowwise=True)
    AdamAdagradTables([v], [v])  # (the element-wise rule takes any shape)
    t3 = torch.nn.Parameter(torch.randn(2, 3, 4))
    with pytest.raises(ValueError, match=r"\(2, 3, 4\)"):
        AdamAdagradTables([t3], [t3], table_rowwise=True)


# ------------------------------------------------------------------------------------------------------------------------- spec
def test_spec_and_constants():
    m = _model()
    opt = MT.build_optimizer(NAME, m, 1e-3, 160.0, 1e-6, table_rowwise=True)
    assert type(opt) is AdamAdagradTables and opt.param_groups[0]["table_rowwise"] is True
    assert MT.build_optimizer(NAME, m, 1e-3).param_groups[0]["table_rowwise"] is False
    spec = OptimSpec.from_optimizer(opt)
    assert spec == OptimSpec("adam", beta1=0.9, beta2=0.999, eps=1e-8, table_kind="rowwise_adagrad", table_eps=1e-6, table_lr_scale=160.0)
    elementwise = OptimSpec.from_optimizer(MT.build_optimizer(NAME, m, 1e-3, 160.0, 1e-6))
    assert elementwise.table_kind == "adagrad" and spec != elementwise and spec == elementwise._replace(table_kind="rowwise_adagrad")
    assert OptimSpec.of(optim=spec) != OptimSpec.of(optim=elementwise)  # (plan-cache keys hold the spec: two plans)
    assert spec.moments and spec.rows_only and not spec.sparse_rows and spec.state_keys == ("exp_avg", "exp_avg_sq")
    assert OptimSpec._fields == ("kind", "beta1", "beta2", "eps", "momentum", "nesterov", "wd", "no_reg", "sparse_rows", "alpha",
                                 "table_kind", "table_eps", "table_lr_scale", "dwd", "ema")
    full = OptimSpec.of(optim=spec, weight_decay=1e-3, no_reg_param_name="_embedding", ema=0.99)
    assert (full.table_kind, full.table_eps, full.table_lr_scale, full.wd, full.ema) == ("rowwise_adagrad", 1e-6, 160.0, 1e-3, 0.99)
    # the regularised-table rule of for_step
    assert OptimSpec.for_step(opt) == spec
    assert OptimSpec.for_step(opt, 1e-3, None) is None and OptimSpec.for_step(opt, 1e-3, "lin") is None
    assert OptimSpec.for_step(opt, 1e-3, "_embedding") == spec._replace(wd=1e-3, no_reg="_embedding")
    # the binding
    assert (L.TABLE_ALGO_SAME, L.TABLE_ALGO_ADAGRAD, L.TABLE_ALGO_ROWWISE_ADAGRAD) == (0, 1, 3)
    assert L.load().nasrec_abi_version() == 17
    names = [f[0] for f in L.OptMomentsDesc._fields_]
    assert names[-2:] == ["sparse_rows", "table_algo"]
    # the descriptor's scalars: the row-wise rule is Adam's algo with its own table_algo, and nothing else is a split
    d = L.OptMomentsDesc()
    from nasrec_amd.engine import SupernetEngine
    SupernetEngine._optim_scalars(d, spec)
    assert d.algo == L.OPTIM_ADAM
    with pytest.raises(L.EngineError, match="table_kind"):
        SupernetEngine._optim_scalars(d, spec._replace(table_kind="rowwise"))
    with pytest.raises(L.EngineError, match="table_kind"):
        SupernetEngine._optim_scalars(d, spec._replace(kind="sgd"))


# ---------------------------------------------------------------------------------------------------------------------- routing
def test_routing(one_process):  # noqa: F811
    m = _model()
    m.engine_train_step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("not called here"))
    opt = MT.build_optimizer(NAME, m, 1e-3, 50.0, table_rowwise=True)
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-3, "_embedding"), False) is True
    assert TU._fused_step_applies(m, opt, TU.L2Loss(1e-3), False) is False  # the tables are regularised
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), True) is False    # AMP
    spec = TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False)
    assert spec.table_kind == "rowwise_adagrad" and spec.table_lr_scale == 50.0
    # the weight average and the decoupled decay ride in the fused step, as with the element-wise rule
    from nasrec_amd.utils.optim import DecoupledWeightDecay, WeightEMA
    assert TU._ema_route(m, spec, TU.L2Loss(0.0)) is None
    decay = DecoupledWeightDecay(m, 0.1)
    assert TU._decay_route(m, spec, TU.L2Loss(0.0), decay) is None
    assert TU._decay_route(m, spec, TU.L2Loss(0.0), decay, ema=WeightEMA(m, 0.99)) is not None
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, WeightEMA(m, 0.99)).ema == 0.99
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, None, decay).dwd == 0.1
    # row-sharded tables and tables on the host keep the torch route
    m.__dict__["_table_sharding"] = "row"
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False
    m.__dict__.update(_table_sharding=None, _place_embedding_on_cpu=True)
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is False
    m.__dict__["_place_embedding_on_cpu"] = False
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False) is True


def test_the_last_layer_step_keeps_the_torch_route(one_process):  # noqa: F811
    m = _model()
    _last_layer_mode(m)
    assert TU._last_layer_step_applies(m, MT.build_optimizer("adam", m, 1e-3), TU.L2Loss(0.0), False) is True
    assert TU._last_layer_step_applies(m, MT.build_optimizer(NAME, m, 1e-3, table_rowwise=True), TU.L2Loss(0.0), False) is False


def test_the_run_says_row_wise(capsys):
    m = _model()
    TU._announce_split_route(MT.build_optimizer(NAME, m, 1e-3, 160.0, table_rowwise=True), TU.L2Loss(0.0), True)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "row-wise" in out and "fused step" in out and "160.0" in out
    TU._announce_split_route(MT.build_optimizer(NAME, m, 1e-3, 160.0, table_rowwise=True), TU.L2Loss(1e-3), False)
    out = capsys.readouterr().out
    assert "row-wise" in out and "torch route" in out and "weight decay reaches the embedding tables" in out
    TU._announce_split_route(MT.build_optimizer(NAME, m, 1e-3, 160.0), TU.L2Loss(0.0), True)
    assert "row-wise" not in capsys.readouterr().out


def test_the_three_clis_take_the_flag_and_other_optimizers_refuse_it():
    from nasrec_amd import eval_subnet_from_scratch, train_supernet
    for mod in (MT, train_supernet, eval_subnet_from_scratch):
        by_flag = {s: a for a in mod.build_parser()._actions for s in a.option_strings}
        act = by_flag["--table-rowwise"]
        assert act.dest == "table_rowwise" and act.default is False and act.const is True and act.nargs == 0, mod.__name__
    m = _model()
    for name in ("adagrad", "adam", "sgd", "row-sparse-adam", "rmsprop"):
        with pytest.raises(ValueError, match="--table-rowwise.*--optimizer"):
            MT.build_optimizer(name, m, 1e-3, table_rowwise=True)
        MT.build_optimizer(name, m, 1e-3, table_rowwise=False)


# ------------------------------------------------------------------------------------------------------------------ bound state
def test_bound_state_shares_the_row_accumulators(monkeypatch):
    """engine_bind_optimizer / engine_sync_optimizer_steps over host arrays: a table's `sum` aliases table_row_state (an existing one — a
    resumed checkpoint — is copied in), table_state stays None, the engine holds no table moments; the other rule's `sum` is refused"""
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    m = _model()
    opt = MT.build_optimizer(NAME, m, 1e-3, 50.0, table_rowwise=True)
    w0 = m._embedding[0].weight
    opt.state[w0]["step"] = torch.tensor(3.0)
    opt.state[w0]["sum"] = torch.arange(7, dtype=torch.float32) * 0.25
    eng = m.__dict__["_engine"] = _HostEngine(m)
    m.engine_bind_optimizer(opt)
    assert eng.table_state is None
    assert all(tabs == [] for _, tabs in eng.moments.values()) and set(eng.moments) == {"exp_avg", "exp_avg_sq"}
    assert [tuple(t.shape) for t in eng.table_row_state] == [(7,), (5,)] and all(t.dtype == torch.float32 for t in eng.table_row_state)
    assert torch.equal(eng.table_row_state[0], torch.arange(7, dtype=torch.float32) * 0.25)
    assert int(eng.table_row_state[1].count_nonzero()) == 0
    assert float(eng.opt_steps[eng.param_index["_embedding.0.weight"]]) == 3.0
    with pytest.raises(L.EngineError, match="table_row_state"):
        eng.moments_view("exp_avg", "_embedding.0.weight")
    # two fused steps that reached the dense parameters and table 0 only
    eng.opt_steps.add_(2.0)
    eng.opt_steps[eng.param_index["_embedding.1.weight"]] = 0.0
    m.__dict__["_engine_steps"] = 2
    m.engine_sync_optimizer_steps(opt)
    arrays = _engine_arrays(eng) + list(eng.table_row_state)
    got = {}
    for n, p in m.named_parameters():
        st = opt.state.get(p)
        if st:
            got[n] = sorted((k, _aliases(v, arrays) if k != "step" else False, float(v) if k == "step" else None) for k, v in st.items())
    dense = [("exp_avg", True, None), ("exp_avg_sq", True, None), ("step", False, 2.0)]
    assert got == {"_embedding.0.weight": [("step", False, 5.0), ("sum", True, None)],
                   "lin.weight": dense, "lin.bias": dense, "_final.weight": dense, "_final.bias": dense}
    assert opt.state[w0]["sum"].data_ptr() == eng.table_row_state[0].data_ptr() and opt.state[w0]["sum"].shape == (7,)
    assert eng.table_state is None
    # an element-wise `sum` under the row-wise rule, and the reverse
    for rowwise, bad in ((True, torch.full_like(w0, 0.25)), (False, torch.ones(7))):
        m2 = _model()
        o2 = MT.build_optimizer(NAME, m2, 1e-3, 50.0, table_rowwise=rowwise)
        o2.state[m2._embedding[0].weight]["step"] = torch.tensor(3.0)
        o2.state[m2._embedding[0].weight]["sum"] = bad.clone()
        m2.__dict__["_engine"] = _HostEngine(m2)
        with pytest.raises(ValueError, match="row-wise" if rowwise else "element-wise"):
            m2.engine_bind_optimizer(o2)


# -------------------------------------------------------------------------------------------------------------------- replicas
def test_the_replicas_compare_the_rule():
    """what assert_replicas_identical all-reduces (MIN against MAX): two ranks that disagree on the tables' rule hold different numbers —
    before, the element-wise and the row-wise rule both encoded as 2"""
    from nasrec_amd.utils import dist as D
    m = _model()
    codes = {name: D.table_rule_code(OptimSpec.from_optimizer(opt)) for name, opt in (
        ("adam", MT.build_optimizer("adam", m, 1e-3)), ("row-sparse-adam", MT.build_optimizer("row-sparse-adam", m, 1e-3)),
        ("elementwise", MT.build_optimizer(NAME, m, 1e-3)), ("rowwise", MT.build_optimizer(NAME, m, 1e-3, table_rowwise=True)))}
    assert codes == {"adam": 0, "row-sparse-adam": 1, "elementwise": 2, "rowwise": 3}
    assert D.table_rule_code(None) == 0 and len(set(codes.values())) == 4
    # the row accumulators are replica state: broadcast and checksummed with the rest
    eng = types.SimpleNamespace(flat_s=None, table_state=None, table_row_state=[torch.ones(7), torch.ones(5)])
    m.__dict__["_engine"] = eng
    tensors = D._replica_tensors(m)
    assert any(t is eng.table_row_state[0] for t in tensors) and any(t is eng.table_row_state[1] for t in tensors)
    m.__dict__["_engine"] = types.SimpleNamespace(flat_s=None, table_state=None)  # (an engine from before the attribute: nothing to add)
    assert len(D._replica_tensors(m)) == len(tensors) - 2


# ------------------------------------------------------------------------------------------------------------ row-sharded checkpoint
def test_a_row_sharded_checkpoint_gathers_a_1d_shard():
    """row-sharded tables train with this optimizer on the torch route: the checkpoint gathers the optimizer's own 1-D `sum` through
    RowShardedTables.whole_table, which keeps its trailing shape — [rows], not [rows, 16], and not a broadcast of it"""
    from nasrec_amd.sharded_tables import RowShardedTables
    from nasrec_amd.utils.io_utils import optimizer_state_for_checkpoint
    m = _model()
    opt = MT.build_optimizer(NAME, m, 1e-3, 50.0, table_rowwise=True)
    for f in range(2):
        w = m._embedding[f].weight
        w.grad = torch.randn_like(w)
    opt.step()
    # one process standing in for rank 0 of 1: whole_table's own code, no collective (world == 1 takes the `parts = [mine]` branch);
    # rp > rows held: the padded tail of `mine` is cut off again
    sh = types.SimpleNamespace(tables={}, state={}, num_embeddings=[7, 5], rp=[16, 16], lo=[0, 0], hi=[7, 5], device=torch.device("cpu"),
                               world=1, group=None)
    sh.whole_table = types.MethodType(RowShardedTables.whole_table, sh)
    for f in range(2):
        own = opt.state[m._embedding[f].weight]["sum"]
        whole = sh.whole_table(f, "state", shard=own)
        assert whole.shape == own.shape == (sh.num_embeddings[f],) and torch.equal(whole, own)
        two_d = sh.whole_table(f, "state", shard=own.view(-1, 1).expand(-1, 16).contiguous())
        assert two_d.shape == (sh.num_embeddings[f], 16)
    sh.world = 2  # (optimizer_state_for_checkpoint gathers only in a sharded run; the stand-in keeps the one-process branch)
    calls = []
    real = sh.whole_table

    def whole_table(f, which="tables", shard=None):
        calls.append((f, which, shard))
        sh.world = 1
        try:
            return real(f, which, shard=shard)
        finally:
            sh.world = 2
    sh.whole_table = whole_table
    m.__dict__.update(_table_sharding="row", _sharded=sh)
    sd = optimizer_state_for_checkpoint(m, opt)
    assert [(f, which) for f, which, _ in calls] == [(0, "state"), (1, "state")]
    assert calls[0][2] is opt.state[m._embedding[0].weight]["sum"]
    assert sd["state"][0]["sum"].shape == (7,) and torch.equal(sd["state"][0]["sum"], opt.state[m._embedding[0].weight]["sum"])
    assert sd["state"][1]["sum"].shape == (5,) and sd["param_groups"][0]["table_rowwise"] is True
