"""`--optimizer rowwise-adam` without a GPU: utils/optim.RowwiseSparseAdam (row-sparse Adam with ONE second-moment float per embedding
row) against an fp64 NumPy restatement written out here, its state shapes, its checkpoint and the two cross-load refusals with
RowSparseAdam, the OptimSpec (table_kind "rowwise_adam", no new field), the harness's choice of route, the CLIs, the replicas' rule
code, the binding's constants and the launcher's refusals (every one returns -1 before anything is launched, so they run without a
device).  Helpers from test_optim_routing_cpu.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import RowSparseAdam, RowwiseSparseAdam
from test_optim_routing_cpu import _last_layer_mode, _model, one_process  # noqa: F401

NAME = "rowwise-adam"
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-8
ROWS = (50, 1)
# ids [B, 2] per step: duplicates inside a batch (rows 3 and 7 of table 0); table 1 has one row; rows 30.. of table 0 are in no batch
IDS = [[[3, 0], [3, 0], [7, 0], [12, 0]], [[7, 0], [7, 0], [0, 0], [29, 0]], [[3, 0], [12, 0], [12, 0], [5, 0]]]
ZERO = {0: 12, 1: 0, 2: 3}  # step -> the touched row of table 0 whose gradient is exactly zero in that step


def _close(a, b, what):
    """the kernel tests' bar: one step from fp32 inputs, in fp32 against fp64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.allclose(a, b, rtol=2e-6, atol=2e-7), (what, float(np.abs(a - b).max()))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    tables = [torch.nn.Parameter(torch.randn(n, 16, generator=g)) for n in ROWS]
    dense = torch.nn.Parameter(torch.randn(8, 3, generator=g))
    return tables, dense


def _grads(step):
    """dense gradients on every row, touched or not (the optimizer must not guess the touched rows from them); one touched row of
    table 0 gets an exactly zero gradient"""
    g = torch.Generator().manual_seed(100 + step)
    gt = [torch.randn(n, 16, generator=g) for n in ROWS]
    gt[0][ZERO[step]] = 0.0
    return gt, torch.randn(8, 3, generator=g)


def test_three_steps_against_fp64():
    """every step's table update is restated in fp64 from the fp32 state it started from; the dense weight takes torch.optim.Adam's
    bits (a twin under torch.optim.Adam sees the same gradients)"""
    tables, dense = _params()
    twin = torch.nn.Parameter(dense.detach().clone())
    start = [t.detach().clone() for t in tables]
    opt = RowwiseSparseAdam(tables + [dense], tables, lr=LR)
    adam = torch.optim.Adam([twin], lr=LR)
    touched_ever = [np.zeros(n, bool) for n in ROWS]
    zero_rows_that_moved = 0
    for step, ids in enumerate(IDS):
        ids = torch.tensor(ids)
        gt, gd = _grads(step)
        t = step + 1
        step_size = LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
        want = []
        for f, w in enumerate(tables):
            st = opt.state[w] if w in opt.state and "exp_avg" in opt.state[w] else None
            m = st["exp_avg"].double().numpy().copy() if st else np.zeros((ROWS[f], 16))
            v = st["exp_avg_sq"].double().numpy().copy() if st else np.zeros(ROWS[f])
            p = w.detach().double().numpy().copy()
            g = gt[f].double().numpy()
            for r in sorted(set(int(i) for i in ids[:, f])):
                m[r] += (g[r] - m[r]) * (1 - B1)
                v[r] += ((g[r] * g[r]).sum() / 16.0 - v[r]) * (1 - B2)
                p[r] -= step_size * m[r] / (np.sqrt(v[r]) + EPS)
                touched_ever[f][r] = True
            want.append((p, m, v))
            w.grad = gt[f].clone()
        dense.grad, twin.grad = gd.clone(), gd.clone()
        before = [(w.detach().clone(), None if w not in opt.state or "exp_avg" not in opt.state[w] else
                   (opt.state[w]["exp_avg"].clone(), opt.state[w]["exp_avg_sq"].clone())) for w in tables]
        opt.touch(ids)
        opt.step()
        adam.step()
        for f, w in enumerate(tables):
            st = opt.state[w]
            assert st["exp_avg"].shape == (ROWS[f], 16) and st["exp_avg_sq"].shape == (ROWS[f],) and st["exp_avg_sq"].dtype == torch.float32
            assert float(st["step"]) == t
            _close(w.detach(), want[f][0], ("p", f, step))
            _close(st["exp_avg"], want[f][1], ("m", f, step))
            _close(st["exp_avg_sq"], want[f][2], ("v", f, step))
            # a row outside THIS batch keeps its bits in p, m and v, whatever its dense gradient
            rest = torch.ones(ROWS[f], dtype=torch.bool)
            rest[ids[:, f].unique()] = False
            assert torch.equal(w.detach()[rest], before[f][0][rest]), ("p", f, step)
            if before[f][1] is not None:
                assert torch.equal(st["exp_avg"][rest], before[f][1][0][rest]) and torch.equal(st["exp_avg_sq"][rest], before[f][1][1][rest])
        # the touched row with an exactly zero gradient: step 0 starts from zero moments and stays; later it decays m and v and moves
        r = ZERO[step]
        w, st = tables[0], opt.state[tables[0]]
        if before[0][1] is not None and bool(before[0][1][0][r].abs().sum() > 0):
            assert not torch.equal(w.detach()[r], before[0][0][r]) and not torch.equal(st["exp_avg"][r], before[0][1][0][r])
            assert float(st["exp_avg_sq"][r]) < float(before[0][1][1][r])
            zero_rows_that_moved += 1
    assert zero_rows_that_moved == 1  # (row 3 at the third step: it had moments from the first)
    # rows never touched: bit for bit as they started, zero moments
    for f, w in enumerate(tables):
        rest = torch.from_numpy(~touched_ever[f])
        assert int(rest.sum()) == (ROWS[f] - 6 if f == 0 else 0)
        assert torch.equal(w.detach()[rest], start[f][rest])
        assert int(opt.state[w]["exp_avg"][rest].count_nonzero()) == 0 and int(opt.state[w]["exp_avg_sq"][rest].count_nonzero()) == 0
    # the dense weight: torch.optim.Adam bit for bit, Adam's state shape
    assert torch.equal(dense.detach(), twin.detach())
    sa, sb = opt.state[dense], adam.state[twin]
    assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"} and sa["exp_avg_sq"].shape == (8, 3)
    for k in sa:
        assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), k


def test_one_second_moment_divides_the_whole_row_and_differs_from_row_sparse_adam():
    ta, da = _params()
    tb, db = _params()
    oa, ob = RowwiseSparseAdam(ta + [da], ta, lr=LR), RowSparseAdam(tb + [db], tb, lr=LR)
    gt, gd = _grads(0)
    ids = torch.tensor(IDS[0])
    for tabs, dense, opt in ((ta, da, oa), (tb, db, ob)):
        for w, g in zip(tabs, gt):
            w.grad = g.clone()
        dense.grad = gd.clone()
        opt.touch(ids)
        opt.step()
    assert torch.equal(da.detach(), db.detach())
    assert not torch.equal(ta[0].detach(), tb[0].detach())
    assert oa.state[ta[0]]["exp_avg_sq"].shape == (50,) and ob.state[tb[0]]["exp_avg_sq"].shape == (50, 16)
    assert torch.equal(oa.state[ta[0]]["exp_avg"], ob.state[tb[0]]["exp_avg"])  # (the first moment stays per element)
    # first step from zero moments: (p0 - p) / g is ONE number across the row
    p0 = _params()[0][0].detach()
    ratio = ((p0[7] - ta[0].detach()[7]).double() / gt[0][7].double())[gt[0][7].abs() > 0.1]
    assert float((ratio.max() - ratio.min()) / ratio.mean().abs()) < 1e-4


def test_step_without_touch_raises_and_a_table_must_be_2d():
    tables, dense = _params()
    opt = RowwiseSparseAdam(tables + [dense], tables, lr=LR)
    tables[0].grad = torch.ones_like(tables[0])
    with pytest.raises(RuntimeError, match="touch"):
        opt.step()
    v = torch.nn.Parameter(torch.randn(6))
    with pytest.raises(ValueError, match=r"\(6,\)"):
        RowwiseSparseAdam([v], [v])
    t3 = torch.nn.Parameter(torch.randn(2, 3, 4))
    with pytest.raises(ValueError, match=r"\(2, 3, 4\)"):
        RowwiseSparseAdam([t3], [t3])
    RowwiseSparseAdam([v, tables[1]], [tables[1]])  # (a 1-D dense parameter is fine)
    assert set(opt.param_groups[0]) == set(RowSparseAdam(tables + [dense], tables).param_groups[0])


def _stepped(cls, seed=0, steps=2):
    tables, dense = _params(seed)
    opt = cls(tables + [dense], tables, lr=LR)
    for step in range(steps):
        gt, gd = _grads(step)
        for w, g in zip(tables, gt):
            w.grad = g.clone()
        dense.grad = gd.clone()
        opt.touch(torch.tensor(IDS[step]))
        opt.step()
    return tables, dense, opt


def test_checkpoint_round_trip_gives_the_same_next_step():
    ta, da, oa = _stepped(RowwiseSparseAdam)
    tb, db = _params()
    with torch.no_grad():
        for dst, src in zip(tb + [db], ta + [da]):
            dst.copy_(src)
    ob = RowwiseSparseAdam(tb + [db], tb, lr=0.5)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert ob.param_groups[0]["lr"] == LR
    assert ob.state[tb[0]]["exp_avg_sq"].shape == (50,) and ob.state[tb[1]]["exp_avg_sq"].shape == (1,)
    gt, gd = _grads(2)
    for tabs, dense, opt in ((ta, da, oa), (tb, db, ob)):
        for w, g in zip(tabs, gt):
            w.grad = g.clone()
        dense.grad = gd.clone()
        opt.touch(torch.tensor(IDS[2]))
        opt.step()
    for a, b in zip(ta + [da], tb + [db]):
        assert torch.equal(a.detach(), b.detach())
        for k, v in oa.state[a].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(ob.state[b][k])), k


def test_the_other_forms_checkpoint_is_refused_both_ways():
    """a RowSparseAdam checkpoint into a RowwiseSparseAdam and the reverse: ValueError that names the rule, nothing loaded"""
    _, _, rowwise = _stepped(RowwiseSparseAdam)
    _, _, elementwise = _stepped(RowSparseAdam)
    sd_row, sd_elem = copy.deepcopy(rowwise.state_dict()), copy.deepcopy(elementwise.state_dict())
    for opt, other, word in ((rowwise, sd_elem, "row-wise"), (elementwise, sd_row, "element-wise")):
        before = copy.deepcopy(opt.state_dict())
        with pytest.raises(ValueError, match=word) as e:
            opt.load_state_dict(copy.deepcopy(other))
        assert "RowSparseAdam" in str(e.value) and "RowwiseSparseAdam" in str(e.value)
        after = opt.state_dict()
        assert after["param_groups"] == before["param_groups"]
        assert all(torch.equal(torch.as_tensor(v), torch.as_tensor(after["state"][i][k])) for i, st in before["state"].items() for k, v in st.items())
    # a state put there by hand is caught by step() before anything broadcasts: [16] against a [16, 16] table would
    w = torch.nn.Parameter(torch.randn(16, 16))
    opt = RowwiseSparseAdam([w], [w])
    opt.state[w].update(step=torch.tensor(1.0), exp_avg=torch.zeros(16, 16), exp_avg_sq=torch.ones(16, 16))
    w.grad = torch.randn(16, 16)
    w0 = w.detach().clone()
    opt.touch(torch.tensor([[1]]))
    with pytest.raises(ValueError, match=r"\(16, 16\)"):
        opt.step()
    assert torch.equal(w.detach(), w0)


# ------------------------------------------------------------------------------------------------------------------------- spec
def test_spec_mapping_and_rows_only():
    m = _model()
    opt = MT.build_optimizer(NAME, m, 0.05)
    assert type(opt) is RowwiseSparseAdam and opt.param_groups[0]["lr"] == 0.05 and opt.param_groups[0]["eps"] == 1e-8
    spec = OptimSpec.from_optimizer(opt)
    assert spec == OptimSpec("adam", beta1=0.9, beta2=0.999, eps=1e-8, table_kind="rowwise_adam")
    assert spec.rows_only and spec.table_rowwise and spec.rowwise_adam and not spec.adagrad_tables and not spec.sparse_rows
    assert not spec.bf16_tables and spec.table_seed == 0 and spec.table_lr_scale == 1.0
    assert spec.moments and spec.state_keys == ("exp_avg", "exp_avg_sq")
    assert OptimSpec._fields == ("kind", "beta1", "beta2", "eps", "momentum", "nesterov", "wd", "no_reg", "sparse_rows", "alpha",
                                 "table_kind", "table_eps", "table_lr_scale", "dwd", "ema")
    sparse = OptimSpec.from_optimizer(MT.build_optimizer("row-sparse-adam", m, 0.05))
    assert sparse.sparse_rows and not sparse.rowwise_adam and not sparse.table_rowwise and spec != sparse
    assert OptimSpec.of(optim=spec) != OptimSpec.of(optim=sparse)  # (plan-cache keys hold the spec: two plans)
    split = OptimSpec.from_optimizer(MT.build_optimizer("adam-adagrad-tables", m, 0.05, table_rowwise=True))
    assert split.adagrad_tables and not split.rowwise_adam
    # the regularised-table rule of for_step: the torch route
    assert OptimSpec.for_step(opt) == spec
    assert OptimSpec.for_step(opt, 1e-3, None) is None and OptimSpec.for_step(opt, 1e-3, "lin") is None
    assert OptimSpec.for_step(opt, 1e-3, "_embedding") == spec._replace(wd=1e-3, no_reg="_embedding")
    # Adam's disqualifiers hold for it too
    opt.param_groups[0]["amsgrad"] = True
    assert OptimSpec.from_optimizer(opt) is None
    # the descriptor's scalars
    from nasrec_amd.engine import SupernetEngine
    d = L.OptMomentsDesc()
    SupernetEngine._optim_scalars(d, spec)
    assert d.algo == L.OPTIM_ADAM and d.sparse_rows == 0
    with pytest.raises(L.EngineError, match="table_kind"):
        SupernetEngine._optim_scalars(d, spec._replace(kind="sgd"))


def test_fused_step_spec_answers(one_process):  # noqa: F811
    m = _model()
    m.engine_train_step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("not called here"))
    opt = MT.build_optimizer(NAME, m, 1e-3)
    plain = TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False)  # no weight decay
    assert plain is not None and plain.table_kind == "rowwise_adam" and plain.wd == 0.0
    dense_only = TU._fused_step_spec(m, opt, TU.L2Loss(1e-3, "_embedding"), False)  # weight decay on the dense parameters only
    assert dense_only == plain._replace(wd=1e-3, no_reg="_embedding")
    assert TU._fused_step_spec(m, opt, TU.L2Loss(1e-3), False) is None   # a regularised table: the torch route
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), True) is None    # AMP
    # the weight average and the decoupled decay ride in the fused step, as with row-sparse Adam
    from nasrec_amd.utils.optim import DecoupledWeightDecay, WeightEMA
    assert TU._ema_route(m, plain, TU.L2Loss(0.0)) is None
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, WeightEMA(m, 0.99)).ema == 0.99
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False, None, DecoupledWeightDecay(m, 0.1)).dwd == 0.1
    # row-sharded tables and tables on the host keep the torch route
    m.__dict__["_table_sharding"] = "row"
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False) is None
    m.__dict__.update(_table_sharding=None, _place_embedding_on_cpu=True)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0), False) is None
    # the harness refuses a regularised table on either route, as for row-sparse Adam; row-sharded tables are refused at construction
    m.__dict__["_place_embedding_on_cpu"] = False
    with pytest.raises(ValueError, match="--no-reg-param-name _embedding"):
        TU._refuse_regularised_tables(opt, TU.L2Loss(1e-3, None))
    TU._refuse_regularised_tables(opt, TU.L2Loss(1e-3, "_embedding"))
    m.__dict__["_table_sharding"] = "row"
    with pytest.raises(ValueError, match="whole tables"):
        MT.build_optimizer(NAME, m, 1e-3)


def test_the_last_layer_step_is_taken_as_with_row_sparse_adam(one_process):  # noqa: F811
    m = _model()
    _last_layer_mode(m)
    want = TU._last_layer_step_applies(m, MT.build_optimizer("row-sparse-adam", m, 1e-3), TU.L2Loss(0.0), False)
    assert TU._last_layer_step_applies(m, MT.build_optimizer(NAME, m, 1e-3), TU.L2Loss(0.0), False) is want is True


def test_the_run_says_which_route(capsys):
    m = _model()
    TU._announce_rowwise_adam_route(m, MT.build_optimizer(NAME, m, 1e-3), TU.L2Loss(0.0), False, True)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "Row-wise Adam" in out and "fused step" in out
    TU._announce_rowwise_adam_route(m, MT.build_optimizer(NAME, m, 1e-3), TU.L2Loss(0.0), True, False)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "torch route" in out and "AMP" in out
    opt = MT.build_optimizer(NAME, m, 1e-3)
    TU._announce_rowwise_adam_route(m, opt, TU.L2Loss(0.0), False, False, switched_off=True)
    TU._announce_rowwise_adam_route(m, opt, TU.L2Loss(0.0), False, False, switched_off=True)  # (once per run)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "switched off" in out
    TU._announce_rowwise_adam_route(m, MT.build_optimizer("row-sparse-adam", m, 1e-3), TU.L2Loss(0.0), False, True)
    assert capsys.readouterr().out == ""


def test_every_cli_offers_the_name_and_table_rowwise_keeps_raising():
    from nasrec_amd import eval_subnet_from_scratch, eval_subnet_from_supernet, train_supernet
    for mod in (MT, train_supernet, eval_subnet_from_scratch, eval_subnet_from_supernet):
        opts = [a for a in mod.build_parser()._actions if "--optimizer" in a.option_strings]
        assert len(opts) == 1 and NAME in opts[0].choices and "row-sparse-adam" in opts[0].choices, mod.__name__
    m = _model()
    for name in (NAME, "row-sparse-adam"):
        with pytest.raises(ValueError, match="--table-rowwise.*--optimizer"):
            MT.build_optimizer(name, m, 1e-3, table_rowwise=True)
    # the candidate fine-tune builds it too
    import types
    args = types.SimpleNamespace(wd=0.0, gpu=None, optimizer=NAME, learning_rate=1e-3, max_train_steps=10, num_epochs=1, lr_schedule="none")
    assert type(eval_subnet_from_supernet.make_optimizer_and_schedule(m, args)[1]) is RowwiseSparseAdam


def test_the_replicas_compare_the_rule():
    from nasrec_amd.utils import dist as D
    m = _model()
    codes = {name: D.table_rule_code(OptimSpec.from_optimizer(opt)) for name, opt in (
        ("adam", MT.build_optimizer("adam", m, 1e-3)), ("row-sparse-adam", MT.build_optimizer("row-sparse-adam", m, 1e-3)),
        ("elementwise", MT.build_optimizer("adam-adagrad-tables", m, 1e-3)),
        ("rowwise", MT.build_optimizer("adam-adagrad-tables", m, 1e-3, table_rowwise=True)),
        (NAME, MT.build_optimizer(NAME, m, 1e-3)))}
    codes["bf16"] = D.table_rule_code(OptimSpec("adam", table_kind=OptimSpec.bf16_table_kind(3)))
    assert {k: v for k, v in codes.items() if k != NAME} == {"adam": 0, "row-sparse-adam": 1, "elementwise": 2, "rowwise": 3, "bf16": 4}
    assert codes[NAME] not in (0, 1, 2, 3, 4) and len(set(codes.values())) == 6


# ---------------------------------------------------------------------------------------------------------------------- binding
def test_lib_constants():
    assert L.TABLE_ALGO_ROWWISE_ADAM == 5
    assert (L.TABLE_ALGO_SAME, L.TABLE_ALGO_ADAGRAD, L.TABLE_ALGO_ROWWISE_ADAGRAD, L.TABLE_ALGO_ROWWISE_ADAGRAD_BF16) == (0, 1, 3, 4)
    assert C.sizeof(L.OptMomentsDesc) == 1568 and L.load().nasrec_abi_version() == 17
    sizes = (C.c_int32 * 43)()
    assert L.load().nasrec_desc_sizes(sizes, 43) > L.OP_OPT_MOMENTS and sizes[L.OP_OPT_MOMENTS] == 1568


def _desc(store, counter=False, **kw):
    """a row-wise Adam descriptor whose pointers are host words (never dereferenced: every case below is refused before a launch).
    `counter` stays NULL unless asked for, which phase 0's last check refuses: a phase-0 case whose own refusal failed to fire still
    launches nothing."""
    def ptr():
        store.append((C.c_double * 64)())
        return C.addressof(store[-1])
    d = L.OptMomentsDesc()
    d.kind, d.phase, d.algo, d.table_algo = L.OP_OPT_MOMENTS, 0, L.OPTIM_ADAM, L.TABLE_ALGO_ROWWISE_ADAM
    d.dense_blocks, d.nblocks, d.B, d.Fs, d.table_step0 = 1, 3, 4, 2, 1
    d.eps, d.beta1, d.beta2 = 1e-8, 0.9, 0.999
    d.lr, d.step, d.idx, d.leader, d.gsum, d.bitmap, d.coef = ptr(), ptr(), ptr(), ptr(), ptr(), ptr(), ptr()
    for f in range(2):
        d.table[f], d.tm[f], d.tv[f], d.rows[f] = ptr(), ptr(), ptr(), 4
    if counter:
        d.counter = ptr()
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


REFUSALS = {
    "sgd": (dict(algo=L.OPTIM_SGD), b"table_algo"),
    "rmsprop": (dict(algo=L.OPTIM_RMSPROP), b"table_algo"),
    "sparse-rows": (dict(sparse_rows=1), b"sparse_rows"),
    "reg-mask": (dict(reg_mask=2), b"reg_mask"),
    "no-table": (dict(table=(1, None)), b"table 1"),
    "no-tv": (dict(tv=(0, None)), b"(tv) of table 0"),
    "no-tm": (dict(tm=(1, None)), b"(tm) of table 1"),
    "no-counter": (dict(), b"counter"),
    "phase-1-tile": (dict(phase=1, n_zero=1, tile_off=(2, 1), counter=True), b"no table owns a tile"),  # (phase 1 asks for the counter first)
    "phase-1-without-zero-chunks": (dict(phase=1, counter=True), b"no table owns a tile"),
    "phase-2": (dict(phase=2), b"phase 2"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_launcher_refusals_return_minus_one_before_any_launch(what):
    kw, word = REFUSALS[what]
    store = []
    d = _desc(store, **kw)
    lib = L.load()
    assert lib.nasrec_launch(None, C.addressof(d)) == -1
    err = lib.nasrec_last_error()
    assert b"opt_moments" in err and word in err, err


def test_table_eps_is_not_among_the_refusals():
    """row-wise Adagrad's table_eps <= 0 refusal is the one this rule drops: with table_eps 0 the launcher walks on to its last check"""
    store = []
    d = _desc(store, table_eps=0.0)
    lib = L.load()
    assert lib.nasrec_launch(None, C.addressof(d)) == -1
    assert b"table_eps" not in lib.nasrec_last_error() and b"counter" in lib.nasrec_last_error()
    d = _desc(store, table_eps=0.0, table_algo=L.TABLE_ALGO_ROWWISE_ADAGRAD)
    assert lib.nasrec_launch(None, C.addressof(d)) == -1 and b"table_eps" in lib.nasrec_last_error()
