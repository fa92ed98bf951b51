"""`--optimizer adam-adagrad-tables --table-rowwise` (utils/optim.AdamAdagradTables(table_rowwise=True): Adam on the network, row-wise
Adagrad on the tables — one accumulator per embedding row, fed the mean of the row's squared gradient) in the fused engine step, on the
GPU.  Helpers and bars from test_split_optimizer_gpu.py: tables atol 2e-5, `sum` rtol 1e-4 / atol 1e-9, the dense half F.TOL["adam"].

Small network (RS._small: tables of at most 997 rows, 4 batches of 16): the fused step against the torch route; graph replay equals
launching; a supernet under any-path sampling; a path that leaves the stem out; resume onto both routes; a weight average and a decoupled
weight decay that reaches the tables, each against the torch route; the engine's state afterwards — `table_state` never allocated, no
table moment array, one float per table row in `table_row_state`; rows outside the batches keep their bits and a zero accumulator; the
element-wise and the row-wise rule are two plans.  One harness case: main_train's arguments with --table-rowwise at batch 8 for 5 steps
(wd 0), which prints the fused-route line and equals the torch route."""
import copy

import numpy as np
import pytest
import torch

import test_fused_optimizers_gpu as F
import test_row_sparse_adam_gpu as RS
from nasrec_amd import main_train as MT
from nasrec_amd._lib import EngineError
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import AdamAdagradTables, DecoupledWeightDecay, WeightEMA
from test_split_optimizer_gpu import LR, NAME, NO_REG, SCALE, TABLE_ATOL, TOL, _compare, _dense

pytestmark = pytest.mark.gpu


def _opt(m, rowwise=True):
    return MT.build_optimizer(NAME, m, LR, SCALE, table_rowwise=rowwise)


def _fused_steps(base, batches, wd=0.0, graph=None, sampler=None, state=None, use_model=None, **step_kw):
    """engine_train_step over `batches` on a copy of `base` -> (parameters, optimizer state, did each step's backward reach the stem, model)"""
    m = copy.deepcopy(base) if use_model is None else use_model
    opt = _opt(m)
    if state is not None:
        opt.load_state_dict(copy.deepcopy(state))
    spec = OptimSpec.from_optimizer(opt)
    assert spec.table_kind == "rowwise_adagrad" and spec.table_lr_scale == SCALE and spec.rows_only
    if sampler is not None:
        np.random.seed(sampler)
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    stem = []
    for int_x, cat_x, y in batches:
        m.engine_train_step(int_x, cat_x, y, lr=LR, clip=5.0, graph=graph, weight_decay=wd, no_reg_param_name=NO_REG if wd else None, optim=spec,
                            **step_kw)
        stem.append(bool(m._engine._last_plan[2].sparse0.grad_written))
    m.engine_sync_optimizer_steps(opt)
    torch.cuda.synchronize()
    assert int(m._engine._row_bitmap().abs().sum()) == 0 and int(m._engine._mom_counter[0]) == 0
    m.__dict__["_test_opt"] = opt
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt), stem, m


def _torch_steps(base, batches, wd=0.0, sampler=None, state=None, use_model=None, ema=None, decay=None):
    m = copy.deepcopy(base) if use_model is None else use_model
    opt = _opt(m)
    if state is not None:
        opt.load_state_dict(copy.deepcopy(state))
    if sampler is not None:
        np.random.seed(sampler)
    avg = WeightEMA(m, ema) if ema else None
    dec = DecoupledWeightDecay(m, decay, None) if decay else None
    for int_x, cat_x, y in batches:
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x).view(-1), y) + TU.get_l2_loss(m, wd, NO_REG, gpu=0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        if dec is not None:
            dec.apply(LR)
        opt.step()
        if avg is not None:
            avg.update()
    torch.cuda.synchronize()
    shadow = {n: s.detach().cpu().clone() for n, s in avg.shadow.items()} if avg is not None else None
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt), shadow


def _sums_are_per_row(state, params):
    for k, s in state.items():
        if k.startswith("_embedding."):
            assert tuple(s["sum"].shape) == (params[k].shape[0],), (k, tuple(s["sum"].shape))


@pytest.fixture(scope="module")
def best():
    choice = RS._best_1shot()
    return RS._small(choice, blocks=choice["num_blocks"], config=choice["config"], layernorm=False, seed=3)


@pytest.fixture(scope="module")
def best_torch(best):
    """the torch route on the small fixed network, once"""
    base, batches = best
    return _torch_steps(base, batches)


def test_fused_step_equals_the_torch_route_and_keeps_one_float_per_row(best, best_torch):
    base, batches = best
    pa, sa, stem, m = _fused_steps(base, batches)
    pb, sb, _ = best_torch
    assert all(stem)
    _compare(pa, sa, pb, sb, "row-wise, small best-1shot")
    _sums_are_per_row(sa, pa)
    _sums_are_per_row(sb, pb)
    assert all(float(s["step"]) == 4.0 for s in sa.values())
    eng = m._engine
    # the engine's state: Adam's moments over the dense arena only, one accumulator per table row, and no [rows, 16] table state at all
    assert eng.table_state is None
    assert set(eng.moments) == {"exp_avg", "exp_avg_sq"} and all(tabs == [] for _, tabs in eng.moments.values())
    rows = sum(int(t.shape[0]) for t in eng.tables)
    assert len(eng.table_row_state) == 26 and sum(t.numel() for t in eng.table_row_state) == rows
    assert all(t.dim() == 1 and t.dtype == torch.float32 for t in eng.table_row_state)
    opt = m.__dict__["_test_opt"]
    assert opt.state[m._embedding[3].weight]["sum"].data_ptr() == eng.table_row_state[3].data_ptr()
    assert opt.state[m._final.weight]["exp_avg"].data_ptr() == eng.moments_view("exp_avg", "_final.weight").data_ptr()
    with pytest.raises(EngineError, match="table_row_state"):
        eng.moments_view("exp_avg", "_embedding.3.weight")
    # rows outside the batches: the bits they started with, nothing accumulated; the batches' rows moved and accumulated
    ids = torch.cat([b[1] for b in batches]).cpu()
    for f in range(26):
        k = "_embedding.%d.weight" % f
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        t0 = base._embedding[f].weight.detach().cpu()
        assert torch.equal(pa[k][rest], t0[rest]) and not sa[k]["sum"][rest].any(), k
        assert bool((sa[k]["sum"][~rest] > 0).all()) and not torch.equal(pa[k][~rest], t0[~rest]), k


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_graph_replay_equals_launch(best, wd):
    base, batches = best
    (pa, sa, _, _), (pb, sb, _, _) = _fused_steps(base, batches, wd, graph=False), _fused_steps(base, batches, wd, graph=True)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert set(sa) == set(sb)
    for n in sa:
        for k in sa[n]:
            assert torch.equal(torch.as_tensor(sa[n][k]), torch.as_tensor(sb[n][k])), (n, k)
    assert any(not torch.equal(pa["_embedding.%d.weight" % f], base._embedding[f].weight.detach().cpu()) for f in range(26))


def test_the_two_table_rules_are_two_plans_and_differ(best):
    base, batches = best
    m = copy.deepcopy(base)
    m._ensure_engine(batches[0][0])
    eng = m._engine
    choice = m._resolve_choice(None)
    specs = [OptimSpec.of(optim=OptimSpec.from_optimizer(_opt(m, r))) for r in (False, True)]
    assert specs[0] != specs[1] and specs[0]._replace(table_kind="rowwise_adagrad") == specs[1]
    plans = [eng.compile(choice, 16, train=True, clip=5.0, graph=False, spec=s) for s in specs]
    assert plans[0] is not plans[1] and eng.compile(choice, 16, train=True, clip=5.0, graph=False, spec=specs[1]) is plans[1]
    assert eng.table_state is not None and eng.table_row_state is not None  # (each plan's own state, side by side)
    assert eng.table_state[0].data_ptr() != eng.table_row_state[0].data_ptr()
    del m
    import test_split_optimizer_gpu as SP
    (pa, _, _, _), (pb, _, _, _) = SP._fused_steps(base, batches[:1]), _fused_steps(base, batches[:1])
    for k in pa:  # (the first step from a zero state: 16 accumulators against their mean — the tables differ, the network does not)
        assert torch.equal(pa[k], pb[k]) == (not k.startswith("_embedding.")), k


def test_supernet_sampled_paths():
    """a weight-sharing supernet, any-path sampling, same paths on both routes: parameters off a step's path are neither moved nor
    counted; every path of this search space reaches the stem"""
    base, batches = RS._small()
    base.configure_path_sampling_strategy("any-path")
    pa, sa, stem, _ = _fused_steps(base, batches, sampler=11)
    pb, sb, _ = _torch_steps(base, batches, sampler=11)
    _compare(pa, sa, pb, sb, "row-wise, supernet any-path")
    _sums_are_per_row(sa, pa)
    assert all(stem) and float(sa["_embedding.0.weight"]["step"]) == 4.0
    assert any(float(s["step"]) < 4.0 for n, s in sa.items() if not n.startswith("_embedding."))  # (some parameter sat out a step)


def test_a_path_that_skips_the_stem_neither_moves_nor_counts_the_tables():
    choice = {"micro": [RS.SKIP], "macro": RS.MACRO, "num_blocks": 1, "use_layernorm": 1, "config": "xlarge-zeros"}
    base, batches = RS._small(choice, blocks=1, config="xlarge-zeros")
    pa, sa, stem, m = _fused_steps(base, batches[:3])
    pb, sb, _ = _torch_steps(base, batches[:3])
    assert stem == [False, False, False]
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert not any(n.startswith("_embedding.") for n in sa) and float(sa["_final.weight"]["step"]) == 3.0
    assert all(torch.equal(pa["_embedding.%d.weight" % f], base._embedding[f].weight.detach().cpu()) for f in range(26))
    assert m._engine.table_state is None and not any(bool(t.any()) for t in m._engine.table_row_state)


def test_resume_after_fused_steps(best):
    """3 fused steps, then the model's and the optimizer's state_dict into a fresh model and a fresh optimizer, then 3 more steps on the
    fused route and on the torch route: both end in the same place, and where 6 steps of the torch route end"""
    base, batches = best
    six = batches + batches[:2]
    pm, s0, _, m = _fused_steps(base, six[:3])
    assert set(s0["_final.weight"]) == {"step", "exp_avg", "exp_avg_sq"} and set(s0["_embedding.0.weight"]) == {"step", "sum"}
    _sums_are_per_row(s0, pm)
    msd, osd = copy.deepcopy(m.state_dict()), copy.deepcopy(m.__dict__["_test_opt"].state_dict())
    assert osd["param_groups"][0]["table_rowwise"] is True
    del m
    ends = []
    for fused in (True, False):
        fresh = copy.deepcopy(base)
        fresh.load_state_dict(msd)
        if fused:
            pa, sa, _, _ = _fused_steps(None, six[3:], state=osd, use_model=fresh)
        else:
            pa, sa, _ = _torch_steps(None, six[3:], state=osd, use_model=fresh)
        ends.append((pa, sa))
    (pa, sa), (pb, sb) = ends
    _compare(pa, sa, pb, sb, "row-wise, resume")
    assert all(float(s["step"]) == 6.0 for s in sa.values())
    pc, sc, _ = _torch_steps(base, six)
    _compare(pa, sa, pc, sc, "row-wise, resume against 6 torch steps")
    # an element-wise checkpoint is refused by the row-wise optimizer at the binding too: nothing is reshaped into the row accumulators
    fresh = copy.deepcopy(base)
    opt = _opt(fresh)
    w0 = fresh._embedding[0].weight
    opt.state[w0]["step"], opt.state[w0]["sum"] = torch.tensor(3.0), torch.full_like(w0, 0.25)
    fresh._ensure_engine(batches[0][0])
    with pytest.raises(ValueError, match="row-wise"):
        fresh.engine_bind_optimizer(opt)


def test_with_a_weight_average(best):
    """ema_decay = 0.99 in the fused step against WeightEMA.update() on the torch route: the parameters as without the average, bit for
    bit; the average against the torch route's shadow at the parameters' bars (an average of the parameters is no further apart than they
    are)"""
    base, batches = best
    decay = 0.99
    m = copy.deepcopy(base)
    opt = _opt(m)
    spec = OptimSpec.from_optimizer(opt)
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    ema = WeightEMA(m, decay)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, ema=ema) == spec._replace(ema=decay)
    m.engine_bind_ema(ema)
    for int_x, cat_x, y in batches:
        m.engine_train_step(int_x, cat_x, y, lr=LR, clip=5.0, optim=spec, ema_decay=decay)
    sd = ema.state_dict()  # (flushes)
    m.engine_sync_ema(ema)
    assert ema.num_updates == len(batches)
    torch.cuda.synchronize()
    end = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    plain, _, _, _ = _fused_steps(base, batches)
    assert all(torch.equal(end[n], plain[n]) for n in end)
    _, _, shadow = _torch_steps(base, batches, ema=decay)
    got = {n: s.cpu() for n, s in sd["shadow"].items()}
    F._compare_params(_dense(got), _dense(shadow), TOL["params"], "adam")
    for n in got:
        if n.startswith("_embedding."):
            assert torch.allclose(got[n], shadow[n], rtol=0, atol=TABLE_ATOL), n
            assert not torch.equal(got[n], base.state_dict()[n].cpu())  # (the average moved)
    assert m._engine.table_state is None


def test_with_a_decoupled_weight_decay_that_reaches_the_tables(best, best_torch):
    """decoupled_wd = 0.1 over every 2-D parameter, the tables included, against DecoupledWeightDecay.apply() on the torch route; the
    rows outside the batches rest, owe, and are paid by the flush (state_dict).  The decay touches W only: the row accumulators are the
    torch route's."""
    base, batches = best
    lam = 0.1
    m = copy.deepcopy(base)
    opt = _opt(m)
    dec = DecoupledWeightDecay(m, lam, None)
    spec = OptimSpec.from_optimizer(opt)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, decay=dec) == spec._replace(dwd=lam)
    pa, sa, stem, fm = _fused_steps(None, batches, use_model=m, decoupled_wd=lam)
    assert all(stem) and not fm._engine._decay_dirty and fm._engine.table_state is None
    pb, sb, _ = _torch_steps(base, batches, decay=lam)
    pc = best_torch[0]
    gap = max(float((pb[k] - pc[k]).abs().max()) for k in pb if k.startswith("_embedding."))
    print("decay against no decay on the torch route, tables: %.3e (10 x bar = %.1e)" % (gap, 10 * TABLE_ATOL))
    assert gap >= 10 * TABLE_ATOL  # (the decay shows on the torch route alone, or the comparison shows nothing)
    _compare(pa, sa, pb, sb, "row-wise, decoupled decay")
    _sums_are_per_row(sa, pa)


def test_refusals_keep_their_messages(best):
    base, batches = best
    m = copy.deepcopy(base)
    spec = OptimSpec.from_optimizer(_opt(m))
    m._ensure_engine(batches[0][0])
    int_x, cat_x, y = batches[0]
    with pytest.raises(EngineError, match="EMA"):  # a weight average beside a decay that reaches the tables
        m.engine_train_step(int_x, cat_x, y, lr=LR, optim=spec, ema_decay=0.99, decoupled_wd=0.1)
    with pytest.raises(EngineError, match="no split optimizer"):  # the last-layer step: the fine-tune keeps the torch route
        m._engine.last_layer_step(int_x, cat_x, y, lr=LR, choice=m._resolve_choice(None), optim=OptimSpec.of(optim=spec))
    w0 = m._embedding[0].weight.detach().cpu().clone()
    m.engine_train_step(int_x, cat_x, y, lr=LR, optim=spec)  # (and the plain step still runs)
    torch.cuda.synchronize()
    assert not torch.equal(m._embedding[0].weight.detach().cpu(), w0)
    assert type(_opt(m)) is AdamAdagradTables


# ------------------------------------------------------------------------------------------------------------------------ harness
def test_the_harness_takes_the_fused_route_and_equals_the_torch_route(tmp_path, capsys):
    """main_train's arguments with --table-rowwise: Criteo best-1shot at full table size, batch 8, 5 steps, wd 0"""
    args = MT.build_parser().parse_args([
        "--root_dir", F._shards(tmp_path), "--net", "supernet-config", "--supernet_config", F.CFG, "--learning_rate", str(LR),
        "--train_batch_size", "8", "--test_batch_size", "16", "--wd", "0.0", "--logging_dir", str(tmp_path / "l"), "--gpu", "0",
        "--optimizer", NAME, "--table-lr-scale", str(SCALE), "--table-rowwise", "--train_limit", "48"])
    assert args.table_rowwise is True and args.table_lr_scale == SCALE and args.table_eps == 1e-2
    base = F._base(args)
    build = lambda m: MT.build_optimizer(NAME, m, args.learning_rate, args.table_lr_scale, args.table_eps, table_rowwise=args.table_rowwise)  # noqa: E731
    assert TU._fused_step_applies(base, build(base), TU.L2Loss(0.0, None, gpu=0), False) is True
    res = []
    for use in (None, False):
        m = copy.deepcopy(base)
        res.append(RS._run(m, build(m), args, use, 5))
        if use is None:
            assert m._engine.table_state is None and sum(t.numel() for t in m._engine.table_row_state) == sum(m._num_embeddings)
        del m
    out = capsys.readouterr().out
    assert "row-wise Adagrad on the tables" in out and "fused step, exactly row-sparse table update" in out
    assert "torch route, AdamAdagradTables.step()" in out
    (la, pa, sa, na), (lb, pb, sb, nb) = res
    assert na == 5 and nb == 0
    assert la["iters"] == lb["iters"] == [0, 1, 2, 3, 4]
    assert np.allclose(la["train_loss"], lb["train_loss"], rtol=1e-5, atol=1e-6), (la["train_loss"], lb["train_loss"])
    with capsys.disabled():
        _compare(pa, sa, pb, sb, "row-wise, best-1shot harness")
    _sums_are_per_row(sa, pa)
    assert all(float(s["step"]) == 5.0 for s in sa.values()) and "_embedding.2.weight" in sa
    ids = RS._ids(args, 5)
    for f in (0, 2, 25):
        k = "_embedding.%d.weight" % f
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        t0 = base._embedding[f].weight.detach().cpu()
        for p, s in ((pa, sa), (pb, sb)):
            assert torch.equal(p[k][rest], t0[rest]) and not torch.equal(p[k][~rest], t0[~rest])
            assert not s[k]["sum"][rest].any() and s[k]["sum"][~rest].any()
