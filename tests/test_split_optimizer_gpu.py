"""`--optimizer adam-adagrad-tables` (utils/optim.AdamAdagradTables: Adam on the network, Adagrad on the tables at lr * table_lr_scale) in
the fused engine step, on the GPU.  Helpers from test_fused_optimizers_gpu.py and test_row_sparse_adam_gpu.py.

Harness loop (Criteo best-1shot at full table size, batch 8, 5 steps, Adam lr 1e-3, --table-lr-scale 50: the tables run at 0.05, the rate
test_weight_decay_gpu.py uses for Adagrad): the fused route against the torch route.  Bars: losses rtol 1e-5 / atol 1e-6; dense parameters
and moments F.TOL["adam"] with its `_key_bias_noise` exclusion; tables atol 2e-5 and `sum` rtol 1e-4 / atol 1e-9 (the Adagrad bars of
test_weight_decay_gpu.py); step counts equal; rows outside the batches' ids bit-identical to the start on both routes with a zero `sum`.

Small network (`_small`: tables of at most 997 rows, 4 batches of 16): graph replay equals launching; a supernet under any-path sampling;
a path that leaves the stem out; resume; no table moment arrays in the engine; two table_lr_scale values are two plans.  One case each
with a weight average and a decoupled weight decay that reaches the tables, against the torch route."""
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

pytestmark = pytest.mark.gpu
NAME, LR, SCALE, TOL, NO_REG = "adam-adagrad-tables", 1e-3, 50.0, F.TOL["adam"], "_embedding"
TABLE_ATOL, SUM_RTOL, SUM_ATOL = 2e-5, 1e-4, 1e-9


def _args(tmp_path, wd):
    extra = ["--no-reg-param-name", NO_REG] if wd else []
    return MT.build_parser().parse_args([
        "--root_dir", F._shards(tmp_path), "--net", "supernet-config", "--supernet_config", F.CFG, "--learning_rate", str(LR),
        "--train_batch_size", "8", "--test_batch_size", "16", "--wd", str(wd), "--logging_dir", str(tmp_path / "l"), "--gpu", "0",
        "--optimizer", NAME, "--table-lr-scale", str(SCALE), "--train_limit", "48"] + extra)


def _opt(m, scale=SCALE):
    return MT.build_optimizer(NAME, m, LR, scale)


def _dense(d):
    return {k: v for k, v in d.items() if not k.startswith("_embedding.")}


def _compare(pa, sa, pb, sb, what=""):
    """the two routes' parameters and optimizer state: the dense half at Adam's bars, the tables at Adagrad's; prints the figures"""
    F._compare_params(_dense(pa), _dense(pb), TOL["params"], "adam")
    F._compare_state(_dense(sa), _dense(sb), TOL)
    tabs = [k for k in pa if k.startswith("_embedding.")]
    perr = max(float((pa[k] - pb[k]).abs().max()) for k in tabs)
    print("%s: tables max |dW| %.3e (bar %.1e)" % (what, perr, TABLE_ATOL))
    for k in tabs:
        assert torch.allclose(pa[k], pb[k], rtol=0, atol=TABLE_ATOL), (k, float((pa[k] - pb[k]).abs().max()))
    assert {k for k in sa if k.startswith("_embedding.")} == {k for k in sb if k.startswith("_embedding.")}
    for k in sa:
        if k.startswith("_embedding."):
            assert set(sa[k]) == set(sb[k]) == {"step", "sum"}, (k, sorted(sa[k]), sorted(sb[k]))
            assert float(sa[k]["step"]) == float(sb[k]["step"]), k
            assert torch.allclose(sa[k]["sum"], sb[k]["sum"], rtol=SUM_RTOL, atol=SUM_ATOL), (k, float((sa[k]["sum"] - sb[k]["sum"]).abs().max()))


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_fused_step_equals_the_torch_route(tmp_path, capsys, wd):
    args = _args(tmp_path, wd)
    assert args.table_lr_scale == SCALE and args.table_eps == 1e-2
    base = F._base(args)
    l2 = TU.L2Loss(wd, args.no_reg_param_name, gpu=0)
    assert TU._fused_step_applies(base, _opt(base), l2, False) is True
    res = []
    for use in (None, False):
        m = copy.deepcopy(base)
        res.append(RS._run(m, MT.build_optimizer(NAME, m, args.learning_rate, args.table_lr_scale, args.table_eps), args, use, 5))
        del m
    out = capsys.readouterr().out
    assert "fused step, exactly row-sparse table update" in out and "torch route, AdamAdagradTables.step()" in out
    (la, pa, sa, na), (lb, pb, sb, nb) = res
    assert na == 5 and nb == 0
    assert la["iters"] == lb["iters"] == [0, 1, 2, 3, 4]
    assert np.allclose(la["train_loss"], lb["train_loss"], rtol=1e-5, atol=1e-6), (la["train_loss"], lb["train_loss"])
    with capsys.disabled():
        _compare(pa, sa, pb, sb, "best-1shot, wd %g" % wd)
    assert all(float(s["step"]) == 5.0 for s in sa.values()) and "_embedding.2.weight" in sa
    assert set(sa["_final.weight"]) == {"step", "exp_avg", "exp_avg_sq"}
    # only the batches' rows moved, on both routes: bit for bit everywhere else, with nothing accumulated there
    ids = RS._ids(args, 5)
    for f in (0, 2, 25):
        k = "_embedding.%d.weight" % f
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        t0 = base._embedding[f].weight.detach().cpu()
        for p, s in ((pa, sa), (pb, sb)):
            assert torch.equal(p[k][rest], t0[rest]) and not torch.equal(p[k][~rest], t0[~rest])
            assert not s[k]["sum"][rest].any() and s[k]["sum"][~rest].any()


# ------------------------------------------------------------------------------------------------------------------ small network
def _fused_steps(base, batches, wd=0.0, graph=None, sampler=None, scale=SCALE, state=None, use_model=None, **step_kw):
    """engine_train_step over `batches` on a copy of `base` -> (parameters, optimizer state, did each step's backward reach the stem, model)"""
    m = copy.deepcopy(base) if use_model is None else use_model
    opt = _opt(m, scale)
    if state is not None:
        opt.load_state_dict(copy.deepcopy(state))
    spec = OptimSpec.from_optimizer(opt)
    assert spec.table_kind == "adagrad" and spec.table_lr_scale == scale
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


def _torch_steps(base, batches, wd=0.0, sampler=None, scale=SCALE, state=None, use_model=None, ema=None, decay=None):
    m = copy.deepcopy(base) if use_model is None else use_model
    opt = _opt(m, scale)
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


@pytest.fixture(scope="module")
def best():
    choice = RS._best_1shot()
    return RS._small(choice, blocks=choice["num_blocks"], config=choice["config"], layernorm=False, seed=3)


@pytest.fixture(scope="module")
def best_torch(best):
    """the torch route on the small fixed network, once"""
    base, batches = best
    return _torch_steps(base, batches)


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


def test_small_network_equals_the_torch_route_and_holds_no_table_moments(best, best_torch):
    base, batches = best
    pa, sa, stem, m = _fused_steps(base, batches)
    pb, sb, _ = best_torch
    assert all(stem)
    _compare(pa, sa, pb, sb, "small best-1shot")
    eng = m._engine
    # the engine's state: Adam's moments over the dense arena only, Adagrad's accumulators on the tables
    assert set(eng.moments) == {"exp_avg", "exp_avg_sq"} and all(tabs == [] for _, tabs in eng.moments.values())
    assert eng.table_state is not None and len(eng.table_state) == 26
    opt = m.__dict__["_test_opt"]
    assert opt.state[m._embedding[3].weight]["sum"].data_ptr() == eng.table_state[3].data_ptr()
    assert opt.state[m._final.weight]["exp_avg"].data_ptr() == eng.moments_view("exp_avg", "_final.weight").data_ptr()
    with pytest.raises(EngineError, match="table_state"):
        eng.moments_view("exp_avg", "_embedding.3.weight")
    # rows outside the batches: the bits they started with, nothing accumulated
    ids = torch.cat([b[1] for b in batches]).cpu()
    for f in range(26):
        k = "_embedding.%d.weight" % f
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        assert torch.equal(pa[k][rest], base._embedding[f].weight.detach().cpu()[rest]) and not sa[k]["sum"][rest].any(), k


def test_two_table_rates_are_two_plans(best):
    base, batches = best
    m = copy.deepcopy(base)
    m._ensure_engine(batches[0][0])
    eng = m._engine
    int_x, cat_x, y = batches[0]
    choice = m._resolve_choice(None)
    specs = [OptimSpec.of(optim=OptimSpec.from_optimizer(_opt(m, s))) for s in (1.0, SCALE)]
    plans = [eng.compile(choice, 16, train=True, clip=5.0, graph=False, spec=s) for s in specs]
    assert plans[0] is not plans[1] and eng.compile(choice, 16, train=True, clip=5.0, graph=False, spec=specs[0]) is plans[0]
    del m
    (pa, _, _, _), (pb, _, _, _) = _fused_steps(base, batches[:1], scale=1.0), _fused_steps(base, batches[:1], scale=SCALE)
    for k in pa:
        assert torch.equal(pa[k], pb[k]) == (not k.startswith("_embedding.")), k


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_supernet_sampled_paths(wd):
    """a weight-sharing supernet, any-path sampling, same paths on both routes: parameters off a step's path are neither moved nor
    counted (the regularised 2-D ones are, with weight decay); every path of this search space reaches the stem"""
    base, batches = RS._small()
    base.configure_path_sampling_strategy("any-path")
    pa, sa, stem, _ = _fused_steps(base, batches, wd, sampler=11)
    pb, sb, _ = _torch_steps(base, batches, wd, sampler=11)
    _compare(pa, sa, pb, sb, "supernet any-path, wd %g" % wd)
    assert all(stem) and float(sa["_embedding.0.weight"]["step"]) == 4.0
    assert any(float(s["step"]) < 4.0 for n, s in sa.items() if not n.startswith("_embedding."))  # (some parameter sat out a step)


def test_a_path_that_skips_the_stem_neither_moves_nor_counts_the_tables():
    """no gradient reaches the tables (test_fused_optimizers_gpu.py's zeros-3d path): torch leaves their grad None, and the fused step
    neither moves them nor counts a step nor creates state for them"""
    choice = {"micro": [RS.SKIP], "macro": RS.MACRO, "num_blocks": 1, "use_layernorm": 1, "config": "xlarge-zeros"}
    base, batches = RS._small(choice, blocks=1, config="xlarge-zeros")
    pa, sa, stem, m = _fused_steps(base, batches[:3])
    pb, sb, _ = _torch_steps(base, batches[:3])
    assert stem == [False, False, False]
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert not any(n.startswith("_embedding.") for n in sa) and float(sa["_final.weight"]["step"]) == 3.0
    assert all(torch.equal(pa["_embedding.%d.weight" % f], base._embedding[f].weight.detach().cpu()) for f in range(26))
    assert not any(bool(t.any()) for t in m._engine.table_state)


def test_resume_after_fused_steps(best):
    """3 fused steps, then the model's and the optimizer's state_dict into a fresh model and a fresh optimizer, then 3 more steps on the
    fused route and on the torch route: both end in the same place, and where 6 steps of the torch route end"""
    base, batches = best
    six = batches + batches[:2]
    _, s0, _, m = _fused_steps(base, six[:3])
    assert set(s0["_final.weight"]) == {"step", "exp_avg", "exp_avg_sq"} and set(s0["_embedding.0.weight"]) == {"step", "sum"}
    msd, osd = copy.deepcopy(m.state_dict()), copy.deepcopy(m.__dict__["_test_opt"].state_dict())
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
    _compare(pa, sa, pb, sb, "resume")
    assert all(float(s["step"]) == 6.0 for s in sa.values())
    pc, sc, _ = _torch_steps(base, six)
    _compare(pa, sa, pc, sc, "resume against 6 torch steps")


# -------------------------------------------------------------------------------------------------------------------- composition
def test_with_a_weight_average(best):
    """ema_decay = 0.99 in the fused step against WeightEMA.update() on the torch route: the parameters as without the average, bit for
    bit; the average against the fp64 average of the run's own snapshots at test_weight_ema_gpu.py's bar (6 T + 2) 2^-24 M, and
    against the torch route's shadow at the parameters' bars (an average of the parameters is no further apart than they are)"""
    from test_weight_ema_cpu import dense_ema_fp64, ema_bar
    base, batches = best
    decay, T = 0.99, len(batches)
    m = copy.deepcopy(base)
    opt = _opt(m)
    spec = OptimSpec.from_optimizer(opt)
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    ema = WeightEMA(m, decay)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, ema=ema) == spec._replace(ema=decay)
    m.engine_bind_ema(ema)

    def params():
        torch.cuda.synchronize()
        return {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    snaps = [params()]
    for int_x, cat_x, y in batches:
        m.engine_train_step(int_x, cat_x, y, lr=LR, clip=5.0, optim=spec, ema_decay=decay)
        snaps.append(params())
    sd = ema.state_dict()  # (flushes)
    m.engine_sync_ema(ema)
    assert ema.num_updates == T
    worst = 0.0
    for n, s in sd["shadow"].items():
        want, M = dense_ema_fp64([sn[n].double().numpy() for sn in snaps[1:]], snaps[0][n].double().numpy(), decay)
        err = np.abs(s.cpu().double().numpy() - want)
        worst = max(worst, float((err / np.maximum(ema_bar(T, M), 1e-300)).max()) if err.size else 0.0)
    print("split optimizer + EMA: largest |s - s_fp64| as a fraction of the bar: %.3f" % worst)
    assert worst <= 1.0
    plain, _, _, _ = _fused_steps(base, batches)
    assert all(torch.equal(snaps[-1][n], plain[n]) for n in snaps[-1])
    _, _, shadow = _torch_steps(base, batches, ema=decay)
    got = {n: s.cpu() for n, s in sd["shadow"].items()}
    F._compare_params(_dense(got), _dense(shadow), TOL["params"], "adam")
    for n in got:
        if n.startswith("_embedding."):
            assert torch.allclose(got[n], shadow[n], rtol=0, atol=TABLE_ATOL), n


def test_with_a_decoupled_weight_decay_that_reaches_the_tables(best, best_torch):
    """decoupled_wd = 0.1 over every 2-D parameter, the tables included, against DecoupledWeightDecay.apply() on the torch route; the
    rows outside the batches rest, owe, and are paid by the flush (state_dict)"""
    base, batches = best
    lam = 0.1
    m = copy.deepcopy(base)
    opt = _opt(m)
    dec = DecoupledWeightDecay(m, lam, None)
    spec = OptimSpec.from_optimizer(opt)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, decay=dec) == spec._replace(dwd=lam)
    pa, sa, stem, fm = _fused_steps(None, batches, use_model=m, decoupled_wd=lam)
    assert all(stem) and not fm._engine._decay_dirty
    pb, sb, _ = _torch_steps(base, batches, decay=lam)
    pc = best_torch[0]
    gap = max(float((pb[k] - pc[k]).abs().max()) for k in pb if k.startswith("_embedding."))
    print("decay against no decay on the torch route, tables: %.3e (10 x bar = %.1e)" % (gap, 10 * TABLE_ATOL))
    assert gap >= 10 * TABLE_ATOL  # (the decay shows on the torch route alone, or the comparison shows nothing)
    _compare(pa, sa, pb, sb, "decoupled decay")


def test_combinations_the_fused_step_cannot_keep_are_refused(best):
    base, batches = best
    m = copy.deepcopy(base)
    spec = OptimSpec.from_optimizer(_opt(m))
    m._ensure_engine(batches[0][0])
    int_x, cat_x, y = batches[0]
    with pytest.raises(EngineError, match="EMA"):  # a weight average beside a decay that reaches the tables
        m.engine_train_step(int_x, cat_x, y, lr=LR, optim=spec, ema_decay=0.99, decoupled_wd=0.1)
    w0 = m._embedding[0].weight.detach().cpu().clone()
    m.engine_train_step(int_x, cat_x, y, lr=LR, optim=spec)  # (and the plain step still runs)
    torch.cuda.synchronize()
    assert not torch.equal(m._embedding[0].weight.detach().cpu(), w0)
    assert type(_opt(m)) is AdamAdagradTables
