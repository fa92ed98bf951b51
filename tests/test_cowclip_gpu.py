"""CowClip (`--cowclip R[,ZETA]`, utils/optim.CowClip) in the fused engine step, on the GPU: engine_train_step(..., cowclip=(r, zeta))
against the torch route with CowClip.apply() between clip_grad_norm_ and optimizer.step(), three steps on the small fixed network of
test_split_optimizer_gpu.py / test_row_sparse_adam_gpu.py (Criteo best-1shot over tables of at most 997 rows).

Cases: B = 8 launched; B = 256 (the level-scheduled program) launched and as a graph; B = 300; B = 2304 (above DEDUP_SPLIT_MAX_B: the
one-launch dedup with its contiguous gsum); --optimizer adagrad, adam-adagrad-tables (element-wise and --table-rowwise) and
row-sparse-adam; one case with a weight average and a decoupled weight decay both on.

Bars: the ones the same comparison has without CowClip.  Adagrad: parameters atol 2e-5, `sum` rtol 1e-4 / atol 1e-9
(test_weight_decay_gpu.py).  adam-adagrad-tables: test_split_optimizer_gpu._compare (the dense half F.TOL["adam"], tables atol 2e-5, `sum`
rtol 1e-4 / atol 1e-9).  row-sparse-adam: F.TOL["adam"] on parameters and moments (test_row_sparse_adam_gpu.py).

r of each case sits near the median of the rows' own flip points G / (cnt ||w||) under the Python definition (measured once per case
on the torch route), so that in every step between 10 % and 90 % of the touched rows are clipped: asserted.

`row-sparse-adam-B2304` runs at lr 1e-4, not the 1e-3 of the other Adam cases.  At B = 2304 the torch route is not reproducible from
run to run (its backward gives row gradients that differ by up to 4.5e-7 of a row's size between two calls on the same weights; the
fused route repeats bit for bit), and at 1e-3 the trajectory multiplies such differences: Adam's first step moves every weight by
the full lr, the global norm goes from 1.0 to 15.8, and weights 1e-7 apart give step-2 row gradients 3.6e-5 apart.  Against
the fused step's result, which repeats bit for bit, one run of the torch route then ends 1.4e-4 of the largest `exp_avg` away and
the next run 1.6e-3 (F.TOL's bar: 1e-4): the reference moves by more than the bar, so nothing could be held to it there.  On equal weights the routes' step-2 rows agree to 5.8e-7 of a row's size, and each agrees with the fp64 sum of the same
per-sample rows to 6.3e-7: the one-launch dedup's gsum, the counts and the clip are not what differed."""
import copy

import pytest
import torch

import test_fused_optimizers_gpu as F
import test_rmsprop_gpu as RM
import test_row_sparse_adam_gpu as RS
import test_split_optimizer_gpu as SO
from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd._lib import EngineError
from nasrec_amd.engine import DEDUP_SPLIT_MAX_B
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import CowClip, DecoupledWeightDecay, WeightEMA

pytestmark = pytest.mark.gpu
LR = {"adagrad": 0.05, "adam-adagrad-tables": 1e-3, "row-sparse-adam": 1e-3, "rmsprop": RM.LR, "adam": F.LR["adam"], "sgd": F.LR["sgd"]}
SCALE, ZETA, STEPS = 50.0, 1e-5, 3
TABLES = [min(n, 997) for n in MT._num_embedding_dict["criteo-kaggle"]][:26]

# name: (optimizer, --table-rowwise, B, graph, r)
CASES = {
    "adagrad-B8": ("adagrad", False, 8, False, 0.05),
    "adagrad-B256-launched": ("adagrad", False, 256, False, 0.002),
    "adagrad-B256-graph": ("adagrad", False, 256, True, 0.002),
    "split-B300": ("adam-adagrad-tables", False, 300, False, 0.0025),
    "split-rowwise-B256": ("adam-adagrad-tables", True, 256, False, 0.0035),
    "row-sparse-adam-B300": ("row-sparse-adam", False, 300, False, 0.0025),
    "adagrad-B2304": ("adagrad", False, 2304, False, 0.0002),
    "row-sparse-adam-B2304": ("row-sparse-adam", False, 2304, False, 0.0002),
    # the optimizers whose tables take no rule of their own: lazily decayed RMSprop rows, and dense Adam / SGD, which move every row
    "rmsprop-B16": ("rmsprop", False, 16, False, 0.03),
    "adam-B16": ("adam", False, 16, False, 0.03),
    "sgd-B16": ("sgd", False, 16, False, 0.03),
}
LR_OF_CASE = {"row-sparse-adam-B2304": 1e-4}  # (the docstring says why)
EMA_DECAY_CASE = ("adagrad", False, 16, False, 0.015)  # (with ema_decay 0.9 and decoupled_wd 0.1 on the dense parameters)


def _batches(B, steps=STEPS):
    g = torch.Generator().manual_seed(100 + B)
    return [(torch.randn(B, 13, generator=g).abs().to(0), torch.stack([torch.randint(0, n, (B,), generator=g) for n in TABLES], 1).to(0),
             torch.randint(0, 2, (B,), generator=g).float().to(0)) for _ in range(steps)]


@pytest.fixture(scope="module")
def base():
    choice = RS._best_1shot()
    return RS._small(choice, blocks=choice["num_blocks"], config=choice["config"], layernorm=False, seed=3)[0]


def _opt(name, m, rowwise=False, lr=None):
    return MT.build_optimizer(name, m, lr or LR[name], SCALE, table_rowwise=rowwise)


def _params(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _torch_steps(base, batches, name, rowwise, cow, ema=0.0, decay=0.0, no_reg=None, lr=None):
    """the torch route -> (parameters, optimizer state, [(touched, clipped)] per step, the average's shadow or None)"""
    m = copy.deepcopy(base)
    lr = lr or LR[name]
    opt = _opt(name, m, rowwise, lr)
    cc = CowClip(list(m._embedding.parameters()), *cow) if cow is not None else None
    avg = WeightEMA(m, ema) if ema else None
    dec = DecoupledWeightDecay(m, decay, no_reg) if decay else None
    shares = []
    for int_x, cat_x, y in batches:
        opt.zero_grad()
        torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x).view(-1), y).backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        if hasattr(opt, "touch"):
            opt.touch(cat_x)
        if dec is not None:
            dec.apply(lr)
        if cc is not None:
            shares.append(cc.apply(cat_x))
        opt.step()
        if avg is not None:
            avg.update()
    torch.cuda.synchronize()
    shadow = {n: s.detach().cpu().clone() for n, s in avg.shadow.items()} if avg is not None else None
    return _params(m), F._state(m, opt), shares, shadow


def _fused_steps(base, batches, name, rowwise, cow, graph=False, use_model=None, avg=None, lr=None, **step_kw):
    """engine_train_step(..., cowclip=cow) -> (parameters, optimizer state, the model)"""
    m = copy.deepcopy(base) if use_model is None else use_model
    lr = lr or LR[name]
    opt = _opt(name, m, rowwise, lr)
    kw = dict(eps=1e-2) if name == "adagrad" else dict(optim=OptimSpec.from_optimizer(opt))
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    if avg is not None:
        m.engine_bind_ema(avg)
    for int_x, cat_x, y in batches:
        m.engine_train_step(int_x, cat_x, y, lr=lr, clip=5.0, graph=graph, cowclip=cow, **kw, **step_kw)
    m.engine_sync_optimizer_steps(opt)
    torch.cuda.synchronize()
    opt.state_dict()  # (LazyRMSprop: brings every row's square_avg current)
    m.__dict__["_test_opt"] = opt
    return _params(m), F._state(m, opt), m


def _compare(name, pa, sa, pb, sb, what):
    if name == "adagrad":
        err = max(float((pa[k] - pb[k]).abs().max()) for k in pa)
        print("%s: max |dW| %.3e (bar 2e-5)" % (what, err))
        for k in pa:
            assert torch.allclose(pa[k], pb[k], rtol=0, atol=2e-5), (k, float((pa[k] - pb[k]).abs().max()))
        assert set(sa) == set(sb)
        for k in sa:
            assert torch.allclose(sa[k]["sum"], sb[k]["sum"], rtol=1e-4, atol=1e-9), (k, float((sa[k]["sum"] - sb[k]["sum"]).abs().max()))
    elif name == "adam-adagrad-tables":
        SO._compare(pa, sa, pb, sb, what)
    elif name == "rmsprop":
        F._compare_params(pa, pb, RM.TOL["params"], "adam")
        F._compare_state(sa, sb, RM.TOL)
    elif name == "sgd":
        F._compare_params(pa, pb, F.TOL["sgd"]["params"], "sgd")
        F._compare_state(sa, sb, F.TOL["sgd"])
    else:  # row-sparse Adam and dense Adam
        F._compare_params(pa, pb, F.TOL["adam"]["params"], "adam")
        F._compare_state(sa, sb, F.TOL["adam"])


def _assert_shares(shares, what):
    for t, k in shares:
        print("%s: %d of %d touched rows clipped (%.0f %%)" % (what, k, t, 100.0 * k / t))
        assert t > 0 and 0.10 <= k / t <= 0.90, (what, shares)


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_step_equals_the_torch_route(base, case):
    name, rowwise, B, graph, r = CASES[case]
    assert (B > DEDUP_SPLIT_MAX_B) == ("B2304" in case)
    batches, cow, lr = _batches(B), (r, ZETA), LR_OF_CASE.get(case)
    pb, sb, shares, _ = _torch_steps(base, batches, name, rowwise, cow, lr=lr)
    _assert_shares(shares, case)
    pa, sa, m = _fused_steps(base, batches, name, rowwise, cow, graph=graph, lr=lr)
    _compare(name, pa, sa, pb, sb, case)
    eng = m._engine
    # the engine's counters are the definition's
    assert eng.cowclip_stats() == (sum(t for t, _ in shares), sum(k for _, k in shares)), (eng.cowclip_stats(), shares)
    assert all(int(c.abs().sum()) == 0 for c in eng.cowclip_cnt), "the count scratch must be all zero between steps"
    # the launch list: exactly two more entries than the plan without CowClip, the clip directly in front of the apply stage
    cp = eng._last_plan[2]
    kinds = [d.kind for d in cp.opt.descs]
    spec = cp.tail.spec
    plain = eng.compile(m._resolve_choice(None), B, train=True, clip=5.0, eps=1e-2, graph=graph, spec=spec)
    assert plain is not cp and plain.tail.cowclip is None and cp.tail.cowclip == cow
    plain_kinds = [d.kind for d in plain.opt.descs]
    assert L.OP_COWCLIP not in plain_kinds and [k for k in kinds if k != L.OP_COWCLIP] == plain_kinds and len(kinds) == len(plain_kinds) + 2
    at = [i for i, d in enumerate(cp.opt.descs) if d.kind == L.OP_COWCLIP]
    assert [cp.opt.descs[i].phase for i in at] == [0, 1]
    assert kinds[at[1] + 1] == (L.OP_OPT_APPLY if name == "adagrad" else L.OP_OPT_MOMENTS)


def test_cowclip_changes_the_step(base):
    """the comparison would show nothing if the clip did nothing: against the torch route WITHOUT CowClip the tables are far apart"""
    name, rowwise, B, graph, r = CASES["adagrad-B256-launched"]
    batches = _batches(B)
    pa, _, _, _ = _torch_steps(base, batches, name, rowwise, (r, ZETA))
    pb, _, _, _ = _torch_steps(base, batches, name, rowwise, None)
    gap = max(float((pa[k] - pb[k]).abs().max()) for k in pa if k.startswith("_embedding."))
    print("CowClip against none on the torch route, tables: %.3e (10 x bar = 2e-4)" % gap)
    assert gap >= 2e-4


def test_a_step_without_cowclip_after_one_with_it_is_a_fresh_engines(base):
    """the pair is part of the plan key: cowclip=None after cowclip steps replays no CowClip plan, and other values are another plan"""
    name, rowwise, B, graph, r = CASES["adagrad-B8"]
    batches = _batches(B)
    m = copy.deepcopy(base)
    _fused_steps(None, batches[:1], name, rowwise, (r, ZETA), use_model=m)
    eng = m._engine
    first = eng._last_plan[2]
    t1 = eng.cowclip_stats()[0]
    m.engine_train_step(*batches[1], lr=LR[name], clip=5.0, graph=False, cowclip=(2 * r, ZETA))
    assert eng._last_plan[2] is not first and eng._last_plan[2].tail.cowclip == (2 * r, ZETA)
    t2 = eng.cowclip_stats()[0]
    assert t2 > t1
    # from here on without: two steps on this engine against two steps of a fresh one from the same weights
    torch.cuda.synchronize()
    start = _params(m)  # (parameters only: Adagrad's sums live in the bound optimizer)
    state = copy.deepcopy(m.__dict__["_test_opt"].state_dict())
    for b in batches[1:]:
        m.engine_train_step(*b, lr=LR[name], clip=5.0, graph=False)
    assert eng._last_plan[2].tail.cowclip is None and eng.cowclip_stats()[0] == t2
    fresh = copy.deepcopy(base)
    fresh.load_state_dict(start)
    opt = _opt(name, fresh)
    fresh._ensure_engine(batches[0][0])
    opt.load_state_dict(state)
    fresh.engine_bind_optimizer(opt)
    for b in batches[1:]:
        fresh.engine_train_step(*b, lr=LR[name], clip=5.0, graph=False)
    torch.cuda.synchronize()
    pa, pb = _params(m), _params(fresh)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def test_with_a_weight_average_and_a_decoupled_decay(base):
    name, rowwise, B, graph, r = EMA_DECAY_CASE
    batches, cow = _batches(B), (r, ZETA)
    ema, lam, no_reg = 0.9, 0.1, "_embedding"
    pb, sb, shares, shadow = _torch_steps(base, batches, name, rowwise, cow, ema=ema, decay=lam, no_reg=no_reg)
    _assert_shares(shares, "ema + decoupled decay")
    m = copy.deepcopy(base)
    avg = WeightEMA(m, ema)
    pa, sa, m = _fused_steps(None, batches, name, rowwise, cow, use_model=m, avg=avg, ema_decay=ema, decoupled_wd=lam, no_reg_param_name=no_reg)
    sd = avg.state_dict()
    m.engine_sync_ema(avg)
    _compare(name, pa, sa, pb, sb, "ema + decoupled decay")
    got = {n: s.cpu() for n, s in sd["shadow"].items()}
    for n in got:
        assert torch.allclose(got[n], shadow[n], rtol=0, atol=2e-5), (n, float((got[n] - shadow[n]).abs().max()))
    kinds = [d.kind for d in m._engine._last_plan[2].opt.descs]
    i = max(j for j, k in enumerate(kinds) if k == L.OP_COWCLIP)
    assert kinds[i - 1] == L.OP_DECOUPLED_DECAY and kinds[i + 1] == L.OP_OPT_APPLY  # (behind the decay's launch, in front of the apply stage)


def test_behind_a_decoupled_decay_that_reaches_the_tables(base, capsys):
    """decoupled_wd = 0.1 over every 2-D parameter, the tables included, no average: rows outside a batch rest and owe, the decay's
    launch pays a touched row's debt and decays it, and CowClip then reads those weights — the torch route's order, decay.apply() in
    front of CowClip.apply().  lambda is large so that a threshold from weights that still owed, or were not yet decayed, would show:
    1 - lr lambda = 0.995 per step moves r ||w|| by 5e-3 of itself, far more than the routes differ."""
    name, rowwise, B, graph, r = EMA_DECAY_CASE
    batches, cow, lam = _batches(B), (r, ZETA), 0.1
    pb, sb, shares, _ = _torch_steps(base, batches, name, rowwise, cow, decay=lam)
    _assert_shares(shares, "decay on the tables")
    pa, sa, m = _fused_steps(base, batches, name, rowwise, cow, decoupled_wd=lam)
    _compare(name, pa, sa, pb, sb, "decay on the tables")
    assert m._engine.cowclip_stats() == (sum(t for t, _ in shares), sum(k for _, k in shares))
    kinds = [d.kind for d in m._engine._last_plan[2].opt.descs]
    i = max(j for j, k in enumerate(kinds) if k == L.OP_COWCLIP)
    assert kinds[i - 1] == L.OP_DECOUPLED_DECAY and kinds[i + 1] == L.OP_OPT_APPLY
    # the decay shows: without it the tables end elsewhere
    pc, _, _, _ = _torch_steps(base, batches, name, rowwise, cow)
    gap = max(float((pb[k] - pc[k]).abs().max()) for k in pb if k.startswith("_embedding."))
    assert gap >= 2e-4, gap


def test_refusals_name_cowclip(base):
    batches = _batches(8)
    int_x, cat_x, y = batches[0]
    m = copy.deepcopy(base)
    m._ensure_engine(int_x)
    with pytest.raises(EngineError, match="cowclip"):  # an L2 term that reaches the tables
        m.engine_train_step(int_x, cat_x, y, lr=0.05, clip=5.0, weight_decay=1e-3, cowclip=(1.0, ZETA))
    with pytest.raises(EngineError, match="cowclip"):  # the persistent form
        m._engine.persist = True
        try:
            m.engine_train_step(int_x, cat_x, y, lr=0.05, clip=5.0, cowclip=(1.0, ZETA))
        finally:
            m._engine.persist = False
    with pytest.raises(EngineError, match="cowclip"):  # the data-parallel step's plan
        m._engine.compile(m._resolve_choice(None), 8, train=True, local_optimizer=False, cowclip=(1.0, ZETA))
    w0 = m._embedding[0].weight.detach().cpu().clone()
    m.engine_train_step(int_x, cat_x, y, lr=0.05, clip=5.0, weight_decay=1e-3, no_reg_param_name="_embedding", cowclip=(1.0, ZETA))
    torch.cuda.synchronize()
    assert not torch.equal(m._embedding[0].weight.detach().cpu(), w0)  # (an L2 term on the dense parameters alone goes with it)


def test_the_harness_takes_both_routes(tmp_path, capsys):
    """main_train's loop with --cowclip on the Criteo best-1shot network at full table size, 3 steps of 8 samples: the fused route and
    the torch route print their route line and the share line, and agree on the losses (rtol 1e-5 / atol 1e-6, the harness bar of
    test_split_optimizer_gpu.py) and the tables (atol 2e-5)"""
    args = MT.build_parser().parse_args([
        "--root_dir", F._shards(tmp_path), "--net", "supernet-config", "--supernet_config", F.CFG, "--learning_rate", "0.05",
        "--train_batch_size", "8", "--test_batch_size", "16", "--wd", "0", "--logging_dir", str(tmp_path / "l"), "--gpu", "0",
        "--optimizer", "adagrad", "--train_limit", "48", "--cowclip", "0.5"])
    assert args.cowclip == (0.5, 1e-5)
    MT.check_cowclip(args)
    start = F._base(args)
    from nasrec_amd.utils.data_pipes import make_loaders
    res = []
    for use in (None, False):
        m = copy.deepcopy(start)
        opt = MT.build_optimizer("adagrad", m, args.learning_rate)
        cow = MT.build_cowclip(args, m)
        train_loader, test_loader = make_loaders(args)
        sched = MT.build_lr_scheduler("constant", opt, 3, 2, args.learning_rate)
        capsys.readouterr()
        logs = TU.train_and_test_one_epoch(m, 0, opt, sched, train_loader, test_loader, torch.nn.BCEWithLogitsLoss(), TU.L2Loss(0.0, None, gpu=0),
                                           8, 0, display_interval=1, test_interval=100, max_train_steps=3, grad_clip_value=5.0,
                                           use_engine_step=use, cowclip=cow)
        torch.cuda.synchronize()
        out = capsys.readouterr().out
        rows = m.engine_cowclip_stats() if use is None else (cow.touched, cow.clipped)
        res.append((logs, _params(m), out, rows, m.__dict__.get("_engine_steps", 0)))
        del m
    (la, pa, oa, ra, na), (lb, pb, ob, rb, nb) = res
    assert na == 3 and nb == 0
    assert "CowClip (r 0.5, zeta 1e-05): fused step" in oa and "CowClip (r 0.5, zeta 1e-05): torch route, CowClip.apply()" in ob
    assert oa.count("touched rows clipped since the last display") == ob.count("touched rows clipped since the last display") == 3
    print("rows touched / clipped: fused %s, torch %s" % (ra, rb))
    assert ra == rb and ra[0] > 0
    assert torch.allclose(torch.tensor(la["train_loss"]), torch.tensor(lb["train_loss"]), rtol=1e-5, atol=1e-6), (la["train_loss"], lb["train_loss"])
    for k in pa:
        assert torch.allclose(pa[k], pb[k], rtol=0, atol=2e-5), (k, float((pa[k] - pb[k]).abs().max()))
