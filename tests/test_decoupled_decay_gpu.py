"""`--decoupled-wd LAMBDA` (utils/optim.DecoupledWeightDecay) in the fused engine step, on the GPU, with test_rmsprop_gpu.py's set-up: the
bench cfg-2 network over tables capped at 997 rows, 6 steps of 8 samples, a learning rate that changes every step.  With Adagrad,
row-sparse Adam and RMSprop the fused step with `decoupled_wd=` lands where the torch route (`apply(lr)` + `optimizer.step()` on the
engine's gradients) lands, under the bars of test_fused_optimizers_gpu.py; the rows in no batch keep their bits until the flush and
then hold their initial value times the product of the factors, within the derived bar of test_decoupled_decay_cpu.py.  lambda = 0 is
the run without the argument, bit for bit; graph replay equals launching; a supernet step that skips the stem moves no table level and
decays no unreached parameter; the evaluation forward and state_dict flush by themselves; `main_train.py --decoupled-wd` on both routes.

lambda per optimizer: lr * lambda = 5e-3, so that six steps take 3 % off a table weight — on the torch route alone that is far more
than 10 x the parameter bar (asserted), else fused-against-torch would show nothing.

Bars: F.TOL["adam"] for row-sparse Adam, test_rmsprop_gpu.py's TOL (the same numbers) for RMSprop; Adagrad's step is linear in g
like SGD's and takes F.TOL["sgd"]["params"], its `sum` the second-moment bar 1e-4 of its largest entry.

Measured on an MI355X, fused against the torch route: parameters 1.2e-7 (Adagrad, bar 2e-5), 5.1e-7 (row-sparse Adam, bar 5e-5),
1.5e-7 (RMSprop, bar 5e-5), 6.0e-8 (supernet, stem skipped in step 2); decay against no decay on the torch route 1.9e-2 on the tables;
the resting rows after the flush 0.05 of the derived bar."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import test_fused_optimizers_gpu as F
import test_rmsprop_gpu as R
import test_row_sparse_adam_gpu as RS
from nasrec_amd import main_train as MT
from nasrec_amd._lib import EngineError
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import DecoupledWeightDecay
from test_decoupled_decay_cpu import decay_bar

pytestmark = pytest.mark.gpu
NAMES = ["adagrad", "row-sparse-adam", "rmsprop"]
LR = {"adagrad": 1e-2, "row-sparse-adam": 1e-3, "rmsprop": 1e-4}
LAM = {"adagrad": 0.5, "row-sparse-adam": 5.0, "rmsprop": 50.0}
TOL = {"adagrad": dict(params=F.TOL["sgd"]["params"], sum=1e-4), "row-sparse-adam": F.TOL["adam"], "rmsprop": R.TOL}
NOISE = {"adagrad": None, "row-sparse-adam": "adam", "rmsprop": "adam"}  # (F._key_bias_noise: Adam's g / (sqrt(v) + eps) structure)


def _lrs(name, T):
    """a learning rate that changes every step, as fp32 values (what the device scalar holds)"""
    return [float(np.float32(LR[name] * (1.0 - 0.1 * t))) for t in range(T)]


def _raw(m):
    """the parameters as they lie in memory: no flush"""
    torch.cuda.synchronize()
    return {n: p.detach().cpu().clone() for n, p in m.named_parameters()}


def _with_paths(m, paths):
    if paths is not None:
        drawn, sample = iter(paths), m._resolve_choice
        m.__dict__["_resolve_choice"] = lambda choices=None: sample(next(drawn) if choices is None else choices)


def _fused(base, batches, name, lam, graph=None, paths=None, no_reg=None, pass_arg=True):
    """engine_train_step(..., decoupled_wd=lam) over `batches` on a copy of `base` -> dict(model, opt, raw = the parameters in memory
    before the first and after every step (no flush), levels = the engine's table levels after every step, stem)"""
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(name, m, LR[name])
    spec = OptimSpec.for_step(opt)
    kw = dict(optim=spec) if spec.moments else dict(eps=spec.eps)
    if pass_arg:
        kw.update(decoupled_wd=lam, no_reg_param_name=no_reg)
    if lam:
        dec = DecoupledWeightDecay(m, lam, no_reg)
        assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, decay=dec) == spec._replace(dwd=lam, no_reg=no_reg)
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    _with_paths(m, paths)
    out = dict(model=m, opt=opt, raw=[_raw(m)], levels=[], stem=[])
    for lr, (int_x, cat_x, y) in zip(_lrs(name, len(batches)), batches):
        m.engine_train_step(int_x, cat_x, y, lr=lr, clip=5.0, graph=graph, **kw)
        out["stem"].append(bool(m._engine._last_plan[2].sparse0.grad_written))
        out["raw"].append(_raw(m))
        lv = getattr(m._engine, "decay_level", None)
        out["levels"].append(lv.cpu().clone() if lv is not None else None)
    out["dirty"] = bool(m._engine._decay_dirty)
    if lam:
        assert int(m._engine._decay_counter.cpu()[0]) == 0 and int(m._engine._row_bitmap().abs().sum()) == 0
    return out


def _finish(run):
    """-> parameters (state_dict: flushes by itself) and optimizer state of a fused run"""
    m, opt = run["model"], run["opt"]
    m.engine_sync_optimizer_steps(opt)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt)


def _torch(base, batches, name, lam, paths=None, no_reg=None):
    """the torch route: the engine's gradients through autograd, clip, touch, apply(lr), optimizer.step() -> parameters, optimizer
    state, and per step the selected parameters that had no gradient"""
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(name, m, LR[name])
    dec = DecoupledWeightDecay(m, lam, no_reg) if lam else None
    no_grad = []
    for k, (lr, (int_x, cat_x, y)) in enumerate(zip(_lrs(name, len(batches)), batches)):
        opt.param_groups[0]["lr"] = lr
        opt.zero_grad()
        out = m(int_x, cat_x, paths[k]) if paths is not None else m(int_x, cat_x)
        torch.nn.functional.binary_cross_entropy_with_logits(out.view(-1), y).backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        if hasattr(opt, "touch"):
            opt.touch(cat_x)
        no_grad.append({n for n, p in m.named_parameters() if p.grad is None and p.dim() >= 2})
        if dec is not None:
            dec.apply(lr)
        opt.step()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt), no_grad


def _compare(name, pa, sa, pb, sb, what):
    perr = max(float((F._key_bias_noise(k, pa[k], NOISE[name]) - F._key_bias_noise(k, pb[k], NOISE[name])).abs().max()) for k in pa)
    print("%s: max |dp| %.3e (bar %.1e)" % (what, perr, TOL[name]["params"]))
    F._compare_params(pa, pb, TOL[name]["params"], NOISE[name])
    if name == "adagrad":  # (a bound Adagrad keeps `sum` for every parameter, torch for those that had a gradient)
        assert set(sb) <= set(sa)
        for n in sb:
            scale = float(sb[n]["sum"].abs().max()) or 1.0
            assert float((sa[n]["sum"] - sb[n]["sum"]).abs().max()) <= TOL[name]["sum"] * scale, n
    else:
        F._compare_state(sa, sb, TOL[name])


@pytest.fixture(scope="module")
def cfg2():
    return R._cfg2()


@pytest.fixture(scope="module")
def fused_runs(cfg2):
    base, batches = cfg2
    return {name: _fused(base, batches, name, LAM[name]) for name in NAMES}


def _resting(batches, f, rows):
    ids = torch.cat([b[1] for b in batches]).cpu()
    rest = torch.ones(rows, dtype=torch.bool)
    rest[ids[:, f]] = False
    return rest


@pytest.mark.parametrize("name", NAMES)
def test_rows_that_rest_keep_their_bits_until_the_flush_and_then_hold_the_product(cfg2, fused_runs, name):
    base, batches = cfg2
    run, T = fused_runs[name], len(batches)
    m = run["model"]
    assert all(run["stem"])
    level = sum(math.log1p(-lr * LAM[name]) for lr in _lrs(name, T))
    got = run["levels"][-1].numpy()
    assert np.abs(got - level).max() <= 1e-15 and run["dirty"]
    factor = float(np.prod([1.0 - lr * LAM[name] for lr in _lrs(name, T)]))
    before = run["raw"][-1]
    m.engine_flush_decay()
    after = _raw(m)
    assert not m._engine._decay_dirty and not m._engine.decay_level.cpu().any() and not any(bool(s.cpu().any()) for s in m._engine.decay_stamps)
    worst, some = 0.0, 0
    for f in (0, 2, 9, 25):
        k = "_embedding.%d.weight" % f
        w0 = base._embedding[f].weight.detach().cpu()
        rest = _resting(batches, f, w0.shape[0])
        some += int(rest.sum())
        assert torch.equal(before[k][rest], w0[rest]), k                     # in no batch: the initial bits, the decay still owed
        err = np.abs(after[k][rest].double().numpy() - w0[rest].double().numpy() * factor)
        bar = decay_bar(T, np.abs(w0[rest].double().numpy()))
        assert (err <= bar).all(), (k, float((err / bar).max()))
        if err.size:
            worst = max(worst, float((err / bar).max()))
            assert not torch.equal(after[k][rest], w0[rest]), k              # (... and it was paid)
    assert some > 0
    print("%s: resting rows, largest error as a fraction of the bar: %.3f" % (name, worst))
    m.engine_flush_decay()  # (nothing owed: nothing launched, no bit changes)
    assert all(torch.equal(a, b) for a, b in zip(after.values(), _raw(m).values()))


@pytest.mark.parametrize("name", NAMES)
def test_fused_step_equals_the_torch_route(cfg2, fused_runs, name):
    base, batches = cfg2
    pa, sa = _finish(fused_runs[name])
    pb, sb, _ = _torch(base, batches, name, LAM[name])
    pc, _, _ = _torch(base, batches, name, 0.0)
    # the decay must show on the torch route alone, or the comparison below shows nothing
    gap = max(float((pb[k] - pc[k]).abs().max()) for k in pb if k.startswith("_embedding."))
    print("%s: decay against no decay on the torch route, tables: %.3e (10 x bar = %.1e)" % (name, gap, 10 * TOL[name]["params"]))
    assert gap >= 10 * TOL[name]["params"]
    _compare(name, pa, sa, pb, sb, "cfg-2, %s, lambda %g" % (name, LAM[name]))


def test_lambda_zero_is_the_run_without_the_argument(cfg2):
    base, batches = cfg2
    a = _fused(base, batches[:4], "adagrad", 0.0)
    b = _fused(base, batches[:4], "adagrad", 0.0, pass_arg=False)
    for x, y in zip(a["raw"], b["raw"]):
        assert all(torch.equal(x[n], y[n]) for n in x)
    eng = a["model"]._engine
    assert getattr(eng, "decay_level", None) is None and not eng._decay_dirty  # (no allocation, no launch)
    assert not torch.equal(a["raw"][-1]["_final.weight"], a["raw"][0]["_final.weight"])


@pytest.mark.parametrize("name", ["adagrad", "rmsprop"])
def test_graph_replay_equals_launch(cfg2, name):
    """the learning rate changes between the replays: it is read from the device scalar"""
    base, batches = cfg2
    a, b = _fused(base, batches[:4], name, LAM[name], graph=False), _fused(base, batches[:4], name, LAM[name], graph=True)
    for x, y in zip(a["raw"], b["raw"]):
        assert all(torch.equal(x[n], y[n]) for n in x)
    assert all(torch.equal(x, y) for x, y in zip(a["levels"], b["levels"]))
    assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a["model"]._engine.decay_stamps, b["model"]._engine.decay_stamps))
    (pa, sa), (pb, sb) = _finish(a), _finish(b)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    assert not torch.equal(pa["_embedding.0.weight"], a["raw"][-1]["_embedding.0.weight"])  # (the flush had something to pay)


def test_a_supernet_step_that_skips_the_stem_moves_no_table_level():
    """test_row_sparse_adam_gpu.py's three paths: the second reaches no table.  torch leaves the tables' grad None there, so they do
    not decay in that step, and neither does a dense parameter off the path; the fused step does the same and ends within the bars"""
    name = "adagrad"
    base, batches = R._net(config="xlarge-zeros", blocks=1, n=3)
    paths = [{"micro": [m], "macro": RS.MACRO} for m in (RS.REACH, RS.SKIP, RS.REACH)]
    run = _fused(base, batches, name, LAM[name], paths=paths)
    assert run["stem"] == [True, False, True]
    lrs = _lrs(name, 3)
    steps = [math.log1p(-lr * LAM[name]) for lr in lrs]
    l1, l2, l3 = (float(lv[0]) for lv in run["levels"])
    assert abs(l1 - steps[0]) <= 1e-15 and l2 == l1 and abs(l3 - (steps[0] + steps[2])) <= 1e-15
    assert all(bool((lv == lv[0]).all()) for lv in run["levels"])
    pb, sb, no_grad = _torch(base, batches, name, LAM[name], paths=paths)
    assert any(n.startswith("_embedding.") for n in no_grad[1]) and not any(n.startswith("_embedding.") for n in no_grad[0])
    off_path = [n for n in no_grad[1] if not n.startswith("_embedding.")]
    assert off_path
    for n in off_path:  # no gradient in step 2: the bits of step 1
        assert torch.equal(run["raw"][2][n], run["raw"][1][n]), n
    # the tables in step 2: no row decays; the rows of its batch that rested through step 1 pay THAT step's factor (the catch-up in
    # front of the gather), the rows of step 1's batch are current and keep their bits, every other row keeps its initial bits
    first, second = batches[0][1].cpu(), batches[1][1].cpu()
    paid = 0
    for f in range(26):
        k = "_embedding.%d.weight" % f
        w0, w1, w2 = (run["raw"][i][k] for i in range(3))
        in1, in2 = torch.zeros(w0.shape[0], dtype=torch.bool), torch.zeros(w0.shape[0], dtype=torch.bool)
        in1[first[:, f]] = True
        in2[second[:, f]] = True
        assert torch.equal(w2[in1], w1[in1]) and torch.equal(w2[~in1 & ~in2], w0[~in1 & ~in2]), k
        late = in2 & ~in1
        err = np.abs(w2[late].double().numpy() - w0[late].double().numpy() * (1.0 - lrs[0] * LAM[name]))
        assert (err <= decay_bar(1, np.abs(w0[late].double().numpy()))).all(), k
        paid += int(late.sum())
    assert paid > 0
    reached = [n for n in run["raw"][0] if n not in no_grad[1] and run["raw"][0][n].dim() >= 2]
    assert reached and all(not torch.equal(run["raw"][2][n], run["raw"][1][n]) for n in reached)
    pa, sa = _finish(run)
    _compare(name, pa, sa, pb, sb, "supernet, stem skipped in step 2")


def test_the_evaluation_forward_and_state_dict_flush_by_themselves(cfg2):
    base, batches = cfg2
    name = "adagrad"
    a, b = _fused(base, batches[:3], name, LAM[name]), _fused(base, batches[:3], name, LAM[name])
    int_x, cat_x, _ = batches[3]
    ma, mb = a["model"], b["model"]
    assert ma._engine._decay_dirty and mb._engine._decay_dirty
    ma.eval()
    with torch.no_grad():
        logits = ma(int_x, cat_x).clone()     # flushes
        assert not ma._engine._decay_dirty
        sd = mb.state_dict()                  # flushes
        assert not mb._engine._decay_dirty
        other = copy.deepcopy(base)
        other.load_state_dict(sd)
        other.eval()
        want = other(int_x, cat_x)
    assert torch.equal(logits, want)
    assert all(torch.equal(sd[n].cpu(), p) for n, p in _raw(ma).items())
    assert not torch.equal(sd["_embedding.0.weight"].cpu(), a["raw"][-1]["_embedding.0.weight"])
    # a torch-route apply() of a bound helper in the middle of a fused run finds every row current
    ma.train()
    ma.engine_train_step(*batches[4], lr=LR[name], clip=5.0, decoupled_wd=LAM[name])
    dec = DecoupledWeightDecay(ma, LAM[name])
    ma.engine_bind_decay(dec)
    assert ma._engine._decay_dirty
    for p in ma.parameters():
        p.grad = torch.zeros_like(p)
    dec.apply(LR[name])
    assert not ma._engine._decay_dirty


def test_combinations_the_fused_step_cannot_keep_are_refused(cfg2):
    base, batches = cfg2
    m = copy.deepcopy(base)
    int_x, cat_x, y = batches[0]
    m._ensure_engine(int_x)
    before = _raw(m)
    with pytest.raises(EngineError):
        m.engine_train_step(int_x, cat_x, y, lr=1e-3, clip=5.0, optim=OptimSpec("adam"), decoupled_wd=0.1)       # dense Adam
    with pytest.raises(EngineError):
        m.engine_train_step(int_x, cat_x, y, lr=1e-2, clip=5.0, ema_decay=0.9, decoupled_wd=0.1)                 # a fused weight EMA
    with pytest.raises(EngineError):
        m.engine_train_step(int_x, cat_x, y, lr=1e-2, clip=5.0, weight_decay=1e-8, decoupled_wd=0.1)             # L2 on the tables
    with pytest.raises(EngineError):
        m.engine_train_step(int_x, cat_x, y, lr=20.0, clip=5.0, decoupled_wd=0.1)                                # lr lambda >= 1
    assert all(torch.equal(a, b) for a, b in zip(before.values(), _raw(m).values()))
    m.engine_train_step(int_x, cat_x, y, lr=1e-2, clip=5.0, ema_decay=0.9, decoupled_wd=0.1, no_reg_param_name="_embedding")
    assert not m._engine._decay_dirty  # (the tables left out: nothing rests)


@pytest.mark.parametrize("optimizer,route", [("adagrad", "fused step"), ("adam", "torch route")])
def test_main_train_runs_with_decoupled_wd(tmp_path, capsys, monkeypatch, optimizer, route):
    monkeypatch.setitem(MT._num_embedding_dict, "criteo-kaggle", [min(n, 997) for n in MT._num_embedding_dict["criteo-kaggle"]])
    logdir = str(tmp_path / "logs")
    args = MT.build_parser().parse_args([
        "--root_dir", "synthetic:steps=6,test_steps=1,seed=3,cap=997", "--net", "supernet-config", "--supernet_config", F.CFG, "--num_epochs", "1",
        "--learning_rate", "1e-3", "--train_batch_size", "8", "--test_batch_size", "16", "--wd", "0", "--logging_dir", logdir, "--gpu", "0",
        "--test_interval", "4", "--display_interval", "2", "--train_limit", "48", "--test_limit", "16", "--optimizer", optimizer,
        "--decoupled-wd", "0.1"])
    torch.manual_seed(0)
    logs = MT.main(args)
    out = capsys.readouterr().out
    assert "Decoupled weight decay (lambda 0.1): %s" % route in out and out.count("Decoupled weight decay") == 1
    assert logs[0]["test_loss"] and all(np.isfinite(v) for v in logs[0]["train_loss"] + logs[0]["test_loss"] + logs[0]["test_AUROC"])
    ck = torch.load(os.path.join(logdir, "supernet-config_checkpoint.pt"), map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict"}  # (the decay has no state)
    assert all(bool(torch.isfinite(v).all()) for v in ck["model_state_dict"].values())
