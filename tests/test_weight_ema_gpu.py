"""`--ema DECAY` (utils/optim.WeightEMA) in the fused engine step, on the GPU, with test_rmsprop_gpu.py's set-up: the bench cfg-2 network
over tables capped at 997 rows, 6 steps of 8 samples, the parameters cloned after every step.  With Adagrad, row-sparse Adam and
RMSprop the flushed average lies within the derived bar of test_weight_ema_cpu.py of the fp64 average of THAT run's parameter
snapshots (the EMA arithmetic alone: no route-against-route noise), and the parameters are bit for bit those of the same run without
an average.  Graph replay equals launching; a supernet step that skips the stem still counts and leaves the tables' rows owing; the
averaged forward equals a second model loaded with the flushed average; `main_train.py --ema 0.9` on both routes."""
import copy
import os

import numpy as np
import pytest
import torch

import test_row_sparse_adam_gpu as RS
import test_rmsprop_gpu as R
from nasrec_amd import main_train as MT
from nasrec_amd._lib import EngineError
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import WeightEMA
from test_weight_ema_cpu import dense_ema_fp64, ema_bar

pytestmark = pytest.mark.gpu
DECAY = 0.9
LR = {"adagrad": 1e-2, "row-sparse-adam": 1e-3, "rmsprop": 1e-4}


def _params(m):
    torch.cuda.synchronize()
    return {n: p.detach().cpu().clone() for n, p in m.named_parameters()}


def _run(base, batches, name="adagrad", decay=DECAY, graph=None, paths=None):
    """engine_train_step over `batches` on a copy of `base` -> dict(model, ema, snaps = the parameters before the first and after every
    step, stem = did each step's backward reach the stem, and — with an average — count, stamps and shadow BEFORE any flush)"""
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(name, m, LR[name])
    spec = OptimSpec.for_step(opt)
    kw = dict(optim=spec) if spec.moments else dict(eps=spec.eps)
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    ema = None
    if decay:
        ema = WeightEMA(m, decay)
        assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, ema=ema) == spec._replace(ema=decay)
        m.engine_bind_ema(ema)
    if paths is not None:
        drawn, sample = iter(paths), m._resolve_choice
        m.__dict__["_resolve_choice"] = lambda choices=None: sample(next(drawn) if choices is None else choices)
    out = dict(model=m, ema=ema, opt=opt, snaps=[_params(m)], stem=[])
    for int_x, cat_x, y in batches:
        m.engine_train_step(int_x, cat_x, y, lr=LR[name], clip=5.0, graph=graph, ema_decay=decay, **kw)
        out["stem"].append(bool(m._engine._last_plan[2].sparse0.grad_written))
        out["snaps"].append(_params(m))
    if ema is not None:
        eng = m._engine
        torch.cuda.synchronize()
        out["count"] = int(eng.ema_count.cpu()[0])
        out["stamps"] = [s.cpu().clone() for s in eng.ema_stamps]
        out["raw"] = {n: s.detach().cpu().clone() for n, s in ema.shadow.items()}
        assert int(eng._ema_counter.cpu()[0]) == 0 and int(eng._row_bitmap().abs().sum()) == 0
    return out


def _check_against_fp64(run, what):
    """the flushed average against the fp64 average of the run's own snapshots -> the largest error as a fraction of the bar"""
    snaps, T = run["snaps"], len(run["snaps"]) - 1
    sd = run["ema"].state_dict()
    worst = 0.0
    for n, s in sd["shadow"].items():
        want, M = dense_ema_fp64([sn[n].double().numpy() for sn in snaps[1:]], snaps[0][n].double().numpy(), DECAY)
        err = np.abs(s.cpu().double().numpy() - want)
        frac = float((err / np.maximum(ema_bar(T, M), 1e-300)).max()) if err.size else 0.0
        worst = max(worst, frac)
    print("%s: largest |s - s_fp64| as a fraction of the bar (6 T + 2) 2^-24 M: %.3f" % (what, worst))
    assert worst <= 1.0, what
    return sd


@pytest.fixture(scope="module")
def cfg2():
    return R._cfg2()


@pytest.mark.parametrize("name", ["adagrad", "row-sparse-adam", "rmsprop"])
def test_fused_average_against_fp64_and_the_parameters_bit_for_bit(cfg2, name):
    base, batches = cfg2
    run = _run(base, batches, name)
    T = len(batches)
    assert all(run["stem"]) and run["count"] == T
    # before the flush: the rows outside the last batches are behind, the last batch's rows are current
    eng = run["model"]._engine
    assert any(int((s < T).sum()) for s in run["stamps"]) and all(int(s.max()) <= T for s in run["stamps"])
    last = batches[-1][1].cpu()
    assert all(bool((run["stamps"][f][last[:, f]] == T).all()) for f in range(26))
    sd = _check_against_fp64(run, "cfg-2, %s" % name)
    assert sd["decay"] == DECAY and all(bool((s == T).all()) for s in eng.ema_stamps)
    run["model"].engine_sync_ema(run["ema"])
    assert run["ema"].num_updates == T
    # the shadow aliases the engine's arrays, and a second state_dict() (a second flush) changes no bit
    assert run["ema"].shadow["_embedding.3.weight"].data_ptr() == eng.ema_tables[3].data_ptr()
    again = run["ema"].state_dict()
    assert all(torch.equal(again["shadow"][n], s) for n, s in sd["shadow"].items())
    # the average only reads the parameters: the same run without it ends on the same bits, step by step
    plain = _run(base, batches, name, decay=0.0)
    for a, b in zip(run["snaps"], plain["snaps"]):
        assert all(torch.equal(a[n], b[n]) for n in a)
    assert not torch.equal(run["snaps"][-1]["_final.weight"], run["snaps"][0]["_final.weight"])


def test_graph_replay_equals_launch(cfg2):
    base, batches = cfg2
    a, b = _run(base, batches[:4], graph=False), _run(base, batches[:4], graph=True)
    assert a["count"] == b["count"] == 4
    assert all(torch.equal(x, y) for x, y in zip(a["stamps"], b["stamps"]))
    assert all(torch.equal(a["raw"][n], b["raw"][n]) for n in a["raw"])
    sa, sb = a["ema"].state_dict(), b["ema"].state_dict()
    assert all(torch.equal(sa["shadow"][n], sb["shadow"][n]) for n in sa["shadow"])
    assert all(torch.equal(x[n], y[n]) for x, y in zip(a["snaps"], b["snaps"]) for n in x)


def test_a_supernet_step_that_skips_the_stem_still_counts_and_the_rows_owe():
    """test_row_sparse_adam_gpu.py's three paths: the second reaches no table, so no leader exists and no row moves; the dense arena
    is averaged whole all the same (the unreached parameters too), the count advances, and the rows of the first batch owe two updates"""
    base, batches = R._net(config="xlarge-zeros", blocks=1, n=3)
    paths = [{"micro": [m], "macro": RS.MACRO} for m in (RS.REACH, RS.SKIP, RS.REACH)]
    run = _run(base, batches, paths=paths)
    assert run["stem"] == [True, False, True] and run["count"] == 3
    first, third = batches[0][1].cpu(), batches[2][1].cpu()
    only_first = [r for r in first[:, 0].tolist() if r not in third[:, 0].tolist()]
    assert only_first and all(int(run["stamps"][0][r]) == 1 for r in only_first)
    assert all(torch.equal(run["snaps"][2][n], run["snaps"][1][n]) for n in run["snaps"][0] if n.startswith("_embedding."))
    _check_against_fp64(run, "supernet, stem skipped in step 2")
    assert all(bool((s == 3).all()) for s in run["model"]._engine.ema_stamps)


def test_the_averaged_forward_and_the_way_back(cfg2):
    base, batches = cfg2
    run = _run(base, batches[:3])
    m, ema = run["model"], run["ema"]
    int_x, cat_x, y = batches[3]
    sd = ema.state_dict()
    before = _params(m)
    m.eval()
    with torch.no_grad():
        with ema.averaged():
            logits = m(int_x, cat_x).clone()
            inside = _params(m)
            with pytest.raises(EngineError):
                m.engine_train_step(int_x, cat_x, y, lr=1e-2, clip=5.0, ema_decay=DECAY)
            with pytest.raises(RuntimeError):
                ema.update()
        other = copy.deepcopy(base)
        other.load_state_dict(sd["shadow"])
        other.eval()
        want = other(int_x, cat_x)
        plain = m(int_x, cat_x)
    assert all(torch.equal(inside[n], sd["shadow"][n].cpu()) for n in inside)
    assert torch.equal(logits, want) and not torch.equal(logits, plain)
    after = _params(m)
    assert all(torch.equal(after[n], before[n]) for n in before)
    assert all(torch.equal(ema.shadow[n].cpu(), sd["shadow"][n].cpu()) for n in sd["shadow"])
    # and training goes on: a torch-route update in the middle of the fused run flushes, averages densely and advances the engine
    m.train()
    ema.update()
    m.engine_sync_ema(ema)
    assert ema.num_updates == 4 and all(bool((s == 4).all()) for s in m._engine.ema_stamps)
    m.engine_train_step(int_x, cat_x, y, lr=1e-2, clip=5.0, ema_decay=DECAY)
    m.engine_sync_ema(ema)
    assert ema.num_updates == 5


@pytest.mark.parametrize("optimizer,route", [("adagrad", "fused step"), ("adam", "torch route")])
def test_main_train_runs_with_ema(tmp_path, capsys, monkeypatch, optimizer, route):
    monkeypatch.setitem(MT._num_embedding_dict, "criteo-kaggle", [min(n, 997) for n in MT._num_embedding_dict["criteo-kaggle"]])
    logdir = str(tmp_path / "logs")
    args = MT.build_parser().parse_args([
        "--root_dir", "synthetic:steps=6,test_steps=1,seed=3,cap=997", "--net", "supernet-config", "--supernet_config", R.F.CFG, "--num_epochs", "1",
        "--learning_rate", "1e-3", "--train_batch_size", "8", "--test_batch_size", "16", "--wd", "0", "--logging_dir", logdir, "--gpu", "0",
        "--test_interval", "4", "--display_interval", "2", "--train_limit", "48", "--test_limit", "16", "--optimizer", optimizer, "--ema", "0.9"])
    torch.manual_seed(0)
    logs = MT.main(args)
    out = capsys.readouterr().out
    assert "Weight EMA (decay 0.9): %s" % route in out and out.count("Weight EMA") == 1
    assert logs[0]["test_loss"] and all(np.isfinite(v) for v in logs[0]["train_loss"] + logs[0]["test_loss"] + logs[0]["test_AUROC"])
    ck = torch.load(os.path.join(logdir, "supernet-config_checkpoint.pt"), map_location="cpu")
    es = ck["ema_state_dict"]
    assert es["decay"] == 0.9 and es["num_updates"] == 6 and set(es["shadow"]) == set(ck["model_state_dict"])
    assert any(not torch.equal(es["shadow"][n], ck["model_state_dict"][n]) for n in es["shadow"])
