"""`--optimizer rmsprop` (utils/optim.LazyRMSprop) in the fused engine step, on the GPU, after test_row_sparse_adam_gpu.py: the bench
cfg-2 network (the Criteo xlarge best-1shot sub-network) over tables capped at 997 rows, 6 steps of 8 samples, lr 1e-4 — RMSprop's
first step is lr / sqrt(1 - alpha) = 10 lr per element, the step size of the Adam tests.  The fused step lands where torch.optim.RMSprop
lands on EVERY row (the rows outside the batches owe only a decay, paid by the flush before anybody reads the state), with and without
weight decay on the dense parameters; the state's keys are torch's; a supernet with sampled paths; a step that skips the stem neither
counts nor decays the tables; graph replay equals launching; a checkpoint after fused steps resumes in a plain torch.optim.RMSprop; and
`--optimizer rmsprop` runs through main_train.main.

Bars: test_fused_optimizers_gpu.py's Adam bars (parameters 0.05 of the Adam tests' lr, the second moment 1e-4 of its largest entry) and
its `_key_bias_noise` exclusion: RMSprop has Adam's g / (sqrt(v) + eps) noise structure.  Measured, fused against the torch route:
parameters 1.0e-6 / 6.8e-7 (cfg-2, wd 0 / wd on the dense parameters), 3.8e-6 (supernet), 6.3e-7 (resume); square_avg 1.5e-5 of its
largest entry and below.  The bars were not widened, and no fp64 floor of the torch route was needed."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import test_fused_optimizers_gpu as F
import test_row_sparse_adam_gpu as RS
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import LazyRMSprop

pytestmark = pytest.mark.gpu
NAME, LR, NO_REG = "rmsprop", 1e-4, "_embedding"
TOL = dict(params=F.TOL["adam"]["params"], square_avg=F.TOL["adam"]["exp_avg_sq"])
CFG2 = os.path.join(F.ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_xlarge_best_1shot.json")
TABLES = [min(n, 997) for n in MT._num_embedding_dict["criteo-kaggle"]][:26]


def _batches(n, B=8, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, 13, generator=g).abs().to(0), torch.stack([torch.randint(0, r, (B,), generator=g) for r in TABLES], 1).to(0),
             torch.randint(0, 2, (B,), generator=g).float().to(0)) for _ in range(n)]


def _net(fixed_choice=None, blocks=3, config="xlarge", layernorm=True, seed=5, n=6):
    batches = _batches(n)
    torch.manual_seed(seed)
    kw = dict(path_sampling_strategy="fixed-path", fixed=True, fixed_choice=fixed_choice) if fixed_choice is not None else \
        dict(path_sampling_strategy="full-path")
    base = SuperNet(num_blocks=blocks, ops_config=ops_config_lib[config], use_layernorm=layernorm, num_embeddings=TABLES, sparse_input_size=26,
                    **kw).to(0)
    with torch.no_grad():
        base(batches[0][0], batches[0][1])
    base.apply(TU.init_weights)
    return base, batches


def _cfg2(seed=5, n=6):
    with open(CFG2) as f:
        choice = json.load(f)
    return _net(choice, blocks=choice["num_blocks"], config=choice["config"], layernorm=False, seed=seed, n=n)


def _snapshot(m, opt):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt)


def _fused(base, batches, wd=0.0, graph=None, sampler=None, state=None, paths=None):
    """engine_train_step over `batches` on a copy of `base` -> parameters, optimizer state (read through state_dict's flush), did each
    step's backward reach the stem, the tables after each step"""
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(NAME, m, LR)
    if state is not None:
        opt.load_state_dict(copy.deepcopy(state))
    spec = OptimSpec.from_optimizer(opt)
    assert TU._fused_step_applies(m, opt, TU.L2Loss(wd, NO_REG if wd else None, gpu=0), False) is True
    if sampler is not None:
        np.random.seed(sampler)
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    if paths is not None:
        drawn, sample = iter(paths), m._resolve_choice
        m.__dict__["_resolve_choice"] = lambda choices=None: sample(next(drawn) if choices is None else choices)
    stem, tables = [], []
    for int_x, cat_x, y in batches:
        m.engine_train_step(int_x, cat_x, y, lr=LR, clip=5.0, graph=graph, weight_decay=wd, no_reg_param_name=NO_REG if wd else None, optim=spec)
        stem.append(bool(m._engine._last_plan[2].sparse0.grad_written))
        torch.cuda.synchronize()
        tables.append(m._embedding[0].weight.detach().cpu().clone())
    m.engine_sync_optimizer_steps(opt)
    torch.cuda.synchronize()
    assert int(m._engine._row_bitmap().abs().sum()) == 0 and int(m._engine._mom_counter[0]) == 0
    sd = copy.deepcopy(opt.state_dict())
    return _snapshot(m, opt) + (stem, tables, sd)


def _torch(base, batches, wd=0.0, sampler=None, state=None, paths=None):
    """the torch route with a plain torch.optim.RMSprop"""
    m = copy.deepcopy(base)
    opt = torch.optim.RMSprop(m.parameters(), lr=LR)
    if state is not None:
        opt.load_state_dict(copy.deepcopy(state))
    if sampler is not None:
        np.random.seed(sampler)
    for k, (int_x, cat_x, y) in enumerate(batches):
        opt.zero_grad()
        out = m(int_x, cat_x, paths[k]) if paths is not None else m(int_x, cat_x)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(out.view(-1), y) + TU.get_l2_loss(m, wd, NO_REG, gpu=0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        opt.step()
    return _snapshot(m, opt)


def _report(pa, pb, sa, sb, what):
    """the figures the bars are compared with, printed before any assertion"""
    perr = max(float((F._key_bias_noise(k, pa[k], "adam") - F._key_bias_noise(k, pb[k], "adam")).abs().max()) for k in pa)
    serr = max(float((sa[n]["square_avg"] - sb[n]["square_avg"]).abs().max()) / (float(sb[n]["square_avg"].abs().max()) or 1.0) for n in sa if n in sb)
    print("%s: max |dp| %.3e (bar %.1e)  max |d square_avg| / max %.3e (bar %.1e)" % (what, perr, TOL["params"], serr, TOL["square_avg"]))


@pytest.mark.parametrize("wd", [0.0, 1e-8], ids=["wd0", "wd-dense-only"])
def test_fused_step_equals_the_torch_route(wd):
    base, batches = _cfg2()
    pa, sa, stem, _, _ = _fused(base, batches, wd)
    pb, sb = _torch(base, batches, wd)
    _report(pa, pb, sa, sb, "cfg-2, wd %g" % wd)
    assert all(stem)
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    # the state's keys are torch's, on every parameter that has state; the stamps stay inside the engine
    assert all(set(s) == {"step", "square_avg"} for s in sa.values()) and all(float(s["step"]) == 6.0 for s in sa.values())
    assert "_embedding.2.weight" in sa
    # rows outside the batches did not move, and their square_avg is torch's: zero gradients leave zero
    ids = torch.cat([b[1] for b in batches]).cpu()
    for f in (0, 2, 25):
        k = "_embedding.%d.weight" % f
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        t0 = base._embedding[f].weight.detach().cpu()
        for p, s in ((pa, sa), (pb, sb)):
            assert torch.equal(p[k][rest], t0[rest]) and not s[k]["square_avg"][rest].any()
        assert not torch.equal(pa[k][~rest], t0[~rest])


def test_supernet_sampled_paths():
    base, batches = _net(n=4)
    base.configure_path_sampling_strategy("any-path")
    pa, sa, stem, _, _ = _fused(base, batches, sampler=11)
    pb, sb = _torch(base, batches, sampler=11)
    _report(pa, pb, sa, sb, "supernet, any-path")
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert all(stem) and float(sa["_embedding.0.weight"]["step"]) == 4.0


def test_a_step_that_skips_the_stem_neither_counts_nor_decays_the_tables():
    """test_row_sparse_adam_gpu.py's three paths: the second reaches no table.  torch leaves their grad None there — no count, no
    decay of square_avg — and so does the fused step: the tables' counter ends at 2, _final's at 3, and a row touched in steps 1 and 3
    decayed once in between, not twice"""
    base, batches = _net(config="xlarge-zeros", blocks=1, n=3)
    paths = [{"micro": [m], "macro": RS.MACRO} for m in (RS.REACH, RS.SKIP, RS.REACH)]
    same = batches[0]
    batches = [same, batches[1], same]  # (steps 1 and 3 touch the same rows)
    pa, sa, stem, tables, _ = _fused(base, batches, paths=paths)
    pb, sb = _torch(base, batches, paths=paths)
    _report(pa, pb, sa, sb, "stem skipped in step 2")
    assert stem == [True, False, True]
    assert not torch.equal(tables[0], base._embedding[0].weight.detach().cpu())
    assert torch.equal(tables[1], tables[0]) and not torch.equal(tables[2], tables[1])
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    for s in (sa, sb):
        assert all(float(s["_embedding.%d.weight" % f]["step"]) == 2.0 for f in range(26)) and float(s["_final.weight"]["step"]) == 3.0


@pytest.mark.parametrize("wd", [0.0, 1e-8], ids=["wd0", "wd-dense-only"])
def test_graph_replay_equals_launch(wd):
    base, batches = _cfg2(seed=3, n=4)
    (pa, sa, _, _, _), (pb, sb, _, _, _) = _fused(base, batches, wd, graph=False), _fused(base, batches, wd, graph=True)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert set(sa) == set(sb)
    for n in sa:
        for k in sa[n]:
            assert torch.equal(torch.as_tensor(sa[n][k]), torch.as_tensor(sb[n][k])), (n, k)


def test_resume_after_fused_steps():
    """three fused steps; the optimizer's state_dict() loads into a fresh plain torch.optim.RMSprop (every row current: a checkpoint
    has torch's shape and torch's values) and into a fresh LazyRMSprop; three more steps on each route end in the same place"""
    base, batches = _cfg2(seed=4)
    p3, s3, _, _, sd = _fused(base, batches[:3])
    assert set(s3["_final.weight"]) == {"step", "square_avg"}
    mid = copy.deepcopy(base)
    mid.load_state_dict(p3)
    pa, sa, _, _, _ = _fused(mid, batches[3:], state=sd)
    pb, sb = _torch(mid, batches[3:], state=sd)
    _report(pa, pb, sa, sb, "resume")
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert all(float(s["step"]) == 6.0 for s in sa.values())
    # and the whole run equals six torch steps
    pc, sc = _torch(base, batches)
    F._compare_params(pa, pc, TOL["params"], "adam")
    F._compare_state(sa, sc, TOL)


def test_main_train_runs_with_optimizer_rmsprop(tmp_path, capsys):
    logdir = str(tmp_path / "logs")
    args = MT.build_parser().parse_args([
        "--root_dir", F._shards(tmp_path), "--net", "supernet-config", "--supernet_config", F.CFG, "--num_epochs", "1", "--learning_rate", str(LR),
        "--train_batch_size", "8", "--test_batch_size", "16", "--wd", "0", "--logging_dir", logdir, "--gpu", "0", "--test_interval", "4",
        "--display_interval", "2", "--train_limit", "48", "--optimizer", NAME])
    torch.manual_seed(0)
    logs = MT.main(args)
    capsys.readouterr()
    assert all(np.isfinite(v) for v in logs[0]["train_loss"] + logs[0]["test_loss"])
    ck = torch.load(os.path.join(logdir, "supernet-config_checkpoint.pt"), map_location="cpu")
    state = ck["optimizer_state_dict"]["state"]
    assert state and all(set(s) == {"step", "square_avg"} for s in state.values())
    assert ck["optimizer_state_dict"]["param_groups"][0]["alpha"] == 0.99
    assert isinstance(MT.build_optimizer(NAME, torch.nn.Linear(2, 2), LR), LazyRMSprop)
