"""Row-sparse Adam (`--optimizer row-sparse-adam`, utils/optim.RowSparseAdam) in the fused engine step, on the GPU, in the harness loop
of test_fused_optimizers_gpu.py (its helpers, its Adam bars and its `_key_bias_noise` exclusion): the fused step is taken and lands
where the torch route lands on the Criteo best-1shot network, with and without weight decay on the dense parameters; every table row
outside the batches' ids keeps its bits in W and both moments; graph replay equals launching; a path that skips the embedding stem
does not count the tables' step; a checkpoint after fused steps resumes on either route; and dense `--optimizer adam` still lands where
its torch route lands."""
import copy
import json

import numpy as np
import pytest
import torch

import test_fused_optimizers_gpu as F
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib
from nasrec_amd.utils import train_utils as TU

pytestmark = pytest.mark.gpu
NAME, LR, TOL = "row-sparse-adam", 1e-3, F.TOL["adam"]
NO_REG = "_embedding"


def _args(tmp_path, wd):
    extra = ["--no-reg-param-name", NO_REG] if wd else []
    return MT.build_parser().parse_args([
        "--root_dir", F._shards(tmp_path), "--net", "supernet-config", "--supernet_config", F.CFG, "--learning_rate", str(LR),
        "--train_batch_size", "8", "--test_batch_size", "16", "--wd", str(wd), "--logging_dir", str(tmp_path / "l"), "--gpu", "0",
        "--optimizer", NAME, "--train_limit", "48"] + extra)


def _run(model, opt, args, use_engine, steps):
    from nasrec_amd.utils.data_pipes import make_loaders
    train_loader, test_loader = make_loaders(args)
    sched = MT.build_lr_scheduler("constant", opt, steps, 2, args.learning_rate)
    logs = TU.train_and_test_one_epoch(model, 0, opt, sched, train_loader, test_loader, torch.nn.BCEWithLogitsLoss(),
                                       TU.L2Loss(args.wd, args.no_reg_param_name, gpu=0), 8, 0, display_interval=1, test_interval=100,
                                       max_train_steps=steps, grad_clip_value=5.0, use_engine_step=use_engine)
    torch.cuda.synchronize()
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return logs, params, F._state(model, opt), model.__dict__.get("_engine_steps", 0)


def _ids(args, steps):
    from nasrec_amd.utils.data_pipes import make_loaders
    return torch.cat([b[1] for b in list(make_loaders(args)[0])[:steps]]).cpu()


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_fused_step_equals_the_torch_route(tmp_path, wd):
    """the Criteo best-1shot network at full table size, 5 steps of 8 samples; weight decay regularises the dense parameters only
    (--no_reg_param_name _embedding): phase 1 then only restores the unreached ranges of g and counts"""
    args = _args(tmp_path, wd)
    base = F._base(args)
    opt = MT.build_optimizer(NAME, base, args.learning_rate)
    assert TU._fused_step_applies(base, opt, TU.L2Loss(wd, args.no_reg_param_name, gpu=0), False) is True
    res = []
    for use in (None, False):
        m = copy.deepcopy(base)
        res.append(_run(m, MT.build_optimizer(NAME, m, args.learning_rate), args, use, 5))
        del m
    (la, pa, sa, na), (lb, pb, sb, nb) = res
    assert na == 5 and nb == 0
    assert la["iters"] == lb["iters"] == [0, 1, 2, 3, 4]
    assert np.allclose(la["train_loss"], lb["train_loss"], rtol=1e-5, atol=1e-6), (la["train_loss"], lb["train_loss"])
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert all(float(s["step"]) == 5.0 for s in sa.values()) and "_embedding.2.weight" in sa
    # only the batches' rows moved, on both routes: bit for bit everywhere else
    ids = _ids(args, 5)
    for f in (0, 2, 25):
        k = "_embedding.%d.weight" % f
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        t0 = base._embedding[f].weight.detach().cpu()
        for p, s in ((pa, sa), (pb, sb)):
            assert torch.equal(p[k][rest], t0[rest]) and not torch.equal(p[k][~rest], t0[~rest])
            assert not s[k]["exp_avg"][rest].any() and not s[k]["exp_avg_sq"][rest].any()


def _small(fixed_choice=None, blocks=3, config="xlarge", layernorm=True, seed=5):
    """a network over tables of at most 997 rows, and 4 batches of 16 samples for it"""
    tables = [min(n, 997) for n in MT._num_embedding_dict["criteo-kaggle"]][:26]
    g = torch.Generator().manual_seed(7)
    batches = [(torch.randn(16, 13, generator=g).abs().to(0), torch.stack([torch.randint(0, n, (16,), generator=g) for n in tables], 1).to(0),
                torch.randint(0, 2, (16,), generator=g).float().to(0)) for _ in range(4)]
    torch.manual_seed(seed)
    kw = dict(path_sampling_strategy="fixed-path", fixed=True, fixed_choice=fixed_choice) if fixed_choice is not None else \
        dict(path_sampling_strategy="full-path")
    base = SuperNet(num_blocks=blocks, ops_config=ops_config_lib[config], use_layernorm=layernorm, num_embeddings=tables, sparse_input_size=26,
                    **kw).to(0)
    with torch.no_grad():
        base(batches[0][0], batches[0][1])
    base.apply(TU.init_weights)
    return base, batches


def _optimizer(m, eps=None):
    if eps is None:
        return MT.build_optimizer(NAME, m, LR)
    from nasrec_amd.utils.optim import RowSparseAdam
    return RowSparseAdam(m.parameters(), list(m._embedding.parameters()), lr=LR, eps=eps)


def _fused_steps(base, batches, wd=0.0, graph=None, sampler=None, eps=None):
    """engine_train_step over `batches` on a copy of `base` -> (parameters, optimizer state, did each step's backward reach the stem)"""
    m = copy.deepcopy(base)
    opt = _optimizer(m, eps)
    spec = OptimSpec.from_optimizer(opt)
    if sampler is not None:
        np.random.seed(sampler)
    m._ensure_engine(batches[0][0])
    m.engine_bind_optimizer(opt)
    stem = []
    for int_x, cat_x, y in batches:
        m.engine_train_step(int_x, cat_x, y, lr=LR, clip=5.0, graph=graph, weight_decay=wd, no_reg_param_name=NO_REG if wd else None, optim=spec)
        stem.append(bool(m._engine._last_plan[2].sparse0.grad_written))
    m.engine_sync_optimizer_steps(opt)
    torch.cuda.synchronize()
    assert int(m._engine._row_bitmap().abs().sum()) == 0 and int(m._engine._mom_counter[0]) == 0
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt), stem


def _torch_steps(base, batches, wd=0.0, sampler=None, eps=None):
    m = copy.deepcopy(base)
    opt = _optimizer(m, eps)
    if sampler is not None:
        np.random.seed(sampler)
    for int_x, cat_x, y in batches:
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x).view(-1), y) + TU.get_l2_loss(m, wd, NO_REG, gpu=0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        opt.touch(cat_x)
        opt.step()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt)


def _best_1shot():
    with open(F.CFG) as f:
        return json.load(f)


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_untouched_rows_keep_their_bits(wd):
    choice = _best_1shot()
    base, batches = _small(choice, blocks=choice["num_blocks"], config=choice["config"], layernorm=False)
    pa, sa, stem = _fused_steps(base, batches, wd)
    assert all(stem)
    ids = torch.cat([b[1] for b in batches]).cpu()
    for f in range(26):
        k = "_embedding.%d.weight" % f
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        t0 = base._embedding[f].weight.detach().cpu()
        assert torch.equal(pa[k][rest], t0[rest]), k
        assert not sa[k]["exp_avg"][rest].any() and not sa[k]["exp_avg_sq"][rest].any(), k
        assert float(sa[k]["step"]) == 4.0
        if rest.any():  # (a table of 3 rows may be touched whole)
            assert sa[k]["exp_avg_sq"][~rest].any()
    assert any(bool((pa["_embedding.%d.weight" % f] != base._embedding[f].weight.detach().cpu()).any()) for f in range(26))


def test_eps_of_the_size_of_sqrt_v():
    """eps = 1e-3, the size of sqrt(v) of a table row after a few steps of these gradients: the fused step and the torch route agree
    only if both put eps where SparseAdam puts it (beside sqrt(v), both bias corrections in the step size); at Adam's default 1e-8
    the two placements are closer than the bars"""
    choice = _best_1shot()
    base, batches = _small(choice, blocks=choice["num_blocks"], config=choice["config"], layernorm=False)
    pa, sa, _ = _fused_steps(base, batches, eps=1e-3)
    pb, sb = _torch_steps(base, batches, eps=1e-3)
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_graph_replay_equals_launch(wd):
    choice = _best_1shot()
    base, batches = _small(choice, blocks=choice["num_blocks"], config=choice["config"], layernorm=False, seed=3)
    (pa, sa, _), (pb, sb, _) = _fused_steps(base, batches, wd, graph=False), _fused_steps(base, batches, wd, graph=True)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert set(sa) == set(sb)
    for n in sa:
        for k in sa[n]:
            assert torch.equal(torch.as_tensor(sa[n][k]), torch.as_tensor(sb[n][k])), (n, k)


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_supernet_sampled_paths(wd):
    """a weight-sharing supernet, any-path sampling, same paths on both routes: parameters off a step's path are neither moved nor
    counted (the regularised 2-D ones are, with weight decay); every path of this search space reaches the stem, so the tables count
    every step"""
    base, batches = _small()
    base.configure_path_sampling_strategy("any-path")
    pa, sa, stem = _fused_steps(base, batches, wd, sampler=11)
    pb, sb = _torch_steps(base, batches, wd, sampler=11)
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert all(stem) and float(sa["_embedding.0.weight"]["step"]) == 4.0


REACH = {"active_nodes": [0, 7], "dense_in_dims": 16, "sparse_in_dims": 16, "dense_sparse_interact": 1, "deep_fm": 0}
SKIP = {"active_nodes": [0, 6], "dense_in_dims": 16, "sparse_in_dims": 16, "dense_sparse_interact": 0, "deep_fm": 0}
MACRO = [{"dense_idx": [0], "sparse_idx": [0], "dense_left_idx": [0], "dense_right_idx": [0]}]


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_a_supernet_step_that_skips_the_stem_does_not_count_the_tables(wd):
    """a weight-sharing supernet over the search space with zero nodes, its paths drawn in a fixed order: linear-2d + linear-3d with
    dense-sparse interaction (reaches the stem), linear-2d + zeros-3d without (no gradient reaches the tables), then the first again.
    The tables move and count in steps 1 and 3 only — their counter ends at 2 while _final's ends at 3 — on both routes"""
    base, batches = _small(config="xlarge-zeros", blocks=1)
    paths = [{"micro": [m], "macro": MACRO} for m in (REACH, SKIP, REACH)]
    res = []
    for fused in (True, False):
        m = copy.deepcopy(base)
        opt = MT.build_optimizer(NAME, m, LR)
        spec = OptimSpec.from_optimizer(opt)
        stem, tables = [], []
        if fused:
            m._ensure_engine(batches[0][0])
            m.engine_bind_optimizer(opt)
            drawn, sample = iter(paths), m._resolve_choice
            m.__dict__["_resolve_choice"] = lambda choices=None: sample(next(drawn) if choices is None else choices)
        for path, (int_x, cat_x, y) in zip(paths, batches):
            if fused:
                m.engine_train_step(int_x, cat_x, y, lr=LR, clip=5.0, weight_decay=wd, no_reg_param_name=NO_REG if wd else None, optim=spec)
                stem.append(bool(m._engine._last_plan[2].sparse0.grad_written))
                torch.cuda.synchronize()
                tables.append(m._embedding[0].weight.detach().cpu().clone())
            else:
                opt.zero_grad()
                loss = torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x, path).view(-1), y) + TU.get_l2_loss(m, wd, NO_REG, gpu=0)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
                opt.touch(cat_x)
                opt.step()
        if fused:
            assert stem == [True, False, True]
            assert not torch.equal(tables[0], base._embedding[0].weight.detach().cpu())
            assert torch.equal(tables[1], tables[0]) and not torch.equal(tables[2], tables[1])
            m.engine_sync_optimizer_steps(opt)
        torch.cuda.synchronize()
        res.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt)))
        del m, opt
    (pa, sa), (pb, sb) = res
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    for s in (sa, sb):
        assert all(float(s["_embedding.%d.weight" % f]["step"]) == 2.0 for f in range(26)) and float(s["_final.weight"]["step"]) == 3.0


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["wd0", "wd-dense-only"])
def test_a_path_that_skips_the_stem_does_not_count_the_tables(wd):
    """no gradient reaches the tables (test_fused_optimizers_gpu.py's zeros-3d path): torch leaves their grad None, and the fused
    step neither moves them nor counts a step nor creates state — with weight decay too, since it leaves the tables out"""
    choice = {"micro": [{"active_nodes": [0, 6], "dense_in_dims": 16, "sparse_in_dims": 16, "dense_sparse_interact": 0, "deep_fm": 0}],
              "macro": [{"dense_idx": [0], "sparse_idx": [0], "dense_left_idx": [0], "dense_right_idx": [0]}],
              "num_blocks": 1, "use_layernorm": 1, "config": "xlarge-zeros"}
    base, batches = _small(choice, blocks=1, config="xlarge-zeros")
    pa, sa, stem = _fused_steps(base, batches[:3], wd)
    pb, sb = _torch_steps(base, batches[:3], wd)
    assert stem == [False, False, False]
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert not any(n.startswith("_embedding.") for n in sa)
    assert all(torch.equal(pa["_embedding.%d.weight" % f], base._embedding[f].weight.detach().cpu()) for f in range(26))


def test_resume_after_fused_steps(tmp_path):
    """2 fused steps, then the model's and the optimizer's state_dict into a fresh model and a fresh optimizer, then 3 more steps on the
    fused route and on the torch route: both end in the same place"""
    args = _args(tmp_path, 0.0)
    base = F._base(args, seed=4)
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(NAME, m, args.learning_rate)
    _, _, s0, n0 = _run(m, opt, args, None, 2)
    assert n0 == 2 and set(s0["_final.weight"]) == {"step", "exp_avg", "exp_avg_sq"}
    msd, osd = copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict())
    del m, opt
    res = []
    for use in (None, False):
        m = copy.deepcopy(base)
        m.load_state_dict(msd)
        opt = MT.build_optimizer(NAME, m, args.learning_rate)
        opt.load_state_dict(osd)
        res.append(_run(m, opt, args, use, 3))
        del m, opt
    (la, pa, sa, na), (lb, pb, sb, nb) = res
    assert na == 3 and nb == 0
    assert np.allclose(la["train_loss"], lb["train_loss"], rtol=1e-5, atol=1e-6)
    F._compare_params(pa, pb, TOL["params"], "adam")
    F._compare_state(sa, sb, TOL)
    assert all(float(s["step"]) == 5.0 for s in sa.values())


def test_dense_adam_is_where_it_was(tmp_path):
    """`--optimizer adam` on the same inputs: the untouched instantiations (every row moves, the bitmap, phase 1's table pass) against
    their torch route, as test_fused_optimizers_gpu.py compares them"""
    F.test_fused_optimizer_step_equals_the_torch_route(tmp_path, "adam", 1e-8)
