"""torch.optim.Adam and Nesterov-momentum SGD (main_train.py:150-160) in the fused engine step, on the GPU: the harness loop takes the
fused step (`_engine_steps > 0`) and lands where the operator-by-operator torch route lands — parameters, exp_avg / exp_avg_sq /
momentum_buffer, Adam's step, the state's key set and the logged losses — with and without weight decay, on the Criteo best-1shot
network at full table size (every table row moves every step) and on a supernet whose sampled paths leave parameters out; graph
replay equals launching; a checkpoint taken after fused steps resumes on either route to the same place."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib
from nasrec_amd.utils import train_utils as TU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_autoctr_best_1shot.json")
LR = {"adam": 1e-3, "sgd": 0.05}


def _shards(tmp_path, repeat=3):
    z = np.load(os.path.join(GOLDEN, "datapipes.npz"), allow_pickle=False)
    root = tmp_path / "data"
    for s in range(2):
        d = root / ("shard-%d" % s)
        d.mkdir(parents=True)
        for name in ("trainval.txt", "train.txt", "test.txt"):
            src = "trainval.txt" if name == "train.txt" else name
            (d / name).write_text("\n".join([str(z["criteo-kaggle/shard-%d/%s" % (s, src)])] * repeat) + "\n")
    return str(root)


def _args(tmp_path, name, wd):
    return MT.build_parser().parse_args([
        "--root_dir", _shards(tmp_path), "--net", "supernet-config", "--supernet_config", CFG, "--learning_rate", str(LR[name]),
        "--train_batch_size", "8", "--test_batch_size", "16", "--wd", str(wd), "--logging_dir", str(tmp_path / "l"), "--gpu", "0",
        "--optimizer", name, "--train_limit", "48"])


def _base(args, seed=1):
    from nasrec_amd.utils.data_pipes import make_loaders
    train_loader, _ = make_loaders(args)
    torch.manual_seed(seed)
    base = MT.get_model(args).to(0)
    with torch.no_grad():
        TU.warmup_model(base, train_loader, 0)
    base.apply(TU.init_weights)
    return base


def _state(model, opt):
    """{parameter name: {state key: cpu tensor}} of the parameters that have optimizer state"""
    out = {}
    for n, p in model.named_parameters():
        if p in opt.state and opt.state[p]:
            out[n] = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()}
    return out


def _run(model, opt, args, use_engine, steps):
    from nasrec_amd.utils.data_pipes import make_loaders
    train_loader, test_loader = make_loaders(args)
    sched = MT.build_lr_scheduler("constant", opt, steps, 2, args.learning_rate)
    logs = TU.train_and_test_one_epoch(model, 0, opt, sched, train_loader, test_loader, torch.nn.BCEWithLogitsLoss(),
                                       TU.L2Loss(args.wd, None, gpu=0), 8, 0, display_interval=1, test_interval=100, max_train_steps=steps,
                                       grad_clip_value=5.0, use_engine_step=use_engine)
    torch.cuda.synchronize()
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return logs, params, _state(model, opt), model.__dict__.get("_engine_steps", 0)


def _key_bias_noise(k, t, name):
    """Adam: the key part of an attention layer's in_proj_bias, [E, 2E), has a gradient that is exactly zero in exact arithmetic (a
    constant shift of every key score of a query cancels in its softmax): both routes see rounding noise there, ~1e-10, and Adam
    turns noise into steps of +-lr (g / (|g| + eps) with |g| ~ eps).  Those entries are left out of the comparison."""
    if name == "adam" and k.endswith("_mha.in_proj_bias"):
        t = t.clone()
        n = t.numel() // 3
        t[n:2 * n] = 0
    return t


def _compare_params(pa, pb, atol, name=None):
    bad = []
    for k in pa:
        err = float((_key_bias_noise(k, pa[k], name) - _key_bias_noise(k, pb[k], name)).abs().max())
        if err > atol:
            bad.append((k, err))
    assert not bad, bad


def _compare_state(sa, sb, atol):
    assert set(sa) == set(sb), sorted(set(sa) ^ set(sb))
    for n in sa:
        assert set(sa[n]) == set(sb[n]), (n, sorted(sa[n]), sorted(sb[n]))
        for k in sa[n]:
            a, b = sa[n][k], sb[n][k]
            if k == "step":
                assert float(a) == float(b), (n, float(a), float(b))
                continue
            scale = float(b.abs().max()) or 1.0
            err = float((a - b).abs().max())
            assert err <= atol[k] * scale, (n, k, err, scale)


# Adam's step is normalised (m / (sqrt(v) + eps), about +-lr per entry and step whatever the gradient's size): where a gradient entry
# is not much larger than its rounding differences between the routes, the routes step it differently by a fraction of lr.  Its
# parameter bar is 0.05 lr (lr = 1e-3 here); SGD's step is linear in g and keeps the bar of the weight-decay tests.
TOL = {"adam": dict(params=5e-5, exp_avg=1e-4, exp_avg_sq=1e-4), "sgd": dict(params=2e-5, momentum_buffer=1e-4)}


@pytest.mark.parametrize("name", ["adam", "sgd"])
@pytest.mark.parametrize("wd", [0.0, 1e-8])
def test_fused_optimizer_step_equals_the_torch_route(tmp_path, name, wd):
    """the Criteo best-1shot network at full table size (33.76 M rows, 8 samples a step: almost every row moves only through its
    moments and the L2 term): fused step against the torch route over 6 steps"""
    args = _args(tmp_path, name, wd)
    base = _base(args)
    opt = MT.build_optimizer(name, base, args.learning_rate)
    assert TU._fused_step_applies(base, opt, TU.L2Loss(wd, None, gpu=0), False) is True
    res = []
    for use in (None, False):
        m = copy.deepcopy(base)
        res.append(_run(m, MT.build_optimizer(name, m, args.learning_rate), args, use, 6))
        del m
    (la, pa, sa, na), (lb, pb, sb, nb) = res
    assert na == 6 and nb == 0
    assert la["iters"] == lb["iters"] == [0, 1, 2, 3, 4, 5]
    assert np.allclose(la["train_loss"], lb["train_loss"], rtol=1e-5, atol=1e-6), (la["train_loss"], lb["train_loss"])
    _compare_params(pa, pb, TOL[name]["params"], name)
    _compare_state(sa, sb, TOL[name])
    if name == "adam":
        assert all(float(s["step"]) == 6.0 for s in sa.values())
    # Adam with weight decay: the L2 gradient alone moves every row of a table (g / (|g| + eps) with |g| << eps)
    t_before = base._embedding[2].weight.detach().cpu()
    moved = (pa["_embedding.2.weight"] != t_before).any(dim=1).float().mean().item()
    assert moved > (0.99 if (wd and name == "adam") else 0.0), moved


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_fused_optimizer_graph_replay_equals_launch(tmp_path, name):
    """the two Adam / SGD launches inside a captured step: replaying the graph gives the same bits as launching the program"""
    args = _args(tmp_path, name, 1e-8)
    base = _base(args, seed=3)
    from nasrec_amd.utils.data_pipes import make_loaders
    train_loader, _ = make_loaders(args)
    batches = [(a.to(0), b.to(0), c.to(0)) for a, b, c in list(train_loader)[:3]]
    out = []
    for graph in (False, True):
        m = copy.deepcopy(base)
        opt = MT.build_optimizer(name, m, args.learning_rate)
        spec = OptimSpec.from_optimizer(opt)
        m._ensure_engine(batches[0][0])
        m.engine_bind_optimizer(opt)
        for int_x, cat_x, y in batches:
            m.engine_train_step(int_x, cat_x, y.view(-1), lr=args.learning_rate, clip=5.0, graph=graph, weight_decay=1e-8, optim=spec)
        m.engine_sync_optimizer_steps(opt)
        torch.cuda.synchronize()
        out.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, _state(m, opt)))
        del m
    (pa, sa), (pb, sb) = out
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert set(sa) == set(sb)
    for n in sa:
        for k in sa[n]:
            assert torch.equal(torch.as_tensor(sa[n][k]), torch.as_tensor(sb[n][k])), (n, k)


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_resume_after_fused_steps(tmp_path, name):
    """3 fused steps, then the model's and the optimizer's state_dict into a fresh model and a fresh plain torch optimizer, then 3
    more steps on the fused route and on the torch route: both end in the same place"""
    args = _args(tmp_path, name, 1e-8)
    base = _base(args, seed=4)
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(name, m, args.learning_rate)
    _, _, s0, n0 = _run(m, opt, args, None, 3)
    assert n0 == 3
    msd, osd = copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict())
    del m, opt
    res = []
    for use in (None, False):
        m = copy.deepcopy(base)
        m.load_state_dict(msd)
        opt = MT.build_optimizer(name, m, args.learning_rate)
        opt.load_state_dict(osd)
        res.append(_run(m, opt, args, use, 3))
        del m, opt
    (la, pa, sa, na), (lb, pb, sb, nb) = res
    assert na == 3 and nb == 0
    assert np.allclose(la["train_loss"], lb["train_loss"], rtol=1e-5, atol=1e-6)
    _compare_params(pa, pb, TOL[name]["params"], name)
    _compare_state(sa, sb, TOL[name])
    if name == "adam":
        assert all(float(s["step"]) == 6.0 for s in sa.values())


@pytest.mark.parametrize("name", ["adam", "sgd"])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_supernet_sampled_paths_move_only_what_torch_moves(name, wd):
    """a weight-sharing supernet (capped tables, any-path sampling): a parameter off the step's path has no gradient in torch and is
    neither updated nor counted (with weight decay the 2-D ones get 2 wd W and are); every table row moves — fused against torch,
    same paths, same state keys"""
    tables = [min(n, 997) for n in MT._num_embedding_dict["criteo-kaggle"]][:26]
    lr = LR[name]
    g = torch.Generator().manual_seed(7)
    batches = [(torch.randn(16, 13, generator=g).abs().to(0), torch.stack([torch.randint(0, n, (16,), generator=g) for n in tables], 1).to(0),
                torch.randint(0, 2, (16,), generator=g).float().to(0)) for _ in range(4)]
    torch.manual_seed(5)
    base = SuperNet(num_blocks=3, ops_config=ops_config_lib["xlarge"], use_layernorm=True, num_embeddings=tables, sparse_input_size=26,
                    path_sampling_strategy="full-path").to(0)
    with torch.no_grad():
        base(batches[0][0], batches[0][1])
    base.apply(TU.init_weights)
    base.configure_path_sampling_strategy("any-path")
    res = []
    for fused in (True, False):
        m = copy.deepcopy(base)
        opt = MT.build_optimizer(name, m, lr)
        spec = OptimSpec.from_optimizer(opt)
        np.random.seed(11)
        if fused:
            m._ensure_engine(batches[0][0])
            m.engine_bind_optimizer(opt)
        for int_x, cat_x, y in batches:
            if fused:
                m.engine_train_step(int_x, cat_x, y, lr=lr, clip=5.0, weight_decay=wd, optim=spec)
            else:
                opt.zero_grad()
                loss = torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x).view(-1), y) + TU.get_l2_loss(m, wd, None, gpu=0)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
                opt.step()
        if fused:
            m.engine_sync_optimizer_steps(opt)
        torch.cuda.synchronize()
        res.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, _state(m, opt)))
        del m, opt
    (pa, sa), (pb, sb) = res
    _compare_params(pa, pb, TOL[name]["params"], name)
    _compare_state(sa, sb, TOL[name])


@pytest.mark.parametrize("name", ["adam", "sgd"])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_path_that_leaves_the_embeddings_out(name, wd):
    """a path whose last block takes its dense input from the raw dense features (linear-2d, no dense-sparse interaction, no
    deep_fm) and whose sparse node is zeros-3d: no gradient reaches the tables.  torch leaves their grad None — not moved, no step
    counted, no state — unless weight decay gives them 2 wd W; the fused step does the same"""
    tables = [min(n, 997) for n in MT._num_embedding_dict["criteo-kaggle"]][:26]
    choice = {"micro": [{"active_nodes": [0, 6], "dense_in_dims": 16, "sparse_in_dims": 16, "dense_sparse_interact": 0, "deep_fm": 0}],
              "macro": [{"dense_idx": [0], "sparse_idx": [0], "dense_left_idx": [0], "dense_right_idx": [0]}],
              "num_blocks": 1, "use_layernorm": 1, "config": "xlarge-zeros"}
    lr = LR[name]
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(16, 13, generator=g).abs().to(0), torch.stack([torch.randint(0, n, (16,), generator=g) for n in tables], 1).to(0),
                torch.randint(0, 2, (16,), generator=g).float().to(0)) for _ in range(3)]
    torch.manual_seed(5)
    base = SuperNet(num_blocks=1, ops_config=ops_config_lib["xlarge-zeros"], use_layernorm=True, num_embeddings=tables, sparse_input_size=26,
                    path_sampling_strategy="fixed-path", fixed=True, fixed_choice=choice).to(0)
    with torch.no_grad():
        base(batches[0][0], batches[0][1])
    base.apply(TU.init_weights)
    res = []
    for fused in (True, False):
        m = copy.deepcopy(base)
        opt = MT.build_optimizer(name, m, lr)
        spec = OptimSpec.from_optimizer(opt)
        if fused:
            m._ensure_engine(batches[0][0])
            m.engine_bind_optimizer(opt)
        for int_x, cat_x, y in batches:
            if fused:
                m.engine_train_step(int_x, cat_x, y, lr=lr, clip=5.0, weight_decay=wd, optim=spec)
            else:
                opt.zero_grad()
                loss = torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x).view(-1), y) + TU.get_l2_loss(m, wd, None, gpu=0)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
                opt.step()
        if fused:
            assert m.__dict__["_engine_steps"] == 3
            assert not m._engine._last_plan[2].sparse0.grad_written  # (the case under test: no embedding gradient)
            m.engine_sync_optimizer_steps(opt)
        torch.cuda.synchronize()
        res.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, _state(m, opt)))
        del m, opt
    (pa, sa), (pb, sb) = res
    _compare_params(pa, pb, TOL[name]["params"], name)
    _compare_state(sa, sb, TOL[name])
    t0 = base._embedding[0].weight.detach().cpu()
    if wd:
        assert "_embedding.0.weight" in sa and not torch.equal(pa["_embedding.0.weight"], t0)
        if name == "adam":
            assert float(sa["_embedding.0.weight"]["step"]) == 3.0
    else:
        assert not any(n.startswith("_embedding.") for n in sa) and torch.equal(pa["_embedding.0.weight"], t0)
