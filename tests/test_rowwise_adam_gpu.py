"""`--optimizer rowwise-adam` (utils/optim.RowwiseSparseAdam: row-sparse Adam with one second-moment float per embedding row) in the
fused engine step, on the GPU.  Two golden networks as nn.Modules (test_parity_gpu.py's drop-in construction): fixed_criteo_xlarge and
the weight-sharing supernet_xlarge_any pinned to its golden path; three steps on the golden batch.

The fused step against the class's torch route at the project's Adam bars — parameters and tables within
test_data_parallel_optim_2rank_gpu.TOL["adam"] = 5e-5 of max(1, max |reference|), the moments within test_fused_optimizers_gpu.TOL["adam"]
of their scale, its `_key_bias_noise` exclusion; launched against graph replay bit for bit; the engine's state (exp_avg [rows, 16],
exp_avg_sq [rows], nothing else of a table's size); engine_bind_optimizer shares that state and refuses the other Adam form both ways;
a weight average and a decoupled weight decay that reaches the tables, each against its torch route; and one main_train run with the
harness's arguments at batch 8 for 5 steps, wd 0, which prints the fused route."""
import copy
import os

import pytest
import torch

import test_data_parallel_optim_2rank_gpu as D2
import test_fused_optimizers_gpu as F
from helpers import GOLDEN, load_golden
from nasrec_amd import main_train as MT
from nasrec_amd._lib import EngineError
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.search_space import ops_config_lib
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import DecoupledWeightDecay, RowSparseAdam, RowwiseSparseAdam, WeightEMA
from oracle import nasrec_oracle as O

pytestmark = pytest.mark.gpu
NAME, LR, STEPS = "rowwise-adam", D2.LR["adam"], 3
CASES = ["fixed_criteo_xlarge", "supernet_xlarge_any"]


def _build(case):
    from nasrec_amd.supernet.supernet import SuperNet
    z, meta = load_golden(os.path.join(GOLDEN, case + ".npz"))
    fixed = meta["mode"] == "fixed"
    model = SuperNet(num_blocks=meta["num_blocks"], ops_config=ops_config_lib[meta["config"]], use_layernorm=meta["use_layernorm"],
                     activation=meta["activation"], num_embeddings=meta["tables"], sparse_input_size=z["cat_x"].shape[1],
                     path_sampling_strategy="fixed-path" if fixed else "full-path", fixed=fixed,
                     fixed_choice=meta["choice"] if fixed else None, last_n_blocks_out=meta.get("last_n_blocks_out", 1)).to("cuda")
    batch = tuple(torch.tensor(z[k]).cuda() for k in ("int_x", "cat_x", "y"))
    with torch.no_grad():
        model(batch[0], batch[1])
    if not fixed:  # pin the golden path, as the candidate fine-tune does
        model.configure_path_sampling_strategy("fixed-path")
        model.configure_choice(meta["choice"])
    model.load_state_dict({k: torch.tensor(O.seeded_param(k, s), dtype=torch.float32) for k, s in meta["param_shapes"].items()}, strict=True)
    model.train()
    return model, batch


def _snap(m, opt):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, F._state(m, opt)


def _torch_steps(base, batch, ema=None, decay=None):
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(NAME, m, LR)
    avg = WeightEMA(m, ema) if ema else None
    dec = DecoupledWeightDecay(m, decay, None) if decay else None
    int_x, cat_x, y = batch
    for _ in range(STEPS):
        opt.zero_grad()
        torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x), y).backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        opt.touch(cat_x)
        if dec is not None:
            dec.apply(LR)
        opt.step()
        if avg is not None:
            avg.update()
    shadow = {n: s.detach().cpu().clone() for n, s in avg.shadow.items()} if avg is not None else None
    return _snap(m, opt) + (shadow,)


def _fused_steps(base, batch, graph=None, **step_kw):
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(NAME, m, LR)
    spec = OptimSpec.from_optimizer(opt)
    assert spec.table_kind == "rowwise_adam" and spec.rows_only
    int_x, cat_x, y = batch
    m._ensure_engine(int_x)
    m.engine_bind_optimizer(opt)
    for _ in range(STEPS):
        m.engine_train_step(int_x, cat_x, y.view(-1), lr=LR, clip=5.0, graph=graph, optim=spec, **step_kw)
    m.engine_sync_optimizer_steps(opt)
    torch.cuda.synchronize()
    assert int(m._engine._row_bitmap().abs().sum()) == 0 and int(m._engine._mom_counter[0]) == 0
    return _snap(m, opt) + (m, opt)


def _compare(pa, sa, pb, sb):
    """the fused route against the torch route at the project's Adam bars"""
    bad = []
    for k in pb:
        scale = max(1.0, float(pb[k].abs().max()))
        err = float((D2._key_bias_noise(k, pa[k], "adam") - D2._key_bias_noise(k, pb[k], "adam")).abs().max())
        if err > D2.TOL["adam"] * scale:
            bad.append((k, err, scale))
    assert not bad, bad[:8]
    F._compare_state(sa, sb, F.TOL["adam"])


@pytest.fixture(scope="module", params=CASES)
def net(request):
    base, batch = _build(request.param)
    return request.param, base, batch, _torch_steps(base, batch)


@pytest.fixture(scope="module")
def fixed_net():
    base, batch = _build(CASES[0])
    return base, batch


def test_fused_step_equals_the_torch_route(net):
    case, base, batch, (pb, sb, _) = net
    pa, sa, m, opt = _fused_steps(base, batch)
    _compare(pa, sa, pb, sb)
    ids = batch[1].cpu()
    t0 = {k: v.detach().cpu() for k, v in base.state_dict().items()}
    moved = fed = 0
    for f in range(ids.shape[1]):
        k = "_embedding.%d.weight" % f
        n = pa[k].shape[0]
        for s in (sa, sb):
            assert tuple(s[k]["exp_avg"].shape) == (n, 16) and tuple(s[k]["exp_avg_sq"].shape) == (n,), (k, case)
            assert float(s[k]["step"]) == float(STEPS)
        rest = torch.ones(n, dtype=torch.bool)
        rest[ids[:, f]] = False
        for p, s in ((pa, sa), (pb, sb)):  # rows outside the batch: the bits they started with, no moments
            assert torch.equal(p[k][rest], t0[k][rest]), k
            assert not s[k]["exp_avg"][rest].any() and not s[k]["exp_avg_sq"][rest].any(), k
        fed += int(bool((sa[k]["exp_avg_sq"][~rest] > 0).all()))
        moved += int(not torch.equal(pa[k][~rest], t0[k][~rest]))
    assert moved > 0 and fed > 0


def test_launched_equals_graph_replay_bit_for_bit(fixed_net):
    base, batch = fixed_net
    (pa, sa, _, _), (pb, sb, _, _) = _fused_steps(base, batch, graph=False), _fused_steps(base, batch, graph=True)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert set(sa) == set(sb)
    for n in sa:
        for k in sa[n]:
            assert torch.equal(torch.as_tensor(sa[n][k]), torch.as_tensor(sb[n][k])), (n, k)
    assert any(not torch.equal(pa[k], v.detach().cpu()) for k, v in base.state_dict().items() if k.startswith("_embedding."))


def test_engine_state_shapes_and_shared_state(fixed_net):
    base, batch = fixed_net
    _, _, m, opt = _fused_steps(base, batch)
    eng = m._engine
    assert set(eng.moments) == {"exp_avg", "exp_avg_sq"}
    for f, t in enumerate(eng.tables):
        n = int(t.shape[0])
        name = "_embedding.%d.weight" % f
        assert tuple(eng.moments_view("exp_avg", name).shape) == (n, 16)
        v = eng.moments_view("exp_avg_sq", name)
        assert tuple(v.shape) == (n,) and v.dtype == torch.float32
        # the optimizer's state IS the engine's arrays
        st = opt.state[m._embedding[f].weight]
        assert st["exp_avg_sq"].data_ptr() == v.data_ptr() and st["exp_avg"].data_ptr() == eng.moments_view("exp_avg", name).data_ptr()
    # no [rows, 16] second moment exists, and nothing else of a table's size
    assert all(t.dim() == 1 for t in eng.moments["exp_avg_sq"][1]) and len(eng.moments["exp_avg_sq"][1]) == len(eng.tables)
    assert eng.table_state is None and getattr(eng, "table_row_state", None) is None and getattr(eng, "lazy_stamps", None) is None
    assert opt.state[m._final.weight]["exp_avg_sq"].data_ptr() == eng.moments_view("exp_avg_sq", "_final.weight").data_ptr()
    # a resumed optimizer: its state is copied into a fresh engine's arrays, which it then aliases
    fresh = copy.deepcopy(base)
    fresh.load_state_dict(m.state_dict())
    opt2 = MT.build_optimizer(NAME, fresh, LR)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    fresh._ensure_engine(batch[0])
    fresh.engine_bind_optimizer(opt2)
    torch.cuda.synchronize()
    v2 = fresh._engine.moments_view("exp_avg_sq", "_embedding.0.weight")
    assert torch.equal(v2, eng.moments_view("exp_avg_sq", "_embedding.0.weight")) and bool(v2.any())
    assert opt2.state[fresh._embedding[0].weight]["exp_avg_sq"].data_ptr() == v2.data_ptr()
    assert float(fresh._engine.opt_steps[fresh._engine.param_index["_embedding.0.weight"]]) == float(STEPS)


def test_the_other_adam_form_is_refused_both_ways(fixed_net):
    base, batch = fixed_net
    # a row-wise plan's engine refuses a RowSparseAdam ...
    _, _, m, _ = _fused_steps(base, batch)
    other = MT.build_optimizer("row-sparse-adam", m, LR)
    assert type(other) is RowSparseAdam
    with pytest.raises(EngineError, match="RowwiseSparseAdam"):
        m.engine_bind_optimizer(other)
    # ... and the engine of a row-sparse Adam plan refuses a RowwiseSparseAdam
    m2 = copy.deepcopy(base)
    m2._ensure_engine(batch[0])
    m2.engine_bind_optimizer(MT.build_optimizer("row-sparse-adam", m2, LR))
    assert m2._engine.moments["exp_avg_sq"][1][0].dim() == 2
    with pytest.raises(EngineError, match="RowwiseSparseAdam"):
        m2.engine_bind_optimizer(MT.build_optimizer(NAME, m2, LR))
    # a RowwiseSparseAdam that carries the other form's second moment (put there by hand) is refused at the binding: nothing is reshaped
    m3 = copy.deepcopy(base)
    opt = MT.build_optimizer(NAME, m3, LR)
    assert type(opt) is RowwiseSparseAdam
    w0 = m3._embedding[0].weight
    opt.state[w0].update(step=torch.tensor(2.0), exp_avg=torch.zeros_like(w0), exp_avg_sq=torch.full_like(w0, 0.25))
    m3._ensure_engine(batch[0])
    with pytest.raises(ValueError, match="row-wise Adam"):
        m3.engine_bind_optimizer(opt)


def test_with_a_weight_average(fixed_net):
    """ema_decay = 0.99 in the fused step against WeightEMA.update() on the torch route: the parameters as without the average, bit for
    bit; the average against the torch route's shadow at the parameters' bar"""
    base, batch = fixed_net
    decay = 0.99
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(NAME, m, LR)
    spec = OptimSpec.from_optimizer(opt)
    int_x, cat_x, y = batch
    m._ensure_engine(int_x)
    m.engine_bind_optimizer(opt)
    ema = WeightEMA(m, decay)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, ema=ema) == spec._replace(ema=decay)
    m.engine_bind_ema(ema)
    for _ in range(STEPS):
        m.engine_train_step(int_x, cat_x, y.view(-1), lr=LR, clip=5.0, optim=spec, ema_decay=decay)
    sd = ema.state_dict()  # (flushes)
    m.engine_sync_ema(ema)
    assert ema.num_updates == STEPS
    torch.cuda.synchronize()
    end = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    plain = _fused_steps(base, batch)[0]
    assert all(torch.equal(end[n], plain[n]) for n in end)
    shadow = _torch_steps(base, batch, ema=decay)[2]
    got = {n: s.cpu() for n, s in sd["shadow"].items()}
    bad = []
    for n in shadow:
        err = float((D2._key_bias_noise(n, got[n], "adam") - D2._key_bias_noise(n, shadow[n], "adam")).abs().max())
        if err > D2.TOL["adam"] * max(1.0, float(shadow[n].abs().max())):
            bad.append((n, err))
    assert not bad, bad[:8]
    t0 = base.state_dict()
    assert any(not torch.equal(got[n], t0[n].cpu()) for n in got if n.startswith("_embedding."))  # (the average moved)


def test_with_a_decoupled_weight_decay_that_reaches_the_tables(fixed_net):
    """decoupled_wd = 1.0 over every 2-D parameter, the tables included, against DecoupledWeightDecay.apply() on the torch route; the
    rows outside the batch rest, owe, and are paid by the flush (state_dict)"""
    base, batch = fixed_net
    lam = 1.0  # (three steps at lr 1e-3 shrink a table entry of 0.3 by 9e-4: well above the bar)
    m = copy.deepcopy(base)
    opt = MT.build_optimizer(NAME, m, LR)
    assert TU._fused_step_spec(m, opt, TU.L2Loss(0.0, None, gpu=0), False, decay=DecoupledWeightDecay(m, lam, None)) == \
        OptimSpec.from_optimizer(opt)._replace(dwd=lam)
    pa, sa, fm, _ = _fused_steps(base, batch, decoupled_wd=lam)
    assert not fm._engine._decay_dirty
    pb, sb, _ = _torch_steps(base, batch, decay=lam)
    pc = _torch_steps(base, batch)[0]
    gap = max(float((pb[k] - pc[k]).abs().max()) for k in pb if k.startswith("_embedding."))
    assert gap >= 10 * D2.TOL["adam"], gap  # (the decay shows on the torch route alone, or the comparison shows nothing)
    _compare(pa, sa, pb, sb)


def test_main_train_arguments_take_the_fused_route(tmp_path, capsys):
    """main_train's arguments with --optimizer rowwise-adam: Criteo best-1shot at full table size, batch 8, 5 steps, wd 0"""
    args = MT.build_parser().parse_args([
        "--root_dir", F._shards(tmp_path), "--net", "supernet-config", "--supernet_config", F.CFG, "--learning_rate", str(LR),
        "--train_batch_size", "8", "--test_batch_size", "16", "--wd", "0.0", "--logging_dir", str(tmp_path / "l"), "--gpu", "0",
        "--optimizer", NAME, "--train_limit", "48"])
    m = F._base(args)
    t0 = {f: m._embedding[f].weight.detach().cpu().clone() for f in (0, 2, 25)}
    opt = MT.build_optimizer(args.optimizer, m, args.learning_rate, args.table_lr_scale, args.table_eps,
                             table_rowwise=args.table_rowwise, table_seed=args.table_seed)
    assert type(opt) is RowwiseSparseAdam
    assert TU._fused_step_applies(m, opt, TU.L2Loss(0.0, None, gpu=0), False) is True
    import test_row_sparse_adam_gpu as RS
    logs, pa, sa, n = RS._run(m, opt, args, None, 5)
    out = capsys.readouterr().out
    assert "Row-wise Adam" in out and "fused step" in out and "torch route" not in out
    assert n == 5 and logs["iters"] == [0, 1, 2, 3, 4] and all(x == x for x in logs["train_loss"])
    assert all(float(s["step"]) == 5.0 for s in sa.values())
    eng = m._engine
    assert sum(t.numel() for t in eng.moments["exp_avg_sq"][1]) == sum(m._num_embeddings) and eng.table_state is None
    ids = RS._ids(args, 5)
    for f in (0, 2, 25):
        k = "_embedding.%d.weight" % f
        assert tuple(sa[k]["exp_avg_sq"].shape) == (pa[k].shape[0],)
        rest = torch.ones(pa[k].shape[0], dtype=torch.bool)
        rest[ids[:, f]] = False
        assert torch.equal(pa[k][rest], t0[f][rest]) and not torch.equal(pa[k][~rest], t0[f][~rest])
        assert not sa[k]["exp_avg"][rest].any() and not sa[k]["exp_avg_sq"][rest].any() and sa[k]["exp_avg_sq"][~rest].any()
