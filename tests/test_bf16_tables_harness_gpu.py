"""`main_train.py --table-dtype bf16` end to end on synthetic batches: the run prints the fused route with the rounding's seed, finishes,
and saves a checkpoint whose tables are bf16 and whose optimizer state carries the seed and one fp32 accumulator per row; a fresh model
and optimizer load it and go on training.  Avazu's shapes (its tables are the smallest of the three datasets), ids capped at 1000 by the
synthetic source's `cap`, 24 steps of batch 8."""
import os

import numpy as np
import pytest
import torch

from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils.io_utils import load_model_checkpoint, load_optimizer_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "nasrec_amd", "configs", "avazu", "ea_avazu_kaggle_autoctr_best_1shot.json")
STEPS = 24


def _args(logdir, extra=()):
    return MT.build_parser().parse_args([
        "--dataset", "avazu", "--root_dir", "synthetic:steps=%d,test_steps=1,seed=3,cap=1000" % STEPS, "--net", "supernet-config",
        "--supernet_config", CFG, "--num_epochs", "1", "--learning_rate", "1e-3", "--train_batch_size", "8", "--test_batch_size", "16",
        "--wd", "0", "--optimizer", "adam-adagrad-tables", "--table-rowwise", "--table-lr-scale", "160", "--table-dtype", "bf16",
        "--table-seed", "11", "--train_limit", str(8 * STEPS), "--logging_dir", logdir, "--gpu", "0", "--test_interval", "100",
        "--display_interval", "8", "--lr_schedule", "constant-no-warmup"] + list(extra))


def test_main_train_with_bf16_tables_trains_saves_and_reloads(tmp_path, capsys):
    logdir = str(tmp_path / "log")
    args = _args(logdir)
    torch.manual_seed(0)
    np.random.seed(0)
    logs = MT.main(args)
    out = capsys.readouterr().out
    assert "fused step" in out and "bf16 tables stored with stochastic rounding (seed 11)" in out and "row-wise" in out
    assert "torch route" not in out
    assert len(logs) == 1 and all(np.isfinite(v) for v in logs[0]["train_loss"] + logs[0]["test_loss"]) and logs[0]["test_loss"]
    ck = load_model_checkpoint(os.path.join(logdir, "supernet-config_checkpoint.pt"))
    tables = {k: v for k, v in ck["model_state_dict"].items() if k.startswith("_embedding.")}
    assert len(tables) == 23 and all(v.dtype == torch.bfloat16 and v.shape[1] == 16 for v in tables.values())
    assert all(v.dtype == torch.float32 for k, v in ck["model_state_dict"].items() if not k.startswith("_embedding."))
    group = ck["optimizer_state_dict"]["param_groups"][0]
    assert group["table_seed"] == 11 and group["table_rowwise"] is True
    sums = [s["sum"] for s in ck["optimizer_state_dict"]["state"].values() if "sum" in s]
    assert len(sums) == 23 and all(s.dtype == torch.float32 and s.dim() == 1 for s in sums)
    assert sorted(int(s.shape[0]) for s in sums) == sorted(int(v.shape[0]) for v in tables.values())
    assert all(float(s["step"]) == STEPS for s in ck["optimizer_state_dict"]["state"].values() if "sum" in s)
    assert sum(int((s > 0).sum()) for s in sums) > 23  # (the batches' rows have accumulated something)
    assert all(not bool(s[1000:].any()) for s in sums)  # (and no row outside the capped ids has)

    # a fresh model and optimizer take the checkpoint and go on
    model = MT.get_model(args).to(0)
    from nasrec_amd.utils.data_pipes import make_loaders
    train_loader, _ = make_loaders(args)
    int_x, cat_x, y = next(iter(train_loader))
    int_x, cat_x, y = int_x.to(0), cat_x.to(0), y.to(0).float()
    with torch.no_grad():
        model(int_x, cat_x)
    model.load_state_dict(ck["model_state_dict"], strict=True)
    for k, v in tables.items():
        w = dict(model.named_parameters())[k]
        assert w.dtype == torch.bfloat16 and torch.equal(w.detach().cpu().view(torch.int16), v.view(torch.int16))
    opt = MT.build_optimizer(args.optimizer, model, args.learning_rate, args.table_lr_scale, args.table_eps, table_rowwise=True, table_seed=0)
    load_optimizer_state(model, opt, ck["optimizer_state_dict"])
    spec = OptimSpec.from_optimizer(opt)
    assert spec.bf16_tables and spec.table_seed == 11
    model.engine_bind_optimizer(opt)
    loss = model.engine_train_step(int_x, cat_x, y, lr=1e-3, clip=5.0, optim=spec)
    model.engine_sync_optimizer_steps(opt)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    assert all(float(opt.state[e.weight]["step"]) == STEPS + 1 for e in model._embedding)
    assert any(not torch.equal(dict(model.named_parameters())[k].detach().cpu().view(torch.int16), v.view(torch.int16)) for k, v in tables.items())


@pytest.mark.parametrize("extra,word", [(["--ema", "0.99"], "--ema"), (["--decoupled-wd", "1e-4"], "--decoupled-wd"),
                                        (["--table-sharding", "row"], "--table-sharding")])
def test_main_refuses_at_start_up(tmp_path, extra, word):
    args = _args(str(tmp_path / "l"), extra)
    with pytest.raises(ValueError, match=word):
        MT.main(args)
    assert not os.path.exists(str(tmp_path / "l"))  # (before anything is built or written)
