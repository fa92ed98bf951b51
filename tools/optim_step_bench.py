#!/usr/bin/env python3
"""Cost of the optimizer choice (`--optimizer adagrad | adam | sgd | row-sparse-adam | rowwise-adam | rmsprop | adam-adagrad-tables`, main_train.py:150-160) on the bench cfg-2 network:
the Criteo best-1shot sub-network, full tables (33.76 M rows), batch 256, clip 5.0; Adagrad(eps 1e-2), Adam(eps 1e-8), SGD(momentum 0.9,
Nesterov), row-sparse Adam (Adam's lr and eps; with --wd the L2 term leaves the tables out, as the optimizer requires), RMSprop (torch's
defaults; fused: lazily decayed rows, with --wd the tables left out too; its line also carries `flush_ms`, the one launch that brings
every row's square_avg current after the timed steps), adam-adagrad-tables (Adam's lr and eps on the network, Adagrad at lr x
`--table-lr-scale` on the tables: one phase-0 launch, W and `sum` of the batch's rows; with --wd the tables left out; `--table-rowwise`:
row-wise Adagrad on the tables, one accumulator per row; `--table-dtype bf16` with it: the tables stored as bf16, written with stochastic
rounding — fused route only).  Every line carries `mem_alloc_mb`, torch.cuda.memory_allocated after construction and the timed steps.  `--ema DECAY` keeps utils/optim.WeightEMA beside the step: inside the fused
step (Adagrad, row-sparse Adam, RMSprop), by WeightEMA.update() on the torch route; the line then carries `ema`, `flush_ms` (the launch
that brings every row's average current) and `swap_ms` (flush + exchange with the parameters: what entering `averaged()` costs).
`--decoupled-wd LAMBDA` applies utils/optim.DecoupledWeightDecay in front of the update: inside the fused step (Adagrad, row-sparse Adam,
RMSprop: the rows outside the batch pay lazily), by `apply(lr)` on the torch route; the line then carries `decoupled_wd` and
`decay_flush_ms` (the launch that brings every table row current and re-bases the stamps).
`--cowclip R[,ZETA]` puts utils/optim.CowClip in front of the update: inside the fused step (two more launches: count, clip), by
`apply(cat_x)` on the torch route; the line then carries `cowclip` and, fused, `cowclip_rows` = [touched, clipped] over all steps.
`--batch` is `--B`.
Prints one JSON line per measured (route, optimizer, wd):

    python tools/optim_step_bench.py --route fused --optimizer adam --wd 0     # the fused engine step
    python tools/optim_step_bench.py --route torch --optimizer adam --wd 0     # forward / autograd / clip_grad_norm_ / torch.optim
    python tools/optim_step_bench.py --all                                     # every pair, each in a child process of its own

The table pass's bandwidth comes from a kernel trace of the fused route (`rocprofv3 --kernel-trace --stats -- python
tools/optim_step_bench.py --route fused --optimizer adam --steps 20`): opt_moments_phase1_kernel reads and writes W and its moments
once (Adam 6 x 2.16 GB, SGD 4 x 2.16 GB) — `--bytes` prints those byte counts for the arithmetic."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR = {"adagrad": 1e-3, "adam": 1e-3, "sgd": 1e-3, "row-sparse-adam": 1e-3, "rowwise-adam": 1e-3, "rmsprop": 1e-4, "adam-adagrad-tables": 1e-3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["fused", "torch"], default="fused")
    ap.add_argument("--optimizer", choices=["adagrad", "adam", "sgd", "row-sparse-adam", "rowwise-adam", "rmsprop", "adam-adagrad-tables"], default="adam")
    ap.add_argument("--table-lr-scale", dest="table_lr_scale", type=float, default=1.0,
                    help="adam-adagrad-tables: the tables' learning rate as a multiple of the network's")
    ap.add_argument("--table-rowwise", dest="table_rowwise", action="store_true",
                    help="adam-adagrad-tables: row-wise Adagrad on the tables (one accumulator per row)")
    ap.add_argument("--table-dtype", dest="table_dtype", choices=["fp32", "bf16"], default="fp32",
                    help="adam-adagrad-tables --table-rowwise, fused route: the tables' storage type")
    ap.add_argument("--table-seed", dest="table_seed", type=int, default=0, help="--table-dtype bf16: the stochastic rounding's seed")
    ap.add_argument("--wd", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", "--batch", dest="B", type=int, default=256)
    ap.add_argument("--cowclip", type=str, default=None, help="R[,ZETA]: CowClip on the batch's table rows in front of the update (absent: none)")
    ap.add_argument("--ema", type=float, default=0.0, help="decay of a weight average kept beside the step (0: none)")
    ap.add_argument("--decoupled-wd", dest="decoupled_wd", type=float, default=0.0, help="lambda of a decoupled weight decay in front of the update (0: none)")
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--all", action="store_true", help="every route x optimizer x wd in {0, 1e-8}, then the fused lazy optimizers x "
                                                       "decoupled lambda in {0, 1e-5}, one child process each")
    ap.add_argument("--timeout", type=int, default=600, help="--all: seconds per child")
    a = ap.parse_args()
    from nasrec_amd.utils.config import NUM_EMBEDDINGS_CRITEO
    tables = list(NUM_EMBEDDINGS_CRITEO)
    rows = sum(tables)
    if a.bytes:
        tb = rows * 64
        print(json.dumps({"table_rows": rows, "table_bytes": tb, "adam_phase1_bytes": 6 * tb, "sgd_phase1_bytes": 4 * tb,
                          "adagrad_wd_phase1_bytes": 4 * tb, "wd_phase0_table_bytes": tb,
                          "table_sum_bytes_elementwise": tb, "table_sum_bytes_rowwise": rows * 4, "table_bytes_bf16": rows * 32}))
        return
    if a.all:
        for route in ("fused", "torch"):
            for opt in ("adagrad", "adam", "sgd", "row-sparse-adam", "rowwise-adam", "rmsprop", "adam-adagrad-tables"):
                for wd in (0.0, 1e-8):
                    steps = a.steps if route == "fused" else min(a.steps, 20)
                    cmd = [sys.executable, os.path.abspath(__file__), "--route", route, "--optimizer", opt, "--wd", str(wd), "--steps", str(steps),
                           "--warmup", str(a.warmup), "--B", str(a.B), "--table-lr-scale", str(a.table_lr_scale)]
                    r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True)
                    if r.returncode != 0:  # (stop at the first failure: nothing more is started on the GPU)
                        sys.stderr.write(r.stdout + r.stderr)
                        raise SystemExit("%s exited with %d" % (" ".join(cmd[2:]), r.returncode))
                    print(r.stdout.strip().splitlines()[-1], flush=True)
        for opt in ("adagrad", "row-sparse-adam", "rowwise-adam", "rmsprop"):
            for lam in (0.0, 1e-5):
                cmd = [sys.executable, os.path.abspath(__file__), "--route", "fused", "--optimizer", opt, "--decoupled-wd", str(lam),
                       "--steps", str(a.steps), "--warmup", str(a.warmup), "--B", str(a.B)]
                r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit("%s exited with %d" % (" ".join(cmd[2:]), r.returncode))
                print(r.stdout.strip().splitlines()[-1], flush=True)
        return

    import torch

    from bench import synthetic_batches
    from nasrec_amd import main_train as MT
    from nasrec_amd.optim_spec import OptimSpec
    from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib
    from nasrec_amd.utils.train_utils import get_l2_loss
    dev = torch.device("cuda", 0)
    if a.table_dtype == "bf16" and not (a.route == "fused" and a.optimizer == "adam-adagrad-tables" and a.table_rowwise and not a.wd
                                        and not a.ema and not a.decoupled_wd):
        raise SystemExit("--table-dtype bf16 goes with --route fused --optimizer adam-adagrad-tables --table-rowwise, --wd 0, no --ema / --decoupled-wd")
    choice_all = json.load(open(os.path.join(ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_xlarge_best_1shot.json")))
    torch.manual_seed(0)
    m = SuperNet(num_blocks=choice_all["num_blocks"], ops_config=ops_config_lib[choice_all["config"]], use_layernorm=False, num_embeddings=tables,
                 sparse_input_size=26, path_sampling_strategy="fixed-path", fixed=True, fixed_choice=choice_all,
                 table_dtype=MT.TABLE_DTYPES[a.table_dtype]).to(dev)
    batches = synthetic_batches(8, a.B, 13, tables, dev, seed=1)
    with torch.no_grad():
        m(batches[0][0], batches[0][1])
    lr = LR[a.optimizer]
    opt = MT.build_optimizer(a.optimizer, m, lr, a.table_lr_scale, table_rowwise=a.table_rowwise, table_seed=a.table_seed)
    spec = OptimSpec.from_optimizer(opt) if a.optimizer != "adagrad" else None
    lazy = a.optimizer in ("row-sparse-adam", "rowwise-adam", "rmsprop", "adam-adagrad-tables") and a.route == "fused"  # (the fused step needs the tables left out of the L2 term)
    no_reg = "_embedding" if ((a.optimizer == "row-sparse-adam" or lazy) and a.wd) else None
    loss_fn = torch.nn.BCEWithLogitsLoss()
    if a.route == "fused":
        m.engine_bind_optimizer(opt)
    ema, ema_kw = None, {}
    if a.ema:
        from nasrec_amd.utils.optim import WeightEMA
        ema = WeightEMA(m, a.ema)
        if a.route == "fused":
            m.engine_bind_ema(ema)
            ema_kw = dict(ema_decay=a.ema)
    decay = None
    if a.decoupled_wd:
        from nasrec_amd.utils.optim import DecoupledWeightDecay
        decay = DecoupledWeightDecay(m, a.decoupled_wd, no_reg)
        if a.route == "fused":
            m.engine_bind_decay(decay)
            ema_kw = dict(ema_kw, decoupled_wd=a.decoupled_wd)
    cow = None
    if a.cowclip:
        from nasrec_amd.utils.optim import CowClip, parse_cowclip
        if a.route == "fused":
            ema_kw = dict(ema_kw, cowclip=parse_cowclip(a.cowclip))
        else:
            cow = CowClip(list(m._embedding.parameters()), *parse_cowclip(a.cowclip))

    def step(i):
        int_x, cat_x, y = batches[i % len(batches)]
        if a.route == "fused":
            if spec is not None:
                m.engine_train_step(int_x, cat_x, y.view(-1), lr=lr, clip=5.0, weight_decay=a.wd, no_reg_param_name=no_reg, optim=spec, **ema_kw)
            else:
                m.engine_train_step(int_x, cat_x, y.view(-1), lr=lr, clip=5.0, eps=1e-2, weight_decay=a.wd, **ema_kw)
            return
        opt.zero_grad()
        loss = loss_fn(m(int_x, cat_x), y.view(-1, 1)) + get_l2_loss(m, a.wd, no_reg, gpu=0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        if hasattr(opt, "touch"):
            opt.touch(cat_x)
        if decay is not None:
            decay.apply(lr)
        if cow is not None:
            cow.apply(cat_x)
        opt.step()
        if ema is not None:
            ema.update()

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(a.steps):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    wall_ms = (time.perf_counter() - t0) / a.steps * 1e3
    extra = {}
    if decay is not None:
        extra["decoupled_wd"] = a.decoupled_wd
        if a.route == "fused":  # the flush: every row outside the timed batches pays the factors it rested through
            wall = time.perf_counter()
            m.engine_flush_decay()
            torch.cuda.synchronize()
            extra["decay_flush_ms"] = round((time.perf_counter() - wall) * 1e3, 4)
    if ema is not None:
        extra["ema"] = a.ema
        if a.route == "fused":
            # the flush (every row outside the timed batches owes its average a catch-up) and the exchange with the parameters, there and back
            eng = m._engine
            for key, fn in (("flush_ms", eng.flush_ema_rows), ("flush_again_ms", eng.flush_ema_rows), ("swap_ms", eng.swap_ema), ("swap_back_ms", eng.swap_ema)):
                wall = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                extra[key] = round((time.perf_counter() - wall) * 1e3, 4)
    elif a.optimizer == "rmsprop" and a.route == "fused":
        # the flush: every row outside the timed batches owes its square_avg a decay (one streaming launch, waited for)
        wall = time.perf_counter()
        m._engine.flush_lazy_rows()
        torch.cuda.synchronize()
        extra["flush_ms"] = round((time.perf_counter() - wall) * 1e3, 4)
        wall = time.perf_counter()
        m._engine.flush_lazy_rows()
        torch.cuda.synchronize()
        extra["flush_again_ms"] = round((time.perf_counter() - wall) * 1e3, 4)  # (nothing owed: the stamps are read, nothing else)
    if a.cowclip:
        extra["cowclip"] = a.cowclip
        extra["cowclip_rows"] = list(m.engine_cowclip_stats()) if a.route == "fused" else [cow.touched, cow.clipped]
    if a.optimizer == "adam-adagrad-tables":
        extra["table_lr_scale"] = a.table_lr_scale
        extra["table_rowwise"] = bool(a.table_rowwise)
        extra["table_dtype"] = a.table_dtype
    extra["mem_alloc_mb"] = round(torch.cuda.memory_allocated(dev) / 2 ** 20, 1)
    print(json.dumps({**extra, "route": a.route, "optimizer": a.optimizer, "wd": a.wd, "B": a.B, "steps": a.steps, "ms_per_step": round(ms, 4),
                      "samples_per_s": round(a.B / ms * 1e3), "wall_ms_per_step": round(wall_ms, 4),
                      "table_rows": rows}))


if __name__ == "__main__":
    main()
