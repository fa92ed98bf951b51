#!/usr/bin/env python3
"""What the data-parallel exchange costs on top of the fused step, per optimizer, on the bench cfg-2 network: the Criteo best-1shot
sub-network, full tables (33.76 M rows), batch 256, clip 5.0.  One GPU, one process, two forms of the step on the SAME engine, timed in
alternating rounds:
  plain     DataParallelStep without a process group: the single-process fused step (engine.train_step);
  exchange  DataParallelStep(force_exchange=True, real_collectives=True) in a single-rank RCCL group: the captured exchange step with
            RCCL's all-reduce / all-gather kernels and the optimizer over the gathered batch — what each of N ranks runs.
Optimizers: Adagrad (eps 1e-2) with wd 0 and 1e-8, Adam (eps 1e-8), Nesterov SGD (momentum 0.9), row-sparse Adam (eps 1e-8); lr 1e-3.

    python tools/dp_optim_bench.py --optimizer adam --wd 0     # one optimizer: one JSON line
    python tools/dp_optim_bench.py --all                       # every configuration, each in a child process of its own"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("adagrad", 0.0), ("adagrad", 1e-8), ("adam", 0.0), ("sgd", 0.0), ("row-sparse-adam", 0.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", choices=["adagrad", "adam", "sgd", "row-sparse-adam"], default="adagrad")
    ap.add_argument("--wd", type=float, default=0.0)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20, help="steps per round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds per form, alternating plain / exchange")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--timeout", type=int, default=600, help="--all: seconds per child")
    a = ap.parse_args()
    if a.all:
        for opt, wd in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--optimizer", opt, "--wd", str(wd), "--B", str(a.B), "--steps", str(a.steps),
                   "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True)
            if r.returncode != 0:  # (stop at the first failure: nothing more is started on the GPU)
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("%s exited with %d" % (" ".join(cmd[2:]), r.returncode))
            print(r.stdout.strip().splitlines()[-1], flush=True)
        return

    import socket

    import torch
    import torch.distributed as dist

    from bench import synthetic_batches
    from nasrec_amd.optim_spec import OptimSpec
    from nasrec_amd.parallel import DataParallelStep
    from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib
    from nasrec_amd.utils.config import NUM_EMBEDDINGS_CRITEO
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tables = list(NUM_EMBEDDINGS_CRITEO)
    choice_all = json.load(open(os.path.join(ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_xlarge_best_1shot.json")))
    torch.manual_seed(0)
    m = SuperNet(num_blocks=choice_all["num_blocks"], ops_config=ops_config_lib[choice_all["config"]], use_layernorm=False, num_embeddings=tables,
                 sparse_input_size=26, path_sampling_strategy="fixed-path", fixed=True, fixed_choice=choice_all).to(dev)
    batches = synthetic_batches(8, a.B, 13, tables, dev, seed=1)
    with torch.no_grad():
        m(batches[0][0], batches[0][1])
    eng, choice = m._engine, m._resolve_choice(None)
    optim = {"adam": OptimSpec("adam", eps=1e-8), "sgd": OptimSpec("sgd", momentum=0.9, nesterov=True),
             "row-sparse-adam": OptimSpec("adam", eps=1e-8, sparse_rows=True)}.get(a.optimizer)
    no_reg = "_embedding" if (a.optimizer == "row-sparse-adam" and a.wd) else None  # (row-sparse Adam: the L2 term leaves the tables out)
    kw = dict(clip=5.0, eps=1e-2, weight_decay=a.wd, no_reg_param_name=no_reg, optim=optim)
    plain = DataParallelStep(eng, choice, a.B, graph=None, **kw)  # (no process group yet: the plain step)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)
    try:
        exch = DataParallelStep(eng, choice, a.B, graph=True, force_exchange=True, real_collectives=True, **kw)
        assert not plain.exchange and exch.exchange
        lr = 1e-3
        forms = {"plain": plain, "exchange": exch}

        def run(dp, n, i0=0):
            for i in range(n):
                int_x, cat_x, y = batches[(i0 + i) % len(batches)]
                dp.step(int_x, cat_x, y.view(-1), lr)

        for dp in forms.values():
            run(dp, a.warmup)
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(a.rounds):
            for k, dp in forms.items():
                e0.record()
                run(dp, a.steps, r * a.steps)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.steps)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        print(json.dumps({"optimizer": a.optimizer, "wd": a.wd, "B": a.B, "steps_per_round": a.steps, "rounds": a.rounds,
                          "plain_ms": round(med["plain"], 4), "exchange_ms": round(med["exchange"], 4),
                          "overhead_ms": round(med["exchange"] - med["plain"], 4), "tail_floats": exch.tail_n,
                          "plain_rounds_ms": [round(t, 4) for t in times["plain"]], "exchange_rounds_ms": [round(t, 4) for t in times["exchange"]]}))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
