#!/usr/bin/env python3
"""Cost of `--wd` (L2 weight decay, get_l2_loss) on the bench cfg-2 network: the Criteo best-1shot sub-network, full tables (33.76 M
rows), batch 256, Adagrad(eps 1e-2) + clip 5.0.  Prints one JSON line per measured route:

    python tools/wd_step_bench.py --route fused --wd 1e-8     # the fused engine step with the two weight-decay launches
    python tools/wd_step_bench.py --route fused --wd 0        # the same step without weight decay (bench.py cfg 2)
    python tools/wd_step_bench.py --route torch --wd 1e-8     # forward / autograd on BCE + L2 / clip_grad_norm_ / torch Adagrad

The table pass's bandwidth comes from a kernel trace of the fused route (`rocprofv3 --kernel-trace --stats -- python
tools/wd_step_bench.py --route fused --steps 20`): weight_decay_phase1_kernel moves 4 x 2.16 GB (W and its Adagrad state, read and
written), phase 0 reads W once (2.16 GB) — `--bytes` prints those byte counts for the arithmetic."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import synthetic_batches  # noqa: E402
from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib  # noqa: E402
from nasrec_amd.utils.config import NUM_EMBEDDINGS_CRITEO  # noqa: E402
from nasrec_amd.utils.train_utils import get_l2_loss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["fused", "torch"], default="fused")
    ap.add_argument("--wd", type=float, default=1e-8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--bytes", action="store_true")
    a = ap.parse_args()
    tables = list(NUM_EMBEDDINGS_CRITEO)
    rows = sum(tables)
    if a.bytes:
        print(json.dumps({"table_rows": rows, "phase0_bytes": rows * 64, "phase1_bytes": rows * 64 * 4}))
        return
    dev = torch.device("cuda", 0)
    choice_all = json.load(open(os.path.join(ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_xlarge_best_1shot.json")))
    torch.manual_seed(0)
    m = SuperNet(num_blocks=choice_all["num_blocks"], ops_config=ops_config_lib[choice_all["config"]], use_layernorm=False, num_embeddings=tables,
                 sparse_input_size=26, path_sampling_strategy="fixed-path", fixed=True, fixed_choice=choice_all).to(dev)
    batches = synthetic_batches(8, a.B, 13, tables, dev, seed=1)
    with torch.no_grad():
        m(batches[0][0], batches[0][1])
    opt = torch.optim.Adagrad(m.parameters(), lr=1e-3, eps=1e-2)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    if a.route == "fused":
        m.engine_bind_optimizer(opt)

    def step(i):
        int_x, cat_x, y = batches[i % len(batches)]
        if a.route == "fused":
            m.engine_train_step(int_x, cat_x, y.view(-1), lr=1e-3, clip=5.0, eps=1e-2, weight_decay=a.wd)
            return
        opt.zero_grad()
        loss = loss_fn(m(int_x, cat_x), y.view(-1, 1)) + get_l2_loss(m, a.wd, None, gpu=0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        opt.step()

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
    print(json.dumps({"route": a.route, "wd": a.wd, "B": a.B, "steps": a.steps, "ms_per_step": round(ms, 4),
                      "samples_per_s": round(a.B / ms * 1e3), "wall_ms_per_step": round((time.perf_counter() - t0) / a.steps * 1e3, 4),
                      "table_rows": rows}))


if __name__ == "__main__":
    main()
