#!/usr/bin/env python3
"""Time of NASREC_OP_ROC_AUC (nasrec_amd.metrics.roc_auc_score) on one GPU against sklearn.metrics.roc_auc_score on the host.

Per size: the op's launch chain alone (HIP events around nasrec_roc_auc on a preallocated workspace), the whole call
(metrics.roc_auc_score: workspace from torch's allocator, the chain and the 12-byte readback, HIP events around it), and sklearn on
host arrays (the harness's route before: .cpu() of both tensors and roc_auc_score).  The results are checked bit for bit.
Sizes: 1 228 800 = the search's 150 evaluation batches of 8192, 4 600 000 = about one Criteo test split.

    python tools/roc_auc_bench.py [--sizes 1228800,4600000] [--iters 50] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import sklearn.metrics  # noqa: E402
import torch  # noqa: E402

from nasrec_amd import _lib as L  # noqa: E402
from nasrec_amd import metrics  # noqa: E402


def inputs(n, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.25).astype(np.float32)
    z = rng.normal(size=n) + 0.8 * y
    return y, (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def event_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(iters):
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1228800,4600000")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = L.load()
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        y, s = inputs(n, seed=n)
        yt, st = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
        ws_bytes = int(lib.nasrec_roc_auc_workspace_bytes(n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(16, dtype=torch.uint8, device="cuda")
        d = L.RocAucDesc(kind=L.OP_ROC_AUC, n=n, score=st.data_ptr(), label=yt.data_ptr(), workspace=ws.data_ptr(),
                         workspace_bytes=ws_bytes, out=out.data_ptr())

        def chain():
            L.check(lib.nasrec_roc_auc(torch.cuda.current_stream().cuda_stream, C.byref(d)))
        for _ in range(5):
            chain()
            metrics.roc_auc_score(yt, st)
        torch.cuda.synchronize()
        chain_med, chain_min = event_ms(chain, a.iters)
        call_med, call_min = event_ms(lambda: metrics.roc_auc_score(yt, st), a.iters)
        got = metrics.roc_auc_score(yt, st)
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            want = sklearn.metrics.roc_auc_score(yt.cpu().numpy(), st.cpu().numpy())
            host.append((time.perf_counter() - t) * 1e3)
        row = {"n": n, "chain_ms_median": round(chain_med, 4), "chain_ms_min": round(chain_min, 4), "call_ms_median": round(call_med, 4),
               "call_ms_min": round(call_min, 4), "sklearn_host_ms_median": round(float(np.median(host)), 2),
               "workspace_mb": round(ws_bytes / 2**20, 1), "auc": got.hex(), "bit_equal_to_sklearn": got.hex() == float(want).hex()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["bit_equal_to_sklearn"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
