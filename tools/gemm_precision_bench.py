#!/usr/bin/env python3
"""Throughput-regime GEMM at the three matmul precisions (DESIGN.md "Matmul precision"): `highest` (csrc/gemm_fast.hip, fp32 MFMA —
the kernel every default run uses, the baseline of this table), `high` (bf16 x 3) and `medium` (bf16), both csrc/gemm_fast_bf16.hip.

Shapes: the five of profiles/r06_gemm_vs_vendor.txt (forward binding) and the three bindings at 4096 x 1024 x 1024.  Random data; one
process; every shape is warmed until the clocks have settled (>= 0.3 s of launches), then the three modes are timed in alternation —
ROUNDS rounds of one window per mode, each window >= 20 launches — and the median window of each mode is reported with its spread.
Every mode's result is checked against the fp64 product first.  A shape that is not a throughput launch runs the same fp32 kernel
at every mode (the precision is a permission only the throughput kernel takes up); the table says so.

    python tools/gemm_precision_bench.py [--out FILE]
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nasrec_amd import _lib as L  # noqa: E402
from nasrec_amd import plan as P  # noqa: E402

MODES = ("highest", "high", "medium")
ROUNDS, ITERS = 7, 20


class _Ctx:
    """what plan.gemm_descs reads from its context"""

    def __init__(self, dev, B, precision):
        self.keep, self.B, self.dev = [], B, dev
        self.sk_workspace = None
        self.shape_only = False
        self.matmul_precision = L.PRECISION_BY_NAME[precision]

    def alloc(self, n):
        t = torch.empty(int(n), dtype=torch.float32, device=self.dev)
        self.keep.append(t)
        return t


def build(kind, M, N, K, dev):
    """kind F: C[M,N] = A[M,K] W[N,K]^T; DX: C = A[M,K] W[K,N]; DW: C = A[K,M]^T X[K,N] -> ({mode: (desc, out, ctx)}, fp64 product)"""
    if kind == "F":
        A, W = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev)
        sd = dict(A=A.data_ptr(), B=W.data_ptr(), M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
        ref, (am, bm), B = A.double() @ W.double().t(), (L.AM_KC, L.AM_KC), M
    elif kind == "DX":
        A, W = torch.randn(M, K, device=dev), torch.randn(K, N, device=dev)
        sd = dict(A=A.data_ptr(), B=W.data_ptr(), M=M, N=N, K=K, lda=K, ldb=N, ldc=N)
        ref, (am, bm), B = A.double() @ W.double(), (L.AM_KC, L.AM_RC), M
    else:
        A, W = torch.randn(K, M, device=dev), torch.randn(K, N, device=dev)
        sd = dict(A=A.data_ptr(), B=W.data_ptr(), M=M, N=N, K=K, lda=M, ldb=N, ldc=N)
        ref, (am, bm), B = A.double().t() @ W.double(), (L.AM_RC, L.AM_RC), K
    arms = {}
    for mode in MODES:
        ctx = _Ctx(dev, B, mode)
        out = torch.zeros(M, N, device=dev)
        d = P.gemm_descs(ctx, am, bm, L.CM_PLAIN, [dict(sd, C=out.data_ptr())], 0)[0]
        arms[mode] = (d, out, ctx)
    return arms, ref, (A, W)


def main():
    lib = L.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    shapes = [("F", 4096, 1024, 1024), ("F", 4096, 1024, 4096), ("F", 4096, 768, 2048), ("F", 8192, 1024, 1024), ("F", 256, 768, 1565),
              ("DX", 4096, 1024, 1024), ("DW", 1024, 1024, 4096)]
    lines = ["# %s, one process, %d alternating rounds of %d launches per mode after a clock-settling warm-up; median window (min .. max)"
             % (torch.cuda.get_device_name(dev), ROUNDS, ITERS),
             "# binding F: y = x W^T (KC/KC), DX: dx = dy W (KC/RC), DW: dW = dy^T x (RC/RC); TF = 2 M N K / time; speed-up against `highest` of the same run",
             "# rel.err = max |C - fp64 product| / max |fp64 product|"]

    def window(d):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            lib.nasrec_launch(st, C.addressof(d))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / ITERS  # us per launch

    for kind, M, N, K in shapes:
        torch.manual_seed(5)
        arms, ref, keep = build(kind, M, N, K, dev)
        errs, names = {}, {}
        for mode, (d, out, _) in arms.items():
            L.check(lib.nasrec_launch(st, C.addressof(d)))
            torch.cuda.synchronize()
            errs[mode] = float((out.double() - ref).abs().max() / ref.abs().max())
            names[mode] = P.gemm_kernel_name(d)
        assert errs["highest"] < 5e-6 and errs["high"] < 5e-5 and errs["medium"] < 2e-2, errs
        t_end = time.time() + 0.3
        while time.time() < t_end:  # clocks settle under the load that is about to be timed
            for d, _, _ in arms.values():
                window(d)
        t = {m: [] for m in MODES}
        for _ in range(ROUNDS):
            for m in MODES:
                t[m].append(window(arms[m][0]))
        med = {m: statistics.median(t[m]) for m in MODES}
        fl = 2.0 * M * N * K
        head = "%-2s M=%5d N=%5d K=%5d splitk=%-2d" % (kind, M, N, K, arms["highest"][0].splitk)
        if names["medium"] != "gemm_fast_bf16_kernel":
            head += " [%s at every mode: not a throughput launch]" % names["medium"]
        lines.append(head)
        for m in MODES:
            lines.append("   %-8s %8.1f us (%7.1f .. %7.1f) = %6.1f TF   x%.2f   rel.err %.1e" % (
                m, med[m], min(t[m]), max(t[m]), fl / med[m] / 1e6, med["highest"] / med[m], errs[m]))
        del arms, ref, keep
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
