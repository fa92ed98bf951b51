#!/usr/bin/env python3
"""The GEMM launches that have a bf16 body at the three matmul precisions (DESIGN.md "Matmul precision"): `highest` (fp32 MFMA — the
kernels every default run uses, the baseline of this table), `high` (bf16 x 3) and `medium` (bf16).  Throughput-regime launches:
csrc/gemm_fast.hip against csrc/gemm_fast_bf16.hip; large-batch token-axis launches: csrc/token_linear.hip against
csrc/token_linear_bf16.hip.

Shapes: the five of profiles/r06_gemm_vs_vendor.txt (forward binding) and the three bindings at 4096 x 1024 x 1024; then token-axis
launches of the config-3 and config-5 supernet steps (forward over K-concatenated segments, the input-gradient batch, the
weight-gradient batch at the planner's split-K).  Random data; one
process; every shape is warmed until the clocks have settled (>= 0.3 s of launches), then the three modes are timed in alternation —
ROUNDS rounds of one window per mode, each window >= 20 launches — and the median window of each mode is reported with its spread.
Every mode's result is checked against the fp64 product first.  A shape that is not a throughput launch runs the same fp32 kernel
at every mode (the precision is a permission only the families with a bf16 body take up); the table says so.

    python tools/gemm_precision_bench.py [--token-only] [--out FILE]
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


def build_token(kind, B, M, Ks, dev):
    """token-axis launches over [B, tokens, 16] slabs.  TF: out[b] = W[M, sum Ks] x[b] over K-concatenated input segments (+ row bias);
    TDX: a batch of len(Ks) input gradients dx_q[b] = W_q[K, M]^T dz[b] (M output rows each); TDW: a batch of len(Ks) weight gradients
    dW_q[M, K] = sum_b dz[b] x_q[b]^T at the planner's split-K -> ({mode: (desc, out, ctx)}, fp64 product, flops, bytes)"""
    E = 16
    if kind == "TF":
        Kt = sum(Ks)
        W, bias = torch.randn(M, Kt, device=dev) * 0.2, torch.randn(M, device=dev)
        xs = [torch.randn(B, k, E, device=dev) for k in Ks]
        ref = torch.einsum("on,bne->boe", W.double(), torch.cat(xs, 1).double()) + bias.double()[None, :, None]
        keep = (W, bias, xs)

        def desc(ctx, out):
            segs, koff = [], 0
            for x, k in zip(xs, Ks):
                segs.append(dict(A=W.data_ptr() + 4 * koff, B=x.data_ptr(), C=out.data_ptr(), M=M, N=B * E, K=k, lda=Kt, ldb=k * E, ldc=M * E))
                koff += k
            return P.gemm_descs(ctx, L.AM_KC, L.AM_TOKR, L.CM_TOKJ, segs, 0, bias=bias.data_ptr(), bias_on_rows=1, mask_on_rows=1)[0]
        shape, flops, nbytes = (B, M, E), 2.0 * M * Kt * B * E, 4.0 * (Kt + M) * B * E
    elif kind == "TDX":
        nq, K = len(Ks), Ks[0]
        W, dz = torch.randn(K, nq * M, device=dev) * 0.2, torch.randn(B, K, E, device=dev)
        ref = torch.einsum("on,boe->bne", W.double(), dz.double())  # [B, nq * M, 16]: problem q is rows q M .. (q + 1) M
        keep = (W, dz)

        def desc(ctx, out):
            segs = [dict(A=W.data_ptr() + 4 * q * M, B=dz.data_ptr(), C=out.data_ptr() + 4 * q * M * E, M=M, N=B * E, K=K, lda=nq * M, ldb=K * E,
                         ldc=nq * M * E) for q in range(nq)]
            return P.gemm_descs(ctx, L.AM_RC, L.AM_TOKR, L.CM_TOKJ, segs, 1)[0]
        shape, flops, nbytes = (B, nq * M, E), 2.0 * nq * M * K * B * E, 4.0 * nq * (K + M) * B * E
    else:
        nq, K = len(Ks), Ks[0]
        dz, xs = torch.randn(B, M, E, device=dev) * 0.3, [torch.randn(B, K, E, device=dev) for _ in Ks]
        ref = torch.stack([torch.einsum("boe,bne->on", dz.double(), x.double()) for x in xs])
        keep = (dz, xs)

        def desc(ctx, out):
            segs = [dict(A=dz.data_ptr(), B=x.data_ptr(), C=out.data_ptr() + 4 * q * M * K, M=M, N=K, K=B * E, lda=M * E, ldb=K * E, ldc=K)
                    for q, x in enumerate(xs)]
            return P.gemm_descs(ctx, L.AM_TOKK, L.AM_TOKK, L.CM_PLAIN, segs, 1)[0]
        shape, flops, nbytes = (nq, M, K), 2.0 * nq * M * K * B * E, 4.0 * nq * (K + M) * B * E
    arms = {}
    for mode in MODES:
        ctx = _Ctx(dev, B, mode)
        out = torch.zeros(*shape, device=dev)
        arms[mode] = (desc(ctx, out), out, ctx)
    return arms, ref, keep, flops, nbytes


BF16_BODIES = ("gemm_fast_bf16_kernel", "token_linear_bf16_kernel", "token_dw_bf16_kernel")


def main():
    lib = L.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    shapes = [("F", 4096, 1024, 1024), ("F", 4096, 1024, 4096), ("F", 4096, 768, 2048), ("F", 8192, 1024, 1024), ("F", 256, 768, 1565),
              ("DX", 4096, 1024, 1024), ("DW", 1024, 1024, 4096)]
    # (kind, B, M, Ks): launches of the config-3 step (B = 4096) and one of config 5's (B = 8192, about 10 tokens)
    token_shapes = [("TF", 4096, 64, [72, 72, 72, 72]), ("TF", 4096, 45, [26, 72, 72]), ("TDX", 4096, 72, [64] * 4), ("TDW", 4096, 64, [72] * 8),
                    ("TF", 8192, 10, [10, 10]),
                    ("TDW", 4096, 72, [72] * 8)]  # 5 x 5 blocks of 16: the token_dw instantiations at the register limit
    lines = ["# %s, one process, %d alternating rounds of %d launches per mode after a clock-settling warm-up; median window (min .. max)"
             % (torch.cuda.get_device_name(dev), ROUNDS, ITERS),
             "# binding F: y = x W^T (KC/KC), DX: dx = dy W (KC/RC), DW: dW = dy^T x (RC/RC); TF = 2 M N K / time; speed-up against `highest` of the same run",
             "# token-axis launches over [B, tokens, 16]: TF forward (KC/TOKR/TOKJ, K-concatenated segments), TDX input-gradient batch (RC/TOKR/TOKJ),",
             "# TDW weight-gradient batch (TOKK/TOKK/PLAIN, main pass + second pass); GB/s = fp32 operand + result bytes of one pass / time",
             "# rel.err = max |C - fp64 product| / max |fp64 product|"]

    def window(d):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            lib.nasrec_launch(st, C.addressof(d))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / ITERS  # us per launch

    if "--token-only" in sys.argv:
        shapes = []
    for shape in shapes + token_shapes:
        torch.manual_seed(5)
        nbytes = None
        if shape[0] in ("F", "DX", "DW"):
            kind, M, N, K = shape
            arms, ref, keep = build(kind, M, N, K, dev)
            fl = 2.0 * M * N * K
            head = "%-2s M=%5d N=%5d K=%5d splitk=%-2d" % (kind, M, N, K, arms["highest"][0].splitk)
        else:
            kind, B, M, Ks = shape
            arms, ref, keep, fl, nbytes = build_token(kind, B, M, Ks, dev)
            what = "K=%s" % "+".join(map(str, Ks)) if kind == "TF" else "%d x (M=%d, K=%d)" % (len(Ks), M, Ks[0]) if kind == "TDX" else "%d x (%d x %d)" % (len(Ks), M, Ks[0])
            head = "%-3s B=%5d %s%s splitk=%-2d" % (kind, B, "M=%d " % M if kind == "TF" else "", what, arms["highest"][0].splitk)
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
        if names["medium"] not in BF16_BODIES:
            head += " [%s at every mode: no bf16 body]" % names["medium"]
        elif nbytes is not None:
            head += " [%s]" % names["medium"]
        lines.append(head)
        for m in MODES:
            lines.append("   %-8s %8.1f us (%7.1f .. %7.1f) = %6.1f TF%s   x%.2f   rel.err %.1e" % (
                m, med[m], min(t[m]), max(t[m]), fl / med[m] / 1e6, "" if nbytes is None else " %6.0f GB/s" % (nbytes / med[m] / 1e3),
                med["highest"] / med[m], errs[m]))
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
