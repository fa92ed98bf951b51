#!/usr/bin/env python3
"""The search loop at ITS operating point: what one candidate of the regularised-evolution search costs
on one MI355X with the recipe of /root/reference scripts/run_ea/criteo_run_ea_from_supernet_xlarge.sh — Criteo xlarge weight-sharing
supernet (7 blocks, LayerNorm), full tables, the candidate's path pinned, `set_mode_to_finelune_last_only`, Adagrad(lr 0.04, eps 1e-2),
500 training steps at batch 512 and 150 evaluation batches of 8192, one test pass at the end — through the SAME functions the search
CLI runs (`searcher_utils._create_model_train_and_get_results` -> `eval_subnet_from_supernet.finetune_and_eval_one_model` ->
`train_and_test_one_epoch`), on the synthetic pipe (`--root_dir synthetic:...`: host-generated Criteo-shaped batches, H2D per batch).
The only timing the reference publishes for anything is a comment at this operating point (eval_subnet_from_supernet.py:114-115, Tesla M40):
0.05 - 0.06 s per batch-512 step with last-layer-only fine-tuning, 0.21 - 0.23 s fine-tuning the whole network.

Printed: per candidate the wall time of the whole call and of its phases (model build + full-path warm-up + checkpoint load; the 500
training steps; the 150 evaluation batches incl. the AUROC, on the GPU since NASREC_OP_ROC_AUC), candidates / hour / GPU; then the same three step kinds on batches
already resident in HBM (no pipe, no Python harness): last-layer-only step, whole-network fine-tune step, evaluation forward.

--resident: in the same call, on the same build, the same candidates kind scored by ONE ResidentCandidateEvaluator (`--resident_candidates 1`:
set-up once, a restored snapshot per candidate, batches kept on the device, the fused last-layer step), with its per-phase breakdown
and the fused last-layer step on resident batches.  --cli N: the real search CLI (`--method random --random_budget N
--num_parallel_workers 1`, checkpoint on disk, full tables only) timed end to end as a child process, without and with
`--resident_candidates 1`.

--check_auroc: every AUROC call of the harness is recomputed by sklearn on host copies of its inputs (outside the timed phases) and
compared bit for bit; the count of equal results is printed at the end.

    python tools/search_operating_point.py [--candidates 3] [--train_steps 500] [--eval_steps 150] [--resident] [--cli 8] [--check_auroc]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=3)
    ap.add_argument("--train_steps", type=int, default=500)
    ap.add_argument("--eval_steps", type=int, default=150)
    ap.add_argument("--train_batch_size", type=int, default=512)
    ap.add_argument("--test_batch_size", type=int, default=8192)
    ap.add_argument("--cap", type=int, default=0, help="cap the tables (0 = the full 33.76 M rows)")
    ap.add_argument("--profile", action="store_true", help="cProfile of the LAST candidate's call (host time by function)")
    ap.add_argument("--resident", action="store_true", help="also score candidates with one resident evaluator (--resident_candidates 1)")
    ap.add_argument("--cli", type=int, default=0, help="time the search CLI with this random budget, both ways (0 = skip)")
    ap.add_argument("--check_auroc", action="store_true", help="compare every AUROC of the harness with sklearn's, bit for bit")
    a = ap.parse_args()

    from nasrec_amd import eval_subnet_from_supernet as E
    from nasrec_amd.searcher import searcher as S
    from nasrec_amd.searcher import searcher_utils as SU
    from nasrec_amd.utils import train_utils as TU
    from nasrec_amd.utils.config import DATASETS

    tables = list(DATASETS["criteo"]["tables"])
    if a.cap:
        tables = [min(n, a.cap) for n in tables]
    root = "synthetic:steps=%d,test_steps=%d,seed=11" % (a.train_steps, a.eval_steps) + (",cap=%d" % a.cap if a.cap else "")
    args = E.build_parser().parse_args([
        "--dataset", "criteo-kaggle", "--root_dir", root, "--logging_dir", "/tmp/nasrec_search_point", "--config", "xlarge", "--num_blocks", "7",
        "--use_layernorm", "1", "--learning_rate", "0.04", "--wd", "0", "--max_train_steps", str(a.train_steps), "--max_eval_steps", str(a.eval_steps),
        "--train_batch_size", str(a.train_batch_size), "--test_batch_size", str(a.test_batch_size), "--method", "random", "--test_only_at_last_step", "1",
        "--finetune_whole_supernet", "0", "--display_interval", "1000000", "--gpu", "0"])
    args.num_embeddings = tables

    # the supernet checkpoint every candidate starts from (init_weights-scale weights: nothing here depends on their values)
    torch.manual_seed(3)
    np.random.seed(21)
    t0 = time.perf_counter()
    base = SU.build_supernet(args, tables).to(0)
    with torch.no_grad():
        base(torch.zeros(4, 13, device="cuda"), torch.zeros(4, 26, dtype=torch.int64, device="cuda"))
    base.apply(TU.init_weights)
    ckpt = {"model_state_dict": {k: v.detach().clone() for k, v in base.state_dict().items()}}  # (kept on the device: the reference shares it through a manager dict)
    torch.cuda.synchronize()
    print("checkpoint of the supernet built in %.1f s (%d parameter tensors, %.2f GB)" % (
        time.perf_counter() - t0, len(ckpt["model_state_dict"]), sum(v.numel() * 4 for v in ckpt["model_state_dict"].values()) / 1e9))
    del base
    torch.cuda.empty_cache()

    # phase timers: wrap the harness's own functions
    phase = {}
    real_train, real_test, real_auroc = E.train_and_test_one_epoch, TU.test_one_epoch, TU._auroc

    def checked(t):  # wall time since t, less the --check_auroc recomputations made meanwhile
        return time.perf_counter() - t - phase.get("auroc_check", 0.0)

    def timed_train(*x, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter() - phase.get("auroc_check", 0.0)
        r = real_train(*x, **kw)
        torch.cuda.synchronize()
        phase["train_and_test"] = checked(t)
        return r

    def timed_test(*x, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter() - phase.get("auroc_check", 0.0)
        r = real_test(*x, **kw)
        torch.cuda.synchronize()
        phase["test"] = phase.get("test", 0.0) + checked(t)
        return r
    auroc_checks = []

    def timed_auroc(*x, **kw):  # (part of the evaluation phase)
        # the host reaches the AUROC while evaluation forwards are still queued: that wait is timed on its own ("auroc_wait"), so that
        # the AUROC alone is "auroc" and wait + AUROC is what this phase measured when the AUROC ran on the host (its .cpu() waited)
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        t = time.perf_counter()
        phase["auroc_wait"] = phase.get("auroc_wait", 0.0) + t - t0
        r = real_auroc(*x, **kw)
        t1 = time.perf_counter()
        phase["auroc"] = phase.get("auroc", 0.0) + t1 - t
        if a.check_auroc:
            import sklearn.metrics
            want = sklearn.metrics.roc_auc_score(x[0].detach().cpu().numpy(), x[1].detach().cpu().numpy())
            auroc_checks.append((float(r).hex() == float(want).hex(), x[1].is_cuda, x[1].numel()))
            phase["auroc_check"] = phase.get("auroc_check", 0.0) + time.perf_counter() - t1
        return r
    E.train_and_test_one_epoch = timed_train
    TU.test_one_epoch = timed_test
    TU._auroc = timed_auroc

    searcher = S.Searcher(E.finetune_and_eval_one_model, args)
    tok = searcher._tokenizer
    rows = []
    for c in range(a.candidates):
        choice = None  # (random search: `configure_path_sampling_strategy("fixed-path")` draws the candidate, searcher.py:134-152)
        phase.clear()
        torch.cuda.synchronize()
        t = time.perf_counter()
        prof = None
        if a.profile and c == a.candidates - 1:
            import cProfile
            prof = cProfile.Profile()
            prof.enable()
        res = SU._create_model_train_and_get_results(argparse.Namespace(**vars(args)), 0, E.finetune_and_eval_one_model, tok, choice, ckpt, {"beta": 0.0})
        if prof is not None:
            prof.disable()
            import io
            import pstats
            buf = io.StringIO()
            pstats.Stats(prof, stream=buf).sort_stats("cumulative").print_stats(45)
            print(buf.getvalue())
        torch.cuda.synchronize()
        total = checked(t)
        tr = phase.get("train_and_test", 0.0) - phase.get("test", 0.0)
        rows.append((total, total - phase.get("train_and_test", 0.0), tr, phase.get("test", 0.0), res["test_loss"][-1], res["test_auroc"][-1]))
        print("candidate %d: %.2f s = set-up (build, full-path warm-up, checkpoint load) %.2f + %d training steps %.2f (%.3f ms/step, %.0f samples/s) "
              "+ %d evaluation batches %.2f (%.2f ms/batch, %.2f M samples/s);  test loss %.4f AUROC %.4f" % (
                  c, total, rows[-1][1], a.train_steps, tr, tr / a.train_steps * 1e3, a.train_batch_size * a.train_steps / max(tr, 1e-9),
                  a.eval_steps, rows[-1][3], rows[-1][3] / a.eval_steps * 1e3, a.test_batch_size * a.eval_steps / max(rows[-1][3], 1e-9) / 1e6,
                  rows[-1][4], rows[-1][5]))
    if rows:
        use = rows[1:] if len(rows) > 1 else rows  # (the first candidate also pays one-off costs: kernels' first launches, allocator growth)
        mean = float(np.mean([r[0] for r in use]))
        print("steady state: %.2f s per candidate = %.0f candidates / hour / GPU  (reference, Tesla M40, from its own comment: 500 x 0.05 - 0.06 s = 25 - 30 s of "
              "training steps alone per candidate)" % (mean, 3600.0 / mean))

    if a.resident:
        from nasrec_amd.searcher import resident as R
        real_rtrain = R.train_and_test_one_epoch
        R.train_and_test_one_epoch = timed_train
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev = R.ResidentCandidateEvaluator(argparse.Namespace(**vars(args)), ckpt, gpu=0)
        torch.cuda.synchronize()
        setup = time.perf_counter() - t
        print("resident evaluator: set-up once (build, full-path warm-up, checkpoint load, snapshot, %s batches on the device) %.2f s" % (
            "first" if ev.resident else "NO", setup))
        rrows = []
        for c in range(a.candidates):
            phase.clear()
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = R.evaluate_candidate(ev, tok, None, {"beta": 0.0})
            torch.cuda.synchronize()
            total = checked(t)
            tt = phase.get("train_and_test", 0.0)
            te = phase.get("test", 0.0)
            rrows.append(total)
            print("resident candidate %d: %.2f s = restore + optimizer %.3f + %d fused last-layer steps %.2f (%.3f ms/step) + %d evaluation batches %.2f "
                  "(%.2f ms/batch; AUROC %.3f s = %.1f %% of the candidate, after %.3f s waiting for the queued forwards);  test loss %.4f AUROC %.4f" % (
                      c, total, total - tt, a.train_steps, tt - te, (tt - te) / a.train_steps * 1e3, a.eval_steps, te, te / a.eval_steps * 1e3,
                      phase.get("auroc", 0.0), 100.0 * phase.get("auroc", 0.0) / total, phase.get("auroc_wait", 0.0), res["test_loss"][-1],
                      res["test_auroc"][-1]))
        R.train_and_test_one_epoch = real_rtrain
        use = rrows[1:] if len(rrows) > 1 else rrows
        rmean = float(np.mean(use))
        print("resident steady state: %.2f s per candidate = %.0f candidates / hour / GPU (set-up %.2f s once per search)" % (rmean, 3600.0 / rmean, setup))
        if rows:
            print("rebuild against resident, same call and build: %.2f s -> %.2f s per candidate (%.1fx)" % (mean, rmean, mean / rmean))
        # the fused last-layer step alone, on batches already on the device
        import bench
        m = ev.model
        tb = bench.synthetic_batches(8, a.train_batch_size, 13, tables, "cuda", 100)
        opt = torch.optim.Adagrad(m.parameters(), lr=0.04, eps=1e-2)
        m.engine_bind_optimizer(opt, last_layer=True)

        def fused(i):
            int_x, cat_x, y = tb[i % len(tb)]
            m.engine_last_layer_step(int_x, cat_x, y.view(-1), 0.04)
        for i in range(10):
            fused(i)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(200):
            fused(i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / 200
        print("resident batches, fused last-layer step (engine_last_layer_step, B = %d): %.3f ms = %.0f samples/s   (torch route, r06: 1.474 ms)" % (
            a.train_batch_size, dt * 1e3, a.train_batch_size / dt))
        del m, opt, tb
        ev.close()
        del ev
    E.train_and_test_one_epoch, TU.test_one_epoch, TU._auroc = real_train, real_test, real_auroc
    if a.check_auroc:
        print("AUROC calls of the harness: %d (%d on the GPU, sizes %s); bit-identical to sklearn on host copies: %d" % (
            len(auroc_checks), sum(c[1] for c in auroc_checks), sorted({c[2] for c in auroc_checks}), sum(c[0] for c in auroc_checks)))

    if a.cli:
        cli_timings(a, args, ckpt, root)

    # ---- the same step kinds on batches resident in HBM: no pipe, no harness loop ----------------------------------------------
    import bench  # (synthetic_batches: the bench's input generator)
    model = SU.build_supernet(args, tables).to(0)
    with torch.no_grad():
        model(torch.zeros(4, 13, device="cuda"), torch.zeros(4, 26, dtype=torch.int64, device="cuda"))
    model.load_state_dict(ckpt["model_state_dict"], strict=True)
    model.configure_path_sampling_strategy("fixed-path")
    loss_fn = torch.nn.BCEWithLogitsLoss()
    tb = bench.synthetic_batches(8, a.train_batch_size, 13, tables, "cuda", 100)
    eb = bench.synthetic_batches(4, a.test_batch_size, 13, tables, "cuda", 200)

    def timeit(fn, n, w=10):
        for i in range(w):
            fn(i)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(n):
            fn(w + i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n

    model.set_mode_to_finelune_last_only()
    opt = torch.optim.Adagrad(model.parameters(), lr=0.04, eps=1e-2)

    def last_only(i):
        int_x, cat_x, y = tb[i % len(tb)]
        opt.zero_grad()
        loss_fn(model(int_x, cat_x), y.view(-1, 1)).backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        opt.step()
    dt = timeit(last_only, 200)
    print("resident batches, last-layer-only fine-tune step (B = %d): %.3f ms = %.0f samples/s   (reference comment: 50 - 60 ms on a Tesla M40)" % (
        a.train_batch_size, dt * 1e3, a.train_batch_size / dt))

    def evaluate(i):
        with torch.no_grad():
            model(eb[i % len(eb)][0], eb[i % len(eb)][1])
    model.eval()
    dt = timeit(evaluate, 100)
    print("resident batches, evaluation forward (B = %d): %.3f ms = %.2f M samples/s" % (a.test_batch_size, dt * 1e3, a.test_batch_size / dt / 1e6))
    model.train()
    model.set_mode_to_normal_mode()
    lr = 0.04

    def whole(i):
        int_x, cat_x, y = tb[i % len(tb)]
        model.engine_train_step(int_x, cat_x, y.view(-1), lr)
    dt = timeit(whole, 200)
    print("resident batches, whole-network fine-tune step, fused engine step (B = %d): %.3f ms = %.0f samples/s   (reference comment: 210 - 230 ms on a Tesla M40)" % (
        a.train_batch_size, dt * 1e3, a.train_batch_size / dt))


def cli_timings(a, args, ckpt, root):
    """the search CLI as a user runs it — `python -m nasrec_amd.eval_subnet_from_supernet --method random --random_budget N
    --num_parallel_workers 1` with the checkpoint on disk — timed end to end, without and with --resident_candidates 1"""
    import shutil
    import subprocess
    import tempfile
    if a.cap:
        print("--cli: the CLI has no table cap (full tables only): skipped")
        return
    d = tempfile.mkdtemp(prefix="nasrec_cli_")
    try:
        if shutil.disk_usage(d).free < 4 * 2.85e9:
            print("--cli: not enough free disk space for the checkpoint in %s: skipped" % d)
            return
        path = os.path.join(d, "supernet.pt")
        t = time.perf_counter()
        torch.save({"model_state_dict": {k: v.cpu() for k, v in ckpt["model_state_dict"].items()}}, path)
        print("checkpoint written in %.1f s (%.2f GB)" % (time.perf_counter() - t, os.path.getsize(path) / 1e9))
        for flag in ("0", "1"):
            cmd = [sys.executable, "-m", "nasrec_amd.eval_subnet_from_supernet", "--dataset", "criteo-kaggle", "--root_dir", root,
                   "--logging_dir", os.path.join(d, "log" + flag), "--config", "xlarge", "--num_blocks", "7", "--use_layernorm", "1",
                   "--learning_rate", "0.04", "--wd", "0", "--max_train_steps", str(a.train_steps), "--max_eval_steps", str(a.eval_steps),
                   "--train_batch_size", str(a.train_batch_size), "--test_batch_size", str(a.test_batch_size), "--method", "random",
                   "--random_budget", str(a.cli), "--num_parallel_workers", "1", "--test_only_at_last_step", "1", "--display_interval",
                   "1000000", "--ckpt_path", path, "--resident_candidates", flag]
            t = time.perf_counter()
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t
            if r.returncode != 0:
                print("CLI --resident_candidates %s failed (exit %d): %s" % (flag, r.returncode, r.stderr.decode(errors="replace")[-2000:]))
                return
            print("CLI --method random --random_budget %d --num_parallel_workers 1 --resident_candidates %s: %.1f s end to end = %.2f s per "
                  "candidate = %.0f candidates / hour / GPU (process start, imports and checkpoint reads included)" % (
                      a.cli, flag, dt, dt / a.cli, 3600.0 * a.cli / dt))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
