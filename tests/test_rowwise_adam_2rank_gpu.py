"""Row-wise Adam (OptimSpec.table_kind "rowwise_adam": row-sparse Adam with one second-moment float per table row) in the data-parallel
fused step (nasrec_amd/parallel.py) on the GPU, in the pattern of test_rowwise_adagrad_2rank_gpu.py: two ranks share cuda:0 over gloo,
each runs DataParallelStep on half the batch, and lands where ONE process's fused engine.train_step lands at the global batch — the bar
of test_data_parallel_optim_2rank_gpu.py, TOL["adam"] = 5e-5 on the dense parameters and on the tables — with bit-identical replicas:
parameters, both moments (the tables' exp_avg [rows, 16] and exp_avg_sq [rows] included), step counters; a clean bitmap and counter;
rows outside the global batch rest.  One case: fixed_criteo_xlarge with the packed dense-gradient tail on (the optimizer reads the rows
in the all-gather's rank layout), wd 0.  Each child process is freshly spawned and runs under its own time limit."""
import os
import time

import pytest
import torch
import torch.multiprocessing as mp

import test_data_parallel_optim_2rank_gpu as D2
from nasrec_amd.optim_spec import OptimSpec

pytestmark = pytest.mark.gpu
WORLD, STEPS, LR = D2.WORLD, D2.STEPS, D2.LR["adam"]
SPEC = OptimSpec("adam", beta1=0.9, beta2=0.999, eps=1e-8, table_kind="rowwise_adam")
CASE, PACK = "fixed_criteo_xlarge", 65536
CHILD_TIMEOUT = 180  # seconds for the two ranks (the case takes a fraction of that)


def _worker(rank, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from helpers import GOLDEN, load_golden
    from nasrec_amd import parallel
    from nasrec_amd.parallel import DataParallelStep
    from test_parity_gpu import build_engine
    parallel.PACK_TAIL_FLOATS = PACK
    z, meta = load_golden(os.path.join(GOLDEN, CASE + ".npz"))
    int_x, cat_x, y = (torch.tensor(a).cuda() for a in D2._inputs(z, meta, 0))
    Bl = int_x.shape[0] // WORLD
    sl = slice(rank * Bl, (rank + 1) * Bl)
    eng = build_engine(z, meta)
    dp = DataParallelStep(eng, meta["choice"], Bl, clip=5.0, eps=1e-2, graph=False, optim=SPEC)
    assert dp.exchange and dp.world == WORLD
    losses = []
    for _ in range(STEPS):
        loss = dp.step(int_x[sl].contiguous(), cat_x[sl].contiguous(), y[sl].contiguous(), LR, choice=meta["choice"])
        torch.cuda.synchronize()
        losses.append(float(loss))
    eng.check_indices()
    out[rank] = dict(params={k: v.cpu() for k, v in eng.state_dict().items()}, state=D2._opt_state(eng), losses=losses, tail=dp.tail_n,
                     clean=int(eng._row_bitmap().abs().sum()) == 0 and int(eng._mom_counter[0]) == 0,
                     no_sums=eng.table_state is None and getattr(eng, "table_row_state", None) is None)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(args):
    ctx = mp.spawn(_worker, args=args, nprocs=WORLD, join=False)
    deadline = time.monotonic() + CHILD_TIMEOUT
    while not ctx.join(timeout=2.0):  # (returns as soon as every rank is done; raises when one failed)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank did not finish within %d s" % CHILD_TIMEOUT)


def test_two_ranks_equal_one_process_at_the_global_batch():
    from helpers import GOLDEN, load_golden
    from test_parity_gpu import build_engine
    z, meta = load_golden(os.path.join(GOLDEN, CASE + ".npz"))
    out = mp.Manager().dict()
    _spawn((D2._free_port(), out))
    int_x, cat_x, y = (torch.tensor(a).cuda() for a in D2._inputs(z, meta, 0))
    eng = build_engine(z, meta)
    before = [t.cpu().clone() for t in eng.tables]
    ref_losses = []
    for _ in range(STEPS):
        ref_losses.append(float(eng.train_step(int_x, cat_x, y, LR, choice=meta["choice"], optim=SPEC)))
        torch.cuda.synchronize()
    ref = {k: v.cpu() for k, v in eng.state_dict().items()}
    ref_state = D2._opt_state(eng)
    r0, r1 = out[0], out[1]
    assert r0["clean"] and r1["clean"], "bitmap and counter are left zero"
    assert r0["no_sums"] and r1["no_sums"], "an Adagrad accumulator was allocated"
    assert r0["tail"] > 0
    # the replicas: bit-identical in parameters, both moments and step counters
    for k in ref:
        assert torch.equal(r0["params"][k], r1["params"][k]), "replicas differ: %s" % k
    assert set(r0["state"]) == set(r1["state"]) == set(ref_state) and {"exp_avg", "exp_avg_sq", "opt_steps"} <= set(ref_state)
    for k in r0["state"]:
        assert len(r0["state"][k]) == len(r1["state"][k]) == len(ref_state[k])
        assert all(torch.equal(a, b) for a, b in zip(r0["state"][k], r1["state"][k])), "replica optimizer state differs: %s" % k
    Fs = len(before)
    assert len(r0["state"]["exp_avg"]) == len(r0["state"]["exp_avg_sq"]) == 1 + Fs  # (the flat arena, then the tables)
    assert [tuple(t.shape) for t in r0["state"]["exp_avg"][1:]] == [tuple(b.shape) for b in before]
    assert [tuple(t.shape) for t in r0["state"]["exp_avg_sq"][1:]] == [(b.shape[0],) for b in before], "one second-moment float per row"
    assert torch.equal(r0["state"]["opt_steps"][0], ref_state["opt_steps"][0]), "step counters"
    assert float(r0["state"]["opt_steps"][0].max()) == float(STEPS)
    # both ranks against one process at the global batch
    bad = []
    for k in ref:
        scale = max(1.0, float(ref[k].abs().max()))
        err = float((D2._key_bias_noise(k, r0["params"][k], "adam") - D2._key_bias_noise(k, ref[k], "adam")).abs().max())
        if err > D2.TOL["adam"] * scale:
            bad.append((k, err, scale))
    assert not bad, bad[:8]
    for t in range(STEPS):
        assert abs(0.5 * (r0["losses"][t] + r1["losses"][t]) - ref_losses[t]) <= 1e-4 * max(1.0, abs(ref_losses[t])), \
            (t, r0["losses"][t], r1["losses"][t], ref_losses[t])
    # rows outside the global batch rest on the replicas too: W and both moments; the batch's rows moved
    ids = cat_x.cpu()
    moved = 0
    for f in range(ids.shape[1]):
        rest = torch.ones(before[f].shape[0], dtype=torch.bool)
        rest[ids[:, f].clamp(0, before[f].shape[0] - 1)] = False
        assert torch.equal(r0["params"]["_embedding.%d.weight" % f][rest], before[f][rest]), f
        m, v = r0["state"]["exp_avg"][1 + f], r0["state"]["exp_avg_sq"][1 + f]
        assert not m[rest].any() and not v[rest].any(), f
        moved += int(not torch.equal(r0["params"]["_embedding.%d.weight" % f][~rest], before[f][~rest]))
        v_ref = ref_state["exp_avg_sq"][1 + f]
        # (test_fused_optimizers_gpu.TOL["adam"]["exp_avg_sq"]: 1e-4 of the array's scale)
        assert float((v - v_ref).abs().max()) <= 1e-4 * (float(v_ref.abs().max()) or 1.0), (f, float((v - v_ref).abs().max()))
        assert v[~rest].any() or rest.all(), f
    assert moved > 0
