"""Row-sparse Adam in the data-parallel fused step (nasrec_amd/parallel.py) on the GPU, in the pattern of
test_data_parallel_optim_2rank_gpu.py: two ranks share cuda:0 over gloo, each runs DataParallelStep on half the batch with the
row-sparse spec, and lands where ONE process's fused engine.train_step lands at the global batch (that file's Adam bar), with
bit-identical replicas — parameters, moments, step counters.  The packed dense-gradient tail on (the optimizer reads the rows in the
all-gather's rank layout) and off, weight decay on the dense parameters, a global batch above NASREC_DEDUP_SPLIT_MAX_B (one-launch
dedup into the contiguous buffer), a weight-sharing supernet."""
import os

import pytest
import torch
import torch.multiprocessing as mp

import test_data_parallel_optim_2rank_gpu as D2
from nasrec_amd.optim_spec import OptimSpec

pytestmark = pytest.mark.gpu
WORLD, STEPS, LR = D2.WORLD, D2.STEPS, D2.LR["adam"]
SPEC = OptimSpec("adam", beta1=0.9, beta2=0.999, eps=1e-8, sparse_rows=True)
NO_REG = "_embedding"


def _worker(rank, port, case, pack, rows, wd, out):
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
    parallel.PACK_TAIL_FLOATS = pack
    z, meta = load_golden(os.path.join(GOLDEN, case + ".npz"))
    int_x, cat_x, y = (torch.tensor(a).cuda() for a in D2._inputs(z, meta, rows))
    Bl = int_x.shape[0] // WORLD
    sl = slice(rank * Bl, (rank + 1) * Bl)
    eng = build_engine(z, meta)
    fixed = meta["mode"] == "fixed"
    dp = DataParallelStep(eng, meta["choice"] if fixed else None, Bl, clip=5.0, eps=1e-2, graph=False, weight_decay=wd,
                          no_reg_param_name=NO_REG if wd else None, optim=SPEC)
    assert dp.exchange and dp.world == WORLD
    losses = []
    for _ in range(STEPS):
        loss = dp.step(int_x[sl].contiguous(), cat_x[sl].contiguous(), y[sl].contiguous(), LR, choice=meta["choice"])
        torch.cuda.synchronize()
        losses.append(float(loss))
    eng.check_indices()
    out[rank] = dict(params={k: v.cpu() for k, v in eng.state_dict().items()}, state=D2._opt_state(eng), losses=losses, tail=dp.tail_n,
                     clean=int(eng._row_bitmap().abs().sum()) == 0 and int(eng._mom_counter[0]) == 0)
    dist.barrier()
    dist.destroy_process_group()


CASES = [
    # (golden network, packed tail floats, synthetic global batch (0: the golden batch), wd on the dense parameters)
    ("fixed_criteo_xlarge", 65536, 0, 0.0),     # rank layout (rows + packed tail), two-halves dedup, one optimizer launch
    ("fixed_criteo_xlarge", 0, 0, 1e-3),        # contiguous receive buffer, phase 1 restores g
    ("fixed_criteo_xlarge", 65536, 4200, 0.0),  # global batch > 2048: one-launch dedup into the contiguous gsum
    ("supernet_xlarge_any", 0, 0, 1e-3),
]


@pytest.mark.parametrize("case,pack,rows,wd", CASES)
def test_two_ranks_equal_one_process_at_the_global_batch(case, pack, rows, wd):
    from helpers import GOLDEN, load_golden
    from test_parity_gpu import build_engine
    z, meta = load_golden(os.path.join(GOLDEN, case + ".npz"))
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(D2._free_port(), case, pack, rows, wd, out), nprocs=WORLD, join=True)
    int_x, cat_x, y = (torch.tensor(a).cuda() for a in D2._inputs(z, meta, rows))
    eng = build_engine(z, meta)
    before = [t.cpu().clone() for t in eng.tables]
    ref_losses = []
    for _ in range(STEPS):
        ref_losses.append(float(eng.train_step(int_x, cat_x, y, LR, choice=meta["choice"], weight_decay=wd,
                                               no_reg_param_name=NO_REG if wd else None, optim=SPEC)))
        torch.cuda.synchronize()
    ref = {k: v.cpu() for k, v in eng.state_dict().items()}
    ref_state = D2._opt_state(eng)
    r0, r1 = out[0], out[1]
    assert r0["clean"] and r1["clean"], "bitmap and counter are left zero"
    assert (r0["tail"] == 0) if pack == 0 else (r0["tail"] > 0)
    for k in ref:
        assert torch.equal(r0["params"][k], r1["params"][k]), "replicas differ: %s" % k
    assert set(r0["state"]) == set(r1["state"]) == set(ref_state) and {"exp_avg", "exp_avg_sq", "opt_steps"} <= set(ref_state)
    for k in r0["state"]:
        assert all(torch.equal(a, b) for a, b in zip(r0["state"][k], r1["state"][k])), "replica optimizer state differs: %s" % k
    assert torch.equal(r0["state"]["opt_steps"][0], ref_state["opt_steps"][0]), "step counters"
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
    # rows outside the global batch rest on the replicas too: W and both moments
    ids = cat_x.cpu()
    for f in range(ids.shape[1]):
        rest = torch.ones(before[f].shape[0], dtype=torch.bool)
        rest[ids[:, f].clamp(0, before[f].shape[0] - 1)] = False
        assert torch.equal(r0["params"]["_embedding.%d.weight" % f][rest], before[f][rest]), f
        assert not r0["state"]["exp_avg"][1 + f][rest].any() and not r0["state"]["exp_avg_sq"][1 + f][rest].any(), f
