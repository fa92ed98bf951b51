"""Weight decay, Adam and Nesterov SGD in the data-parallel fused step, without a GPU: the harness's choice of route at world 2 (a real gloo
group: a model whose fused step runs them in its exchange step — SuperNet.engine_dp_optimizers — takes it with whole tables; row-sharded
tables, and models without that exchange, keep the torch route), the replica state that broadcast / checksum cover once an engine
holds moments and step counters, and the refusals that remain."""
import os
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU

WORLD = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self.ln = torch.nn.LayerNorm(3)
        self._final = torch.nn.Linear(3, 1)

    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


def _zero_l2(m):
    return TU.get_l2_loss(m, 0.0, None)


class _DPTiny(_Tiny):
    engine_dp_optimizers = True  # (as SuperNet: its engine_train_step runs them inside the data-parallel exchange step)


def _routes(m):
    res = {}
    for name in ("adagrad", "adam", "sgd"):
        opt = MT.build_optimizer(name, m, 0.05)
        res[name] = [TU._fused_step_applies(m, opt, TU.L2Loss(wd), False) for wd in (0.0, 1e-8, 1e-3)]
        res[name + "_no_reg"] = TU._fused_step_applies(m, opt, TU.L2Loss(1e-3, "_embedding"), False)
        res[name + "_opaque"] = TU._fused_step_applies(m, opt, lambda mm: TU.get_l2_loss(mm, 1e-8, None), False)
        m._table_sharding = "row"
        res[name + "_row"] = [TU._fused_step_applies(m, opt, TU.L2Loss(wd), False) for wd in (0.0, 1e-8)]
        m._table_sharding = None
    return res


def _route_worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from nasrec_amd.supernet.supernet import SuperNet
    from nasrec_amd.utils.dist import world_info
    out[rank] = dict(world=world_info()[1], dp=_routes(_DPTiny()), plain=_routes(_Tiny()), supernet=bool(SuperNet.engine_dp_optimizers))
    dist.destroy_process_group()


def test_world_2_takes_the_fused_step_with_whole_tables():
    port = _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_route_worker, args=(port, out), nprocs=WORLD, join=True)
    for r in range(WORLD):
        assert out[r]["world"] == WORLD and out[r]["supernet"]
        res = out[r]["dp"]
        assert res["adagrad"] == [True, True, True]
        assert res["adam"] == [True, True, True] and res["sgd"] == [True, True, True]
        assert res["adagrad_no_reg"] and res["adam_no_reg"] and res["sgd_no_reg"]
        # an opaque non-zero L2 callable: the torch route, at any world size
        assert not (res["adagrad_opaque"] or res["adam_opaque"] or res["sgd_opaque"])
        # row-sharded tables: Adagrad without weight decay only (its own sharded step)
        assert res["adagrad_row"] == [True, False]
        assert res["adam_row"] == [False, False] and res["sgd_row"] == [False, False]
        # a model whose fused step has no data-parallel exchange for them: weight decay, Adam and SGD keep the torch route (Adagrad without
        # weight decay as before)
        res = out[r]["plain"]
        assert res["adagrad"] == [True, False, False]
        assert res["adam"] == [False, False, False] and res["sgd"] == [False, False, False]


def test_one_process_answers_do_not_depend_on_the_flag(monkeypatch):
    from nasrec_amd.utils import dist as D
    monkeypatch.setattr(D, "world_info", lambda: (0, 1))
    assert _routes(_Tiny()) == _routes(_DPTiny())


# ---- replica state ---------------------------------------------------------------------------------------------------------------

def test_replica_tensors_cover_moments_and_step_counters():
    from nasrec_amd.utils.dist import _replica_tensors
    m = _Tiny()
    base = _replica_tensors(m)
    eng = types.SimpleNamespace(flat_s=None, table_state=None)
    m._engine = eng
    assert len(_replica_tensors(m)) == len(base)  # (no optimizer state yet)
    flat_a, tabs_a = torch.zeros(10), [torch.zeros(7, 16), torch.zeros(5, 16)]
    flat_b, tabs_b = torch.ones(10), [torch.ones(7, 16), torch.ones(5, 16)]
    eng.moments = {"exp_avg_sq": (flat_b, tabs_b), "exp_avg": (flat_a, tabs_a)}
    eng.opt_steps = torch.zeros(6)
    got = _replica_tensors(m)
    extra = got[len(base):]
    want = [flat_a] + tabs_a + [flat_b] + tabs_b + [eng.opt_steps]  # (state keys in sorted order: the same on every rank)
    assert len(extra) == len(want) and all(a is b for a, b in zip(extra, want))
    # SGD: one moment array per parameter
    eng.moments = {"momentum_buffer": (flat_a, tabs_a)}
    extra = _replica_tensors(m)[len(base):]
    assert len(extra) == 4 and extra[0] is flat_a and extra[-1] is eng.opt_steps


# ---- refusals --------------------------------------------------------------------------------------------------------------------

class _ProtocolEngine:
    """the data-parallel protocol's surface, nothing behind it (the refusal comes before any plan is built)"""
    cfg = types.SimpleNamespace(fixed=False)
    device = torch.device("cpu")
    Fs = 2

    def dp_plan(self, *a, **k):
        raise AssertionError("not called")


@pytest.mark.parametrize("kw", [dict(weight_decay=1e-8), dict(optim=OptimSpec("adam"))])
def test_per_rank_paths_refuse_weight_decay_and_moments(kw):
    from nasrec_amd._lib import EngineError
    from nasrec_amd.parallel import DataParallelStep
    with pytest.raises(EngineError, match="per-rank"):
        DataParallelStep(_ProtocolEngine(), None, 4, paths="per-rank", **kw)
    DataParallelStep(_ProtocolEngine(), None, 4, paths="per-rank")  # (Adagrad without weight decay: as before)
