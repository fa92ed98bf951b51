"""Row-sparse Adam without a GPU: the torch route (utils/optim.RowSparseAdam with `touch`) against torch itself — torch.optim.SparseAdam on
twin tables built with sparse=True, torch.optim.Adam on the rest, in fp64 —, its OptimSpec and the harness's choice of route at world 1
and at world 2 (a real gloo group), the refusal of a regularised table, the four CLIs' choice, and the grown descriptor's layout check."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import RowSparseAdam

ROWS = (7, 5)
LR, CLIP = 0.05, 0.5
# ids [B, 2] per step: duplicates inside a batch; row 6 of table 0 at steps 1 and 4 only; step 3 reaches table 0 alone
IDS = [[[6, 1], [2, 1], [2, 4]], [[0, 0], [0, 3], [3, 3]], [[1, 2], [1, 2], [5, 2]], [[6, 4], [4, 4], [6, 0]]]
NO_TABLE_1 = 2  # (index of the step in which table 1 receives no gradient at all)


class _Net(torch.nn.Module):
    def __init__(self, sparse):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(n, 16, sparse=sparse) for n in ROWS])
        self.lin = torch.nn.Linear(32, 1)

    def forward(self, ids, second=True):
        a = self._embedding[0](ids[:, 0])
        b = self._embedding[1](ids[:, 1]) if second else torch.zeros_like(a)
        return self.lin(torch.cat([a, b], 1)).view(-1)


def _clip(params):
    """clip_grad_norm_'s coefficient over dense and sparse gradients alike, applied in place"""
    grads = [p.grad for p in params if p.grad is not None]
    total = torch.sqrt(sum(((g.coalesce().values() if g.is_sparse else g) ** 2).sum() for g in grads))
    coef = torch.clamp(CLIP / (total + 1e-6), max=1.0)
    for g in grads:
        g.mul_(coef)
    return float(coef)


def _train():
    torch.manual_seed(3)
    a = _Net(False).double()
    b = _Net(True).double()
    b.load_state_dict(a.state_dict())
    opt = RowSparseAdam(a.parameters(), list(a._embedding.parameters()), lr=LR)
    sp = torch.optim.SparseAdam(list(b._embedding.parameters()), lr=LR)
    ad = torch.optim.Adam(list(b.lin.parameters()), lr=LR)
    y = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)
    snaps, coefs = [], []
    for k, ids in enumerate(IDS):
        ids = torch.tensor(ids)
        for m in (a, b):
            for p in m.parameters():
                p.grad = None
            torch.nn.functional.binary_cross_entropy_with_logits(m(ids, second=k != NO_TABLE_1), y).backward()
        coefs.append((_clip(list(a.parameters())), _clip(list(b.parameters()))))
        opt.touch(ids)
        opt.step()
        sp.step()
        ad.step()
        snaps.append(copy.deepcopy({n: dict(opt.state[p]) for n, p in a.named_parameters() if p in opt.state}))
    return a, b, opt, sp, ad, snaps, coefs


def _close(x, y, what):
    err = float((x - y).abs().max())
    assert torch.allclose(x, y, rtol=1e-12, atol=0.0), (what, err)


def test_torch_route_equals_sparse_adam_and_adam():
    a, b, opt, sp, ad, snaps, coefs = _train()
    assert all(abs(ca - cb) <= 1e-12 * cb for ca, cb in coefs) and min(c for c, _ in coefs) < 1.0  # (the clip was active)
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        _close(p.detach(), pb[n].detach(), n)
        ref = (sp if n.startswith("_embedding.") else ad).state[pb[n]]
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        _close(st["exp_avg"], ref["exp_avg"], (n, "exp_avg"))
        _close(st["exp_avg_sq"], ref["exp_avg_sq"], (n, "exp_avg_sq"))
        assert float(st["step"]) == float(ref["step"]), n
    assert float(opt.state[a._embedding[0].weight]["step"]) == 4.0 and float(opt.state[a._embedding[1].weight]["step"]) == 3.0
    assert float(opt.state[a.lin.weight]["step"]) == 4.0
    # the row touched at steps 1 and 4 only: its moments rest in between, bit for bit; and it did move at step 1
    e0 = "_embedding.0.weight"
    for key in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(snaps[0][e0][key][6], snaps[2][e0][key][6]) and snaps[0][e0][key][6].abs().sum() > 0
        assert not torch.equal(snaps[2][e0][key][6], snaps[3][e0][key][6])
    # the table without a gradient: counter and state as they were
    e1 = "_embedding.1.weight"
    assert float(snaps[NO_TABLE_1][e1]["step"]) == float(snaps[NO_TABLE_1 - 1][e1]["step"]) == 2.0
    assert torch.equal(snaps[NO_TABLE_1][e1]["exp_avg"], snaps[NO_TABLE_1 - 1][e1]["exp_avg"])


def test_a_touched_row_with_zero_gradient_still_moves():
    """a row counts as touched because its id is in the batch: with a zero summed gradient its moments decay and it moves"""
    w = torch.nn.Parameter(torch.ones(4, 16, dtype=torch.float64))
    opt = RowSparseAdam([w], [w], lr=LR)
    w.grad = torch.zeros_like(w)
    w.grad[1] = 1.0
    opt.touch(torch.tensor([[1], [2]]))
    opt.step()
    w.grad = torch.zeros_like(w)
    before, m0 = w.detach().clone(), opt.state[w]["exp_avg"].clone()
    opt.touch(torch.tensor([[1], [3]]))
    opt.step()
    assert torch.equal(opt.state[w]["exp_avg"][1], m0[1] + (1 - 0.9) * (0 - m0[1])) and not torch.equal(w[1], before[1])
    assert torch.equal(w[0], before[0]) and torch.equal(w[2], before[2]) and torch.equal(w[3], before[3])


def test_step_without_touch_raises():
    w = torch.nn.Parameter(torch.ones(4, 16))
    lin = torch.nn.Parameter(torch.ones(3))
    opt = RowSparseAdam([w, lin], [w], lr=LR)
    w.grad, lin.grad = torch.ones_like(w), torch.ones_like(lin)
    with pytest.raises(RuntimeError, match="touch"):
        opt.step()
    opt.touch(torch.tensor([[0]]))
    opt.step()
    with pytest.raises(RuntimeError, match="touch"):  # the ids were consumed by the step
        opt.step()
    w.grad = None
    opt.step()  # no table gradient: nothing to touch


def test_touch_refuses_ids_outside_a_table():
    """a row-sharded table holds one rank's rows under local ids: the batch's ids do not address it, whoever built the optimizer"""
    w = torch.nn.Parameter(torch.ones(4, 16))
    opt = RowSparseAdam([w], [w], lr=LR)
    for bad in ([[4]], [[-1]], [[0], [9]]):
        with pytest.raises(ValueError, match="outside its table"):
            opt.touch(torch.tensor(bad))
    assert opt._ids is None
    opt.touch(torch.tensor([[3]]))


# ---------------------------------------------------------------------------------------------------------------------------------
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self.ln = torch.nn.LayerNorm(3)
        self._final = torch.nn.Linear(3, 1)

    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


class _DPTiny(_Tiny):
    engine_dp_optimizers = True


def test_optim_spec_of_a_row_sparse_adam():
    m = _Tiny()
    opt = MT.build_optimizer("row-sparse-adam", m, 0.05)
    assert type(opt) is RowSparseAdam and opt.param_groups[0]["lr"] == 0.05 and opt.param_groups[0]["eps"] == 1e-8
    spec = OptimSpec.from_optimizer(opt)
    assert spec == OptimSpec("adam", sparse_rows=True) and spec.moments and spec.state_keys == ("exp_avg", "exp_avg_sq")
    assert OptimSpec.from_optimizer(torch.optim.Adam(m.parameters(), lr=0.05)).sparse_rows is False
    assert OptimSpec.for_step(opt) == spec
    assert OptimSpec.for_step(opt, 1e-3, None) is None and OptimSpec.for_step(opt, 1e-3, "lin") is None
    assert OptimSpec.for_step(opt, 1e-3, "_embedding") == spec._replace(wd=1e-3, no_reg="_embedding")
    assert OptimSpec.of(optim=spec, weight_decay=1e-3, no_reg_param_name="_embedding").sparse_rows is True
    # Adam's disqualifiers hold for it too
    opt.param_groups[0]["amsgrad"] = True
    assert OptimSpec.from_optimizer(opt) is None


def _routes(m):
    opt = MT.build_optimizer("row-sparse-adam", m, 0.05)
    ref = MT.build_optimizer("adam", m, 0.05)
    res = {"wd0": TU._fused_step_applies(m, opt, TU.L2Loss(0.0), False),
           "wd": TU._fused_step_applies(m, opt, TU.L2Loss(1e-3), False),
           "no_reg": TU._fused_step_applies(m, opt, TU.L2Loss(1e-3, "_embedding"), False)}
    m._table_sharding = "row"
    res["row"] = [TU._fused_step_applies(m, o, TU.L2Loss(0.0), False) for o in (opt, ref)]
    m._table_sharding = None
    return res


def test_routing_at_world_1():
    for m in (_Tiny(), _DPTiny()):
        assert _routes(m) == {"wd0": True, "wd": False, "no_reg": True, "row": [False, False]}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _route_worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    from nasrec_amd.utils.dist import assert_replicas_identical
    m = _DPTiny()
    res = dict(dp=_routes(m), plain=_routes(_Tiny()))
    # the start-up agreement: one rank on row-sparse Adam, the other on Adam
    torch.manual_seed(0)
    m = _DPTiny()
    assert_replicas_identical(m, MT.build_optimizer("row-sparse-adam", m, 0.05))
    try:
        assert_replicas_identical(m, MT.build_optimizer("row-sparse-adam" if rank else "adam", m, 0.05))
        res["agreement"] = None
    except RuntimeError as e:
        res["agreement"] = str(e)
    # touch at world 2: the ids of every rank's batch
    opt = MT.build_optimizer("row-sparse-adam", m, 0.05)
    opt.touch(torch.tensor([[rank, rank + 1]]))
    res["ids"] = opt._ids.tolist()
    out[rank] = res
    dist.destroy_process_group()


def test_routing_and_agreement_at_world_2():
    out = mp.Manager().dict()
    mp.spawn(_route_worker, args=(_free_port(), out), nprocs=2, join=True)
    for r in range(2):
        assert out[r]["dp"] == {"wd0": True, "wd": False, "no_reg": True, "row": [False, False]}
        # a model whose fused step has no exchange for the moments keeps the torch route, as with Adam
        assert out[r]["plain"] == {"wd0": False, "wd": False, "no_reg": False, "row": [False, False]}
        assert out[r]["agreement"] is not None and "sparse_rows" in out[r]["agreement"]
        assert out[r]["ids"] == [[0, 1], [1, 2]]


def test_the_harness_refuses_a_regularised_table():
    m = _Tiny()
    opt = MT.build_optimizer("row-sparse-adam", m, 0.05)
    for use in (None, False):
        with pytest.raises(ValueError) as e:
            TU.train_and_test_one_epoch(m, 0, opt, None, [], [], None, TU.L2Loss(1e-3, None), 8, None, use_engine_step=use)
        assert "--no-reg-param-name _embedding" in str(e.value) and "--wd 0" in str(e.value)
    TU._refuse_regularised_tables(opt, TU.L2Loss(1e-3, "_embedding"))
    TU._refuse_regularised_tables(opt, TU.L2Loss(0.0, None))
    TU._refuse_regularised_tables(MT.build_optimizer("adam", m, 0.05), TU.L2Loss(1e-3, None))
    m._table_sharding = "row"
    with pytest.raises(ValueError, match="whole tables"):
        MT.build_optimizer("row-sparse-adam", m, 0.05)


def test_the_four_clis_take_the_choice():
    from nasrec_amd import eval_subnet_from_scratch, eval_subnet_from_supernet, train_supernet
    for mod in (MT, train_supernet, eval_subnet_from_scratch, eval_subnet_from_supernet):
        opts = [a for a in mod.build_parser()._actions if "--optimizer" in a.option_strings]
        assert len(opts) == 1 and "row-sparse-adam" in opts[0].choices and "adam" in opts[0].choices, mod.__name__


def test_layout_check_passes_with_the_grown_descriptor():
    import ctypes as C
    lib = L.load()
    assert lib.nasrec_abi_version() == 17
    sizes = (C.c_int32 * 43)()
    n = lib.nasrec_desc_sizes(sizes, 43)
    assert n > L.OP_OPT_MOMENTS and sizes[L.OP_OPT_MOMENTS] == C.sizeof(L.OptMomentsDesc)
    assert L.OptMomentsDesc.sparse_rows.offset == L.OptMomentsDesc.rank_stride.offset + 8
    assert C.sizeof(L.OptMomentsDesc) == L.OptMomentsDesc.sparse_rows.offset + 8
