"""`--cowclip R[,ZETA]` without a GPU: utils/optim.CowClip against a plain per-row loop in fp64, its counts with duplicates and ids
outside the tables, the flag's parser in the three CLIs, every start-up refusal by the flag's name, the route line, the binding's
layout and the scheduler's footprints of NASREC_OP_COWCLIP.  (tests/_dry_engine.py is an fp64 oracle engine: it composes no optimizer
tail, so the launch list is checked on the GPU, tests/test_cowclip_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import eval_subnet_from_scratch as ES
from nasrec_amd import main_train as MT
from nasrec_amd import schedule as S
from nasrec_amd import train_supernet as TS
from nasrec_amd.optim_spec import TABLE_RULES, OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import CowClip, parse_cowclip

ROWS = [40, 7, 1]


def _tables(seed=0, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(scale * torch.randn(n, 16, generator=g)) for n in ROWS]


def _ids(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randint(0, n, (B,), generator=g) for n in ROWS], 1)
    ids[0, 0], ids[1, 0], ids[2, 1], ids[3, 1] = -1, ROWS[0], ROWS[1] + 3, ids[4, 1]  # outside the tables, and a duplicate
    return ids


def _restate(tables, grads, ids, r, zeta):
    """the rule, one row at a time, in fp64 -> (new gradients, touched, clipped, ratios G / T)"""
    out = [g.double().numpy().copy() for g in grads]
    touched = clipped = 0
    ratios = []
    r32, z32 = float(np.float32(r)), float(np.float32(zeta))
    for f, w in enumerate(tables):
        col = [int(v) for v in ids[:, f] if 0 <= int(v) < w.shape[0]]
        for k in sorted(set(col)):
            cnt = col.count(k)
            g, wk = grads[f][k].double().numpy(), w[k].detach().double().numpy()
            G, T = np.sqrt((g * g).sum()), cnt * max(r32 * np.sqrt((wk * wk).sum()), z32)
            touched += 1
            ratios.append(G / T)
            if G > T:
                clipped += 1
                out[f][k] = g * (T / G)
    return out, touched, clipped, ratios


@pytest.mark.parametrize("r,zeta", [(1.0, 1e-5), (0.05, 1e-5), (1.0, 0.5)])
@pytest.mark.parametrize("B", [1, 8, 64])
def test_apply_against_a_per_row_loop_in_fp64(B, r, zeta):
    tables = _tables()
    ids = _ids(max(B, 5))[:B] if B >= 5 else torch.tensor([[3, 2, 0]])
    g = torch.Generator().manual_seed(7 + B)
    with torch.no_grad():
        tables[0][5] = 0.0  # (a row of zero weights: zeta is its threshold)
    grads = []
    for f, w in enumerate(tables):
        # the gradients' scale spans the thresholds: rows on both sides of them
        scale = torch.exp(torch.empty(w.shape[0], 1).uniform_(-2.5, 2.5, generator=g)) * max(r * 0.4, zeta)
        grads.append(scale * torch.randn(w.shape, generator=g))
    grads[0][int(ids[-1, 0])] = 0.0 if 0 <= int(ids[-1, 0]) < ROWS[0] else grads[0][0]
    for w, gr in zip(tables, grads):
        w.grad = gr.clone()
    want, touched, clipped, ratios = _restate(tables, grads, ids, r, zeta)
    assert all(abs(v - 1.0) > 1e-3 for v in ratios), "a row sits on its threshold: choose another seed"
    cc = CowClip(tables, r, zeta)
    before = [w.detach().clone() for w in tables]
    assert cc.apply(ids) == (touched, clipped) and (cc.touched, cc.clipped) == (touched, clipped)
    if B >= 8:
        assert 0 < clipped < touched
    for f, w in enumerate(tables):
        assert torch.equal(w.detach(), before[f])  # (the weights are read only)
        err = np.abs(w.grad.double().numpy() - want[f])
        assert (err <= 2e-7 + 2e-6 * np.abs(want[f])).all(), f
        rows = {int(v) for v in ids[:, f] if 0 <= int(v) < w.shape[0]}
        rest = torch.tensor([k not in rows for k in range(w.shape[0])])
        assert torch.equal(w.grad[rest], grads[f][rest])  # rows outside the batch: their bits
    # unclipped rows keep their bits too
    for f, w in enumerate(tables):
        for k in range(w.shape[0]):
            if np.array_equal(want[f][k], grads[f][k].double().numpy()):
                assert torch.equal(w.grad[k], grads[f][k]), (f, k)
    assert cc.apply(ids)[0] == touched and cc.touched == 2 * touched


def test_counts_with_duplicates_and_ids_outside_the_tables():
    tables = _tables()
    cc = CowClip(tables)
    assert (cc.r, cc.zeta) == (1.0, 1e-5)
    ids = torch.tensor([[3, 2, 0], [3, 6, 0], [-1, 7, 0], [40, 2, 1], [3, -5, 0], [39, 2, 0]])
    got = [tuple(t.tolist() for t in cc.rows(ids, f)) for f in range(3)]
    assert got == [([3, 39], [3, 1]), ([2, 6], [3, 1]), ([0], [5])]
    # cnt scales the threshold: one row, the same gradient, seen once and three times
    w = tables[0]
    for n, clipped in ((1, 1), (3, 0)):
        for t in tables:
            t.grad = torch.zeros_like(t)
        w.grad[3] = w[3].detach() * 2.0  # G = 2 |w|: over |w|, under 3 |w|
        assert cc.apply(torch.tensor([[3, 0, 0]] * n)) == (3, clipped)
        assert torch.equal(w.grad[3], w[3].detach() * 2.0) == (not clipped)
    # a zero and a NaN gradient are never clipped; a table without a gradient is skipped
    for t in tables:
        t.grad = torch.zeros_like(t)
    w.grad[4, 2] = float("nan")
    tables[2].grad = None
    assert cc.apply(torch.tensor([[4, 1, 0], [5, 1, 0]])) == (3, 0)
    assert torch.isnan(w.grad[4, 2]) and not w.grad[5].any()
    with pytest.raises(ValueError, match="ids of shape"):
        cc.apply(torch.zeros(4, 2, dtype=torch.long))


def test_the_flag_parser():
    assert parse_cowclip(None) is None and parse_cowclip("") is None
    assert parse_cowclip("1") == (1.0, 1e-5) and parse_cowclip("0.5,1e-4") == (0.5, 1e-4) and parse_cowclip("0") == (0.0, 1e-5)
    for bad in ("x", "1,2,3", "-1", "1,0", "1,-1e-5", "nan", "1,nan", "inf", ","):
        with pytest.raises(ValueError, match="--cowclip"):
            parse_cowclip(bad)
    with pytest.raises(ValueError, match="--cowclip"):
        CowClip(_tables(), r=-1.0)
    for mod in (MT, TS, ES):
        p = mod.build_parser()
        assert p.parse_args([]).cowclip is None  # absent: off
        assert p.parse_args(["--cowclip", "0.5"]).cowclip == (0.5, 1e-5)
        assert p.parse_args(["--cowclip", "1,1e-3"]).cowclip == (1.0, 1e-3)
        for bad in ("-1", "1,0", "a,b"):
            with pytest.raises(SystemExit):
                p.parse_args(["--cowclip", bad])
        assert MT.build_cowclip(p.parse_args([]), None) is None


class _Tiny(torch.nn.Module):
    """test_weight_ema_cpu.py's stand-in for a SuperNet in the routing questions"""

    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self._final = torch.nn.Linear(3, 1)

    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


def test_every_refusal_names_the_flag(monkeypatch):
    from nasrec_amd.utils import dist
    m = _Tiny()
    opt = MT.build_optimizer("adagrad", m, 0.05)
    no_wd = TU.L2Loss(0.0)
    TU.refuse_cowclip(m, opt, no_wd)                               # nothing to refuse
    TU.refuse_cowclip(m, opt, TU.L2Loss(1e-8, "_embedding"))       # an L2 term that leaves the tables out
    with pytest.raises(ValueError, match="--cowclip.*--wd"):       # a regularised table
        TU.refuse_cowclip(m, opt, TU.L2Loss(1e-8))
    with pytest.raises(ValueError, match="--cowclip.*bf16"):       # bf16 tables
        TU.refuse_cowclip(m, opt, no_wd, table_dtype="bf16")
    bf = MT.build_optimizer("adam-adagrad-tables", m, 1e-3, table_rowwise=True)
    bf.__class__ = type("Bf16", (type(bf),), {"bf16_tables": property(lambda self: True)})
    with pytest.raises(ValueError, match="--cowclip.*bf16"):
        TU.refuse_cowclip(m, bf, no_wd)
    m._place_embedding_on_cpu = True
    with pytest.raises(ValueError, match="--cowclip.*host"):       # host embedding
        TU.refuse_cowclip(m, opt, no_wd)
    m._place_embedding_on_cpu = False
    m._table_sharding = "row"
    with pytest.raises(ValueError, match="--cowclip.*--table-sharding row"):
        TU.refuse_cowclip(m, opt, no_wd)
    m._table_sharding = None
    with pytest.raises(ValueError, match="--cowclip.*last-layer"):
        TU.refuse_cowclip(m, opt, no_wd, last_layer_step=True)
    monkeypatch.setenv("NASREC_PERSIST_DEFAULT", "1")
    with pytest.raises(ValueError, match="--cowclip.*persistent"):
        TU.refuse_cowclip(m, opt, no_wd)
    monkeypatch.delenv("NASREC_PERSIST_DEFAULT")
    monkeypatch.setattr(dist, "world_info", lambda: (0, 2))
    with pytest.raises(ValueError, match="--cowclip.*world size of 2"):
        TU.refuse_cowclip(m, opt, no_wd)
    monkeypatch.setattr(dist, "world_info", lambda: (0, 1))
    # train_and_test_one_epoch asks before it touches a loader
    with pytest.raises(ValueError, match="--cowclip"):
        TU.train_and_test_one_epoch(m, 0, opt, None, None, None, None, TU.L2Loss(1e-8), 8, None, cowclip=CowClip(list(m._embedding.parameters())))
    # the CLIs' start-up check, from the flags alone
    p = MT.build_parser()
    MT.check_cowclip(p.parse_args(["--wd", "1e-8"]))  # (no flag: nothing is asked)
    MT.check_cowclip(p.parse_args(["--cowclip", "1", "--wd", "0"]))
    MT.check_cowclip(p.parse_args(["--cowclip", "1", "--wd", "1e-8", "--no-reg-param-name", "_embedding"]))
    for extra, word in ((["--wd", "1e-8"], "--wd"), (["--wd", "0", "--table-sharding", "row"], "--table-sharding row"),
                        (["--wd", "0", "--table-dtype", "bf16"], "bf16")):
        with pytest.raises(ValueError, match="--cowclip.*" + word):
            MT.check_cowclip(p.parse_args(["--cowclip", "1"] + extra))
    with pytest.raises(ValueError, match="--cowclip.*world size of 4"):
        MT.check_cowclip(p.parse_args(["--cowclip", "1", "--wd", "0"]), world=4)
    with pytest.raises(ValueError, match="--cowclip.*last-layer"):
        MT.check_cowclip(p.parse_args(["--cowclip", "1", "--wd", "0"]), last_layer=True)


def test_the_route_line(capsys):
    cc = CowClip(_tables(), 0.5, 1e-4)
    TU._announce_cowclip_route(cc, True)
    TU._announce_cowclip_route(cc, True)  # once per run
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "CowClip (r 0.5, zeta 0.0001): fused step" in out
    for kw, why in ((dict(), "the fused step does not apply"), (dict(use_amp=True), "AMP keeps the torch route"),
                    (dict(switched_off=True), "the fused step was switched off")):
        TU._announce_cowclip_route(CowClip(_tables()), False, **kw)
        out = capsys.readouterr().out
        assert "torch route, CowClip.apply() before every step" in out and why in out


def test_the_feature_changes_no_pinned_record():
    assert len(TABLE_RULES) == 8 and "cowclip" not in OptimSpec._fields and not any("cow" in f for f in OptimSpec._fields)
    lib = L.load()
    assert lib.nasrec_abi_version() == 17
    sizes = (C.c_int32 * 46)()
    assert lib.nasrec_desc_sizes(sizes, 46) == 46
    assert L.OP_COWCLIP == 45 and L.DESC_BY_KIND[L.OP_COWCLIP] is L.CowClipDesc and sizes[45] == C.sizeof(L.CowClipDesc) == 864
    assert L.CowClipDesc.clip.offset == 816 and L.CowClipDesc.stat.offset == 856 and L.CowClipDesc.cnt.offset == 304
    assert sizes[L.OP_OPT_MOMENTS] == 1568 and sizes[L.OP_DECOUPLED_DECAY] == C.sizeof(L.DecoupledDecayDesc)  # (as before)


def _desc(phase):
    d = L.CowClipDesc()
    d.kind, d.phase, d.B, d.Fs = L.OP_COWCLIP, phase, 4, 2
    d.idx, d.leader, d.gsum = 4096, 8192, 12288
    for f in range(2):
        d.table[f], d.cnt[f], d.rows[f] = 100000 * (f + 1), 500000 * (f + 1), 10
    d.clip.n_a, d.clip.partial_a, d.clip.out, d.stat = 2, 900000, 910000, 920000
    return d


def test_the_schedulers_footprints():
    key = lambda accs: sorted((a.ptr, a.width) for a in accs)
    R0, W0 = S.desc_io(_desc(0))
    assert key(W0) == [(500000, 40), (1000000, 40)] and key(R0) == [(4096, 64), (500000, 40), (1000000, 40)]
    R1, W1 = S.desc_io(_desc(1))
    assert key(W1) == sorted([(500000, 40), (1000000, 40), (12288, 512), (910000, 8), (920000, 8)])
    assert key(R1) == sorted([(4096, 64), (8192, 32), (900000, 8), (100000, 640), (200000, 640), (500000, 40), (1000000, 40), (12288, 512),
                              (920000, 8)])
    # the clip launch follows the count launch (RAW on the counts) and whatever wrote gsum; two count launches stay in order
    nodes = S.expand([_desc(0), _desc(1)])
    assert S._depends(nodes[1], nodes[0]) and S._depends(S.expand([_desc(0), _desc(0)])[1], nodes[0])
