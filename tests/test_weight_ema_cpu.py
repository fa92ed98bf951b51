"""`--ema DECAY` without a GPU: utils/optim.WeightEMA against the fp64 rule s <- s + (1 - d)(p - s), its `averaged()` exchange and its
state round trip; the lazy rule of csrc/weight_ema.hip — `lazy_ema_reference`, an fp64 NumPy restatement (catch-up on touch, update,
flush), the reference of the GPU kernel test — against the dense fp64 average; the harness's choice of route with an average; the
spec's appended field; the descriptor's layout; main_train's parser.

The bar (derived, not measured; DESIGN.md "Lazy weight EMA"): against the fp64 average of the same fp32 parameter history, per update
fl(p - s) adds at most 2 * 2^-24 M, the multiply-add one rounding 2^-24 M (two where a route does not fuse it, which 6 per update still
covers: 2 + 2 + 2 w < 6), w = (float)(1 - d) against 1 - d at most 2 * 2^-24 M w, earlier error contracts by d, a catch-up is one
rounding of an fp64 result: (6 T + 2) 2^-24 M per element, M = the largest |p| or |s| of that element's history."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import OptimSpec
from nasrec_amd.utils import train_utils as TU
from nasrec_amd.utils.optim import WeightEMA
from test_rmsprop_kernel_gpu import IDS as RMSPROP_IDS
from test_rmsprop_kernel_gpu import ROWS as RMSPROP_ROWS


def ema_bar(T, M):
    """the derived bound on |fp32 average - fp64 average| after T updates, per element (M: array or scalar)"""
    return (6 * T + 2) * 2.0 ** -24 * M


def dense_ema_fp64(history, s0, decay):
    """s after averaging history[0], history[1], ... (fp64 arrays of one shape) from s0 -> (s, M = max |p| or |s| per element)"""
    s = np.asarray(s0, np.float64).copy()
    M = np.abs(s)
    for p in history:
        p = np.asarray(p, np.float64)
        s = s + (1.0 - decay) * (p - s)
        M = np.maximum(M, np.maximum(np.abs(p), np.abs(s)))
    return s, M


def lazy_ema_catch_up(p, s, stamp, count, rows, decay):
    """phase 0 on one table, fp64: the given rows pay what they owe since their stamp and are stamped `count`"""
    for r in rows:
        n = count - int(stamp[r])
        if n > 0:
            s[r] = p[r] + decay ** n * (s[r] - p[r])
            stamp[r] = count


def lazy_ema_update(p, s, stamp, count, rows, decay):
    """phase 1 on one table, fp64: the dense statement on the given (current) rows, stamped count + 1 -> count + 1"""
    for r in rows:
        assert stamp[r] == count, "phase 1 finds the batch's rows current"
        s[r] = s[r] + (1.0 - decay) * (p[r] - s[r])
        stamp[r] = count + 1
    return count + 1


def lazy_ema_flush(p, s, stamp, count, decay):
    owed = (count - stamp) > 0
    k = (decay ** (count - stamp[owed]).astype(np.float64))[:, None]
    s[owed] = p[owed] + k * (s[owed] - p[owed])
    stamp[owed] = count


def lazy_ema_reference(p, s, stamp, count, rows, move, decay):
    """One step of the lazy average on one table, fp64, as the launches do it: catch-up of the batch's `rows`, then `move(p, rows)`
    (the optimizer: it changes those rows of p in place and no other), then the update.  -> the new count"""
    lazy_ema_catch_up(p, s, stamp, count, rows, decay)
    move(p, rows)
    return lazy_ema_update(p, s, stamp, count, rows, decay)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._embedding = torch.nn.ModuleList([torch.nn.Embedding(7, 16), torch.nn.Embedding(5, 16)])
        self.lin = torch.nn.Linear(4, 3)
        self.ln = torch.nn.LayerNorm(3)
        self._final = torch.nn.Linear(3, 1)

    def engine_train_step(self, *a, **k):
        raise AssertionError("not called here")


def _perturb(m, g):
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n != "ln.bias":  # (a parameter that never moves is averaged all the same)
                p.add_(0.1 * torch.randn(p.shape, generator=g))


def test_weight_ema_against_fp64():
    T, decay = 6, 0.9
    g = torch.Generator().manual_seed(5)
    m = _Tiny()
    _perturb(m, g)
    ema = WeightEMA(m, decay)
    assert ema.num_updates == 0 and set(ema.shadow) == {n for n, _ in m.named_parameters()}
    s0 = {n: p.detach().double().numpy().copy() for n, p in m.named_parameters()}
    assert all(torch.equal(ema.shadow[n], p) and ema.shadow[n].data_ptr() != p.data_ptr() for n, p in m.named_parameters())
    hist = {n: [] for n in s0}
    for _ in range(T):
        _perturb(m, g)
        ema.update()
        for n, p in m.named_parameters():
            hist[n].append(p.detach().double().numpy().copy())
    assert ema.num_updates == T
    for n in s0:
        want, M = dense_ema_fp64(hist[n], s0[n], decay)
        err = np.abs(ema.shadow[n].double().numpy() - want)
        assert (err <= ema_bar(T, M)).all(), (n, float((err / np.maximum(ema_bar(T, M), 1e-300)).max()))
        assert n == "ln.bias" or not torch.equal(ema.shadow[n], dict(m.named_parameters())[n])
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            WeightEMA(m, bad)


def test_averaged_exchanges_and_restores_bit_for_bit():
    g = torch.Generator().manual_seed(6)
    m = _Tiny()
    ema = WeightEMA(m, 0.99)
    for _ in range(3):
        _perturb(m, g)
        ema.update()
    p0 = {n: p.detach().clone() for n, p in m.named_parameters()}
    s0 = {n: s.clone() for n, s in ema.shadow.items()}
    with ema.averaged() as inside:
        assert inside is m
        for n, p in m.named_parameters():
            assert torch.equal(p, s0[n]) and torch.equal(ema.shadow[n], p0[n]), n
        with pytest.raises(RuntimeError):
            ema.update()
        with pytest.raises(RuntimeError):
            with ema.averaged():
                pass
    for n, p in m.named_parameters():
        assert torch.equal(p, p0[n]) and torch.equal(ema.shadow[n], s0[n]), n
    assert ema.num_updates == 3
    ema.update()  # (and outside it works again)
    assert ema.num_updates == 4


def test_state_round_trip():
    g = torch.Generator().manual_seed(7)
    m = _Tiny()
    ema = WeightEMA(m, 0.9)
    for _ in range(2):
        _perturb(m, g)
        ema.update()
    sd = ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow"} and sd["decay"] == 0.9 and sd["num_updates"] == 2
    assert all(sd["shadow"][n].data_ptr() != s.data_ptr() for n, s in ema.shadow.items())
    other = WeightEMA(_Tiny(), 0.5)
    other.load_state_dict(sd)
    assert other.decay == 0.9 and other.num_updates == 2
    for n, s in ema.shadow.items():
        assert torch.equal(other.shadow[n], s), n
    # hooks of a bound average: the flush runs first in state_dict() and update(), the exchange is the engine's
    calls = []
    ema._hooks = dict(flush=lambda: calls.append("flush"), swap=lambda: calls.append("swap"), advance=lambda: calls.append("advance"))
    ema.state_dict()
    ema.update()
    with ema.averaged():
        pass
    assert calls == ["flush", "flush", "advance", "swap", "swap"] and ema.num_updates == 3


def test_the_lazy_rule_with_the_flush_is_the_dense_average():
    """the touch schedule of test_rmsprop_kernel_gpu.py (tables of 1, 65 and 130 rows, six steps, ids outside their table among them):
    table 1's row 1 is never touched, table 2's row 129 at steps 1, 2 and 6.  In fp64 the lazy rule with the flush and the dense
    average differ by rounding alone — far below the fp32 bar, which a wrong power or a stamp off by one exceeds (1 - d = 1e-2)."""
    decay, T, count0 = 0.99, 6, 4
    rng = np.random.default_rng(1)
    for f, R in enumerate(RMSPROP_ROWS):
        p = rng.standard_normal((R, 16))
        s = p + 0.1 * rng.standard_normal((R, 16))
        pl, sl, stamp, count = p.copy(), s.copy(), np.full(R, count0, np.int64), count0
        s_dense, hist, touched_at = s.copy(), [], {}

        def move(pp, rows):
            for r in rows:
                pp[r] += 0.05 * rng.standard_normal(16)
        for t in range(T):
            rows = sorted({b[f] for b in RMSPROP_IDS[t] if 0 <= b[f] < R})
            for r in rows:
                touched_at.setdefault(r, []).append(t + 1)
            before = (pl.copy(), sl.copy(), stamp.copy())
            count = lazy_ema_reference(pl, sl, stamp, count, rows, move, decay)
            rest = np.ones(R, bool)
            rest[rows] = False
            assert all(np.array_equal(x[rest], y[rest]) for x, y in zip(before, (pl, sl, stamp))), (f, t)
            hist.append(pl.copy())
            s_dense = s_dense + (1.0 - decay) * (pl - s_dense)
        if f == 1:
            assert 1 not in touched_at and stamp[1] == count0
        if f == 2:
            assert touched_at[129] == [1, 2, 6]
        assert count == count0 + T
        behind = stamp < count
        if behind.any():
            assert np.abs(sl - s_dense)[behind].max() > 1e-4  # (before the flush the resting rows are behind)
        lazy_ema_flush(pl, sl, stamp, count, decay)
        assert (stamp == count).all()
        want, M = dense_ema_fp64(hist, s, decay)
        assert np.array_equal(want, s_dense)
        assert (np.abs(sl - want) <= 1e-6 * ema_bar(T, M)).all()
        again = sl.copy()
        lazy_ema_flush(pl, sl, stamp, count, decay)
        assert np.array_equal(again, sl)


def test_routing_with_an_average():
    m = _Tiny()
    ema = WeightEMA(m, 0.9)
    no_wd, dense_wd, table_wd = TU.L2Loss(0.0), TU.L2Loss(1e-8, "_embedding"), TU.L2Loss(1e-8)
    for name in ("adagrad", "row-sparse-adam", "rmsprop"):
        opt = MT.build_optimizer(name, m, 0.05)
        for l2 in (no_wd, dense_wd):
            plain = TU._fused_step_spec(m, opt, l2, False)
            with_ema = TU._fused_step_spec(m, opt, l2, False, ema=ema)
            assert plain is not None and plain.ema == 0.0 and with_ema == plain._replace(ema=0.9), name
            assert TU._fused_step_applies(m, opt, l2, False, ema) is True
        assert TU._fused_step_spec(m, opt, table_wd, False, ema=ema) is None, name  # weight decay reaches a table
        assert TU._fused_step_spec(m, opt, no_wd, True, ema=ema) is None, name     # AMP
    for name in ("adam", "sgd"):
        opt = MT.build_optimizer(name, m, 0.05)
        assert TU._fused_step_spec(m, opt, no_wd, False) is not None
        assert TU._fused_step_spec(m, opt, no_wd, False, ema=ema) is None, name
        assert "every table row" in TU._ema_route(m, TU._fused_step_spec(m, opt, no_wd, False), no_wd)
    opt = MT.build_optimizer("adagrad", m, 0.05)
    m._place_embedding_on_cpu = True
    assert TU._fused_step_spec(m, opt, no_wd, False, ema=ema) is None
    m._place_embedding_on_cpu = False
    m._table_sharding = "row"
    assert TU._fused_step_spec(m, opt, no_wd, False) is not None  # (Adagrad without weight decay trains row-sharded tables fused)
    assert TU._fused_step_spec(m, opt, no_wd, False, ema=ema) is None
    m._table_sharding = None
    # ema=None: every answer is the one the three-argument form gives
    for name in ("adagrad", "adam", "sgd", "row-sparse-adam", "rmsprop"):
        opt = MT.build_optimizer(name, m, 0.05)
        for l2 in (no_wd, dense_wd, table_wd):
            for amp in (False, True):
                assert TU._fused_step_spec(m, opt, l2, amp, ema=None) == TU._fused_step_spec(m, opt, l2, amp), (name, amp)


def test_spec_default():
    assert OptimSpec._fields[-1] == "ema" and OptimSpec._field_defaults["ema"] == 0.0
    assert OptimSpec("adagrad", eps=1e-2)._replace() == OptimSpec("adagrad", eps=1e-2, ema=0.0)
    assert OptimSpec("adam") == OptimSpec("adam", 0.9, 0.999, 1e-8, 0.0, False, 0.0, None, False, 0.99)
    assert OptimSpec.of(1e-2) == OptimSpec("adagrad", eps=1e-2) and OptimSpec.of(1e-2).ema == 0.0
    assert OptimSpec.of(1e-2, ema=0.99) == OptimSpec("adagrad", eps=1e-2, ema=0.99) != OptimSpec.of(1e-2)
    rms = OptimSpec("rmsprop", alpha=0.9)
    assert OptimSpec.of(optim=rms, ema=0.5) == rms._replace(ema=0.5)
    assert OptimSpec.of(optim=rms._replace(ema=0.5)).ema == 0.5
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            OptimSpec.of(1e-2, ema=bad)


def test_descriptor_layout_matches_the_header():
    lib = L.load()
    assert lib.nasrec_abi_version() == 17
    sizes = (C.c_int32 * 44)()
    n = lib.nasrec_desc_sizes(sizes, 44)
    assert n == 44 and L.OP_WEIGHT_EMA == 43 and sizes[43] == C.sizeof(L.WeightEmaDesc)
    assert L.DESC_BY_KIND[L.OP_WEIGHT_EMA] is L.WeightEmaDesc and hasattr(lib, "nasrec_weight_ema")
    D = L.WeightEmaDesc
    assert D.decay.offset == 24 and D.idx.offset == 32 and D.table.offset == 48
    assert D.shadow.offset == D.table.offset + 8 * L.MAX_TABLES and D.stamp.offset == D.shadow.offset + 8 * L.MAX_TABLES
    assert D.tile_off.offset == D.rows.offset + 8 * L.MAX_TABLES and D.bitmap.offset == D.tile_off.offset + 8 * (L.MAX_TABLES + 1)
    assert C.sizeof(D) == D.counter.offset + 8


def test_main_train_parser():
    p = MT.build_parser()
    assert p.parse_args([]).ema == 0.0 and p.parse_args(["--ema", "0.99"]).ema == 0.99
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit):
            p.parse_args(["--ema", bad])
    assert "not implemented" not in p.format_help()
