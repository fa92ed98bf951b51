"""NASREC_OP_WEIGHT_EMA (include/nasrec_hip.h, csrc/weight_ema.hip) through the C-ABI, after test_rmsprop_kernel_gpu.py: six steps of
catch-up (phase 0), a torch perturbation of the batch's rows and of the dense arena standing in for the optimizer, and update (phase 1);
then the flush (phase 2) and the exchange (phase 3), against the dense fp64 average of the recorded parameter history under the
derived bar of test_weight_ema_cpu.py.

Tables of 1, 65 and 130 rows (64-row tiles: a last tile of 1 and of 2 rows, one exact tile boundary), B = 5 with a duplicate id, a
non-leader pair and the ids -1 and rows[f] (the touch schedule of test_rmsprop_kernel_gpu.py); a guard row on either side of every table,
shadow and stamp array; a dense arena of 2080 floats averaged whole and over its first 1027 (a tail that is no float4 multiple).
decay 0.99, the count starts at 4 with every stamp there.  Row 0 of table 0 is in every batch, and dense elements [0, 16) are fed its
weights: same history, same bits (n = 0 skips the fp64 catch-up)."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from test_rmsprop_kernel_gpu import IDS, ROWS
from test_weight_ema_cpu import dense_ema_fp64, ema_bar

pytestmark = pytest.mark.gpu

FS, B, T = 3, 5, 6
N_ARENA = 2080
DECAY, COUNT0 = 0.99, 4


def _leaders(idx):
    leader = torch.zeros(B, FS, dtype=torch.int32)
    for f in range(FS):
        seen = set()
        for b in range(B):
            if int(idx[b, f]) not in seen:
                leader[b, f] = 1
                seen.add(int(idx[b, f]))
    return leader


def _touched(t, f):
    return sorted({b[f] for b in IDS[t] if 0 <= b[f] < ROWS[f]})


class _Device:
    """the arrays of one run on the device (tables, shadows and stamps with a guard row before and behind) and the descriptor"""

    def __init__(self, n_dense, dense_blocks=3, nblocks=1):
        dev = torch.device("cuda", 0)
        g = torch.Generator().manual_seed(31)
        self.n_dense = n_dense
        self.big_t = [torch.randn(n + 2, 16, generator=g).to(dev) for n in ROWS]
        self.big_s = [torch.randn(n + 2, 16, generator=g).to(dev) for n in ROWS]
        self.big_stamp = [torch.full((n + 2,), COUNT0, dtype=torch.int32, device=dev) for n in ROWS]
        self.tables = [x[1:-1] for x in self.big_t]
        self.shadow = [x[1:-1] for x in self.big_s]
        self.stamp = [x[1:-1] for x in self.big_stamp]
        self.p = torch.randn(N_ARENA, generator=g).to(dev)
        self.s = torch.randn(N_ARENA, generator=g).to(dev)
        self.p[:16] = self.tables[0][0]
        self.s[:16] = self.shadow[0][0]
        self.idx = torch.zeros(B, FS, dtype=torch.int64, device=dev)
        self.leader = torch.zeros(B, FS, dtype=torch.int32, device=dev)
        self.bitmap = torch.zeros(sum(2 * ((n + 63) // 64) for n in ROWS), dtype=torch.int32, device=dev)
        self.count = torch.tensor([COUNT0], dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        d = self.d = L.WeightEmaDesc()
        d.kind, d.phase, d.B, d.Fs, d.decay = L.OP_WEIGHT_EMA, 0, B, FS, DECAY
        d.dense_blocks, d.nblocks = dense_blocks, nblocks
        d.idx, d.leader = self.idx.data_ptr(), self.leader.data_ptr()
        tile = 0
        for f in range(FS):
            d.table[f], d.shadow[f], d.stamp[f], d.rows[f] = self.tables[f].data_ptr(), self.shadow[f].data_ptr(), self.stamp[f].data_ptr(), ROWS[f]
            d.tile_off[f] = tile
            tile += (ROWS[f] + 63) // 64
        d.tile_off[FS] = tile
        d.bitmap, d.p, d.s, d.n = self.bitmap.data_ptr(), self.p.data_ptr(), self.s.data_ptr(), n_dense
        d.count, d.counter = self.count.data_ptr(), self.counter.data_ptr()

    def launch(self, phase, d=None):
        d = L.WeightEmaDesc.from_buffer_copy(self.d if d is None else d)
        if phase is not None:
            d.phase = phase
        rc = L.load().nasrec_weight_ema(torch.cuda.current_stream().cuda_stream, C.addressof(d))
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return dict(tables=[x.cpu() for x in self.big_t], shadow=[x.cpu() for x in self.big_s], stamp=[x.cpu() for x in self.big_stamp],
                    p=self.p.cpu(), s=self.s.cpu(), count=int(self.count.cpu()[0]), counter=int(self.counter.cpu()[0]),
                    bitmap=self.bitmap.cpu())


def _same(a, b):
    for k in a:
        if isinstance(a[k], list):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _steps(dev, snaps=None):
    """six steps on `dev`: catch-up, the optimizer's stand-in (the batch's rows and the dense arena move), update"""
    g = torch.Generator().manual_seed(32)
    for t in range(T):
        idx = torch.tensor(IDS[t], dtype=torch.int64)
        dev.idx.copy_(idx)
        dev.leader.copy_(_leaders(idx))
        assert dev.launch(0) == 0, L.load().nasrec_last_error()
        for f in range(FS):
            for r in _touched(t, f):
                dev.tables[f][r] += (0.05 * torch.randn(16, generator=g)).to(dev.p.device)
        dev.p += (0.05 * torch.randn(N_ARENA, generator=g)).to(dev.p.device)
        dev.p[:16] = dev.tables[0][0]
        assert dev.launch(1) == 0, L.load().nasrec_last_error()
        if snaps is not None:
            snaps.append(dev.snapshot())


def _six_steps(n_dense, **grid):
    """-> the device, [snapshot before the first step and after each step], the snapshots after the flush and after a second flush"""
    dev = _Device(n_dense, **grid)
    snaps = [dev.snapshot()]
    _steps(dev, snaps)
    assert dev.launch(2) == 0, L.load().nasrec_last_error()
    flushed = dev.snapshot()
    assert dev.launch(2) == 0
    return dev, snaps, flushed, dev.snapshot()


@pytest.fixture(scope="module")
def runs():
    return {n: _six_steps(n) for n in (N_ARENA, 1027)}


@pytest.mark.parametrize("n_dense", [N_ARENA, 1027])
def test_six_steps_and_a_flush_against_the_dense_average_in_fp64(runs, n_dense):
    dev, snaps, flushed, again = runs[n_dense]
    worst = 0.0
    # the dense arena: every element of [0, n) every step; the rest keeps its bits
    want, M = dense_ema_fp64([s["p"][:n_dense].double().numpy() for s in snaps[1:]], snaps[0]["s"][:n_dense].double().numpy(), DECAY)
    err = np.abs(flushed["s"][:n_dense].double().numpy() - want)
    assert (err <= ema_bar(T, M)).all(), ("dense", float((err / ema_bar(T, M)).max()))
    worst = max(worst, float((err / ema_bar(T, M)).max()))
    assert torch.equal(flushed["s"][n_dense:], snaps[0]["s"][n_dense:])
    assert torch.equal(flushed["p"], snaps[-1]["p"])  # (p is only read)
    for f in range(FS):
        # before the flush: a row outside the batch keeps its shadow bits and its stamp; the batch's rows are stamped with the count
        for t in range(T):
            rest = torch.ones(ROWS[f] + 2, dtype=torch.bool)
            rest[[r + 1 for r in _touched(t, f)]] = False
            for key in ("shadow", "stamp"):
                assert torch.equal(snaps[t + 1][key][f][rest], snaps[t][key][f][rest]), (key, f, t)
            assert all(int(snaps[t + 1]["stamp"][f][r + 1]) == COUNT0 + t + 1 for r in _touched(t, f)), (f, t)
            assert snaps[t + 1]["count"] == COUNT0 + t + 1 and snaps[t + 1]["counter"] == 0
        never = [r for r in range(ROWS[f]) if all(r not in _touched(t, f) for t in range(T))]
        assert f == 0 or never
        for r in never:
            assert torch.equal(snaps[-1]["shadow"][f][r + 1], snaps[0]["shadow"][f][r + 1]) and int(snaps[-1]["stamp"][f][r + 1]) == COUNT0
        # after the flush: the dense fp64 average of the recorded history, on every row
        want, M = dense_ema_fp64([s["tables"][f][1:-1].double().numpy() for s in snaps[1:]], snaps[0]["shadow"][f][1:-1].double().numpy(), DECAY)
        err = np.abs(flushed["shadow"][f][1:-1].double().numpy() - want)
        assert (err <= ema_bar(T, M)).all(), ("table", f, float((err / ema_bar(T, M)).max()))
        worst = max(worst, float((err / ema_bar(T, M)).max()))
        assert (flushed["stamp"][f][1:-1] == COUNT0 + T).all()
        assert torch.equal(flushed["tables"][f], snaps[-1]["tables"][f])  # (the flush moves no weight)
        # ids -1 and rows[f] wrote nothing: the guard rows keep their bits in all three arrays, through every launch
        for key in ("tables", "shadow", "stamp"):
            for s in snaps + [flushed]:
                assert torch.equal(s[key][f][0], snaps[0][key][f][0]) and torch.equal(s[key][f][-1], snaps[0][key][f][-1]), (key, f)
    print("largest error as a fraction of the bar: %.3f" % worst)
    assert flushed["count"] == COUNT0 + T == 10 and flushed["counter"] == 0 and int(flushed["bitmap"].abs().sum()) == 0
    # the flush had something to pay, the row touched at steps 1, 2 and 6 did not owe (stamps 5, 6, 6, 6, 6, 10)
    assert not torch.equal(flushed["shadow"][2], snaps[-1]["shadow"][2])
    assert [int(s["stamp"][2][130]) for s in snaps] == [4, 5, 6, 6, 6, 6, 10]
    # a row in every batch has the bits of a dense element fed the same weights: n = 0 skips the fp64 catch-up
    assert all(0 in _touched(t, 0) for t in range(T))
    assert torch.equal(flushed["shadow"][0][1], flushed["s"][:16]) and not torch.equal(flushed["s"][:16], snaps[0]["s"][:16])
    # a second flush changes no bit
    _same(flushed, again)


def test_a_second_run_and_another_grid_give_the_same_bits(runs):
    _, snaps, flushed, _ = runs[N_ARENA]
    for grid in (dict(), dict(dense_blocks=1, nblocks=2)):
        _, snaps2, flushed2, _ = _six_steps(N_ARENA, **grid)
        for x, y in zip(snaps + [flushed], snaps2 + [flushed2]):
            _same(x, y)


@pytest.mark.parametrize("n_dense", [N_ARENA, 1027])
def test_exchange_flushes_swaps_and_restores(n_dense):
    dev = _Device(n_dense)
    _steps(dev)
    before = dev.snapshot()
    assert any(int((s[1:-1] < COUNT0 + T).sum()) for s in before["stamp"])  # (rows still owe: the exchange flushes them itself)
    ref = _Device(n_dense)
    assert dev.launch(3) == 0, L.load().nasrec_last_error()
    swapped = dev.snapshot()
    # the flushed state, from a flush of its own on a copy of the arrays
    for f in range(FS):
        ref.big_t[f].copy_(before["tables"][f])
        ref.big_s[f].copy_(before["shadow"][f])
        ref.big_stamp[f].copy_(before["stamp"][f])
    ref.p.copy_(before["p"])
    ref.s.copy_(before["s"])
    ref.count.fill_(before["count"])
    assert ref.launch(2) == 0
    flushed = ref.snapshot()
    for f in range(FS):
        assert torch.equal(swapped["tables"][f][1:-1], flushed["shadow"][f][1:-1]) and torch.equal(swapped["shadow"][f][1:-1], flushed["tables"][f][1:-1])
        assert torch.equal(swapped["stamp"][f], flushed["stamp"][f])
        for key in ("tables", "shadow"):  # the guard rows stay
            assert torch.equal(swapped[key][f][0], before[key][f][0]) and torch.equal(swapped[key][f][-1], before[key][f][-1])
    assert torch.equal(swapped["p"][:n_dense], flushed["s"][:n_dense]) and torch.equal(swapped["s"][:n_dense], flushed["p"][:n_dense])
    assert torch.equal(swapped["p"][n_dense:], before["p"][n_dense:]) and torch.equal(swapped["s"][n_dense:], before["s"][n_dense:])
    assert swapped["count"] == before["count"] and swapped["counter"] == 0
    assert dev.launch(3) == 0
    _same(flushed, dev.snapshot())


def test_an_empty_batch_averages_the_dense_arena_and_counts():
    dev = _Device(N_ARENA)
    before = dev.snapshot()
    d = L.WeightEmaDesc.from_buffer_copy(dev.d)
    d.B, d.idx, d.leader = 0, None, None
    assert dev.launch(0, d) == 0
    _same(before, dev.snapshot())  # (nothing to catch up: nothing written)
    assert dev.launch(1, d) == 0, L.load().nasrec_last_error()
    after = dev.snapshot()
    assert after["count"] == COUNT0 + 1 and after["counter"] == 0 and not torch.equal(after["s"], before["s"])
    for key in ("tables", "shadow", "stamp"):
        assert all(torch.equal(x, y) for x, y in zip(before[key], after[key])), key


@pytest.mark.parametrize("what", ["no-stamps", "no-shadow", "decay-0", "decay-1", "phase-4"])
def test_refusals_launch_nothing(what):
    dev = _Device(N_ARENA)
    idx = torch.tensor(IDS[0], dtype=torch.int64)
    dev.idx.copy_(idx)
    dev.leader.copy_(_leaders(idx))
    dev.count.fill_(COUNT0 + 3)  # (every phase would have something to write)
    before = dev.snapshot()
    for phase in ((4,) if what == "phase-4" else (0, 1, 2, 3)):
        d = L.WeightEmaDesc.from_buffer_copy(dev.d)
        if what == "no-stamps":
            d.stamp[1] = None
        elif what == "no-shadow":
            d.shadow[2] = None
        elif what == "decay-0":
            d.decay = 0.0
        elif what == "decay-1":
            d.decay = 1.0
        assert dev.launch(phase, d) == -1, (what, phase)
        assert L.load().nasrec_last_error()
        _same(before, dev.snapshot())
