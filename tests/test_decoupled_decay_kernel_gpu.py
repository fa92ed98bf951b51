"""NASREC_OP_DECOUPLED_DECAY (include/nasrec_hip.h, csrc/decoupled_decay.hip) through the C-ABI, after test_weight_ema_kernel_gpu.py:
six steps of catch-up (phase 0), decay (phase 1) and a torch addition to the batch's rows and the selected dense ranges standing in for
the optimizer; then the flush (phase 2) — against a dense fp64 mirror that decays EVERY row of the decaying tables every step, under
the derived bar of test_decoupled_decay_cpu.py.

Three tables of {5, 64, 200} and of {1, 63, 65} rows (the edges of the 64-row tiles of the table pass); the mask covers tables 1 and 2.
Batches of 1, 3 and 64 samples drawn from the lower three quarters of each table (the rest is in no batch), with the ids -1 and rows[f]
among them; a guard row on either side of every table and stamp array.  A dense arena of 1040 floats of which n in {0, 3, 1027} are in
play, through a chunk table that selects some ranges (one starts off a 16-byte boundary, one is a 3-float tail).  lambda = 0.1, lr from a
cosine between 1e-2 and 1e-3 rounded to fp32.

Measured on an MI355X: the largest error is 0.17 to 0.39 of the bar (3 T + 2) 2^-24 M over the six cases, i.e. also inside the
(2 T + 2) 2^-24 M that counts no rounding for the factor."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from test_decoupled_decay_cpu import cosine_lrs, decay_bar

pytestmark = pytest.mark.gpu

FS, T, LAM = 3, 6, 0.1
MASK = 0b110
N_ARENA = 1040
ROW_SETS = [(5, 64, 200), (1, 63, 65)]
N_OF_B = {1: 0, 3: 1027, 64: 3}
CHUNKS = {0: [], 3: [(0, 3)], 1027: [(0, 512), (516, 8), (601, 30), (1024, 3)]}
LRS = cosine_lrs(T)


def _ids(rows, B, t, g):
    """[B, FS] ids of step t: from the lower three quarters of each table; -1 and rows[f] once each"""
    idx = torch.stack([torch.randint(0, max(1, (3 * r) // 4), (B,), generator=g) for r in rows], dim=1)
    if B >= 3:
        idx[0, t % FS] = -1
        idx[1, (t + 1) % FS] = rows[(t + 1) % FS]
        idx[2] = idx[B - 1]  # (a duplicate id in every field: one leader, one follower)
    elif t == 2:
        idx[0, 1] = -1
    elif t == 3:
        idx[0, 2] = rows[2]
    return idx


def _leaders(idx):
    B = idx.shape[0]
    leader = torch.zeros(B, FS, dtype=torch.int32)
    for f in range(FS):
        seen = set()
        for b in range(B):
            if int(idx[b, f]) not in seen:
                leader[b, f] = 1
                seen.add(int(idx[b, f]))
    return leader


def _touched(idx, rows, f):
    return sorted({int(r) for r in idx[:, f] if 0 <= int(r) < rows[f]})


def _selected(n):
    sel = torch.zeros(N_ARENA, dtype=torch.bool)
    for o, c in CHUNKS[n]:
        sel[o:o + c] = True
    return sel


class _Device:
    """the arrays of one run on the device (tables and stamps with a guard row before and behind) and the descriptor"""

    def __init__(self, rows, B, n, dense_blocks=3, nblocks=1):
        dev = self.dev = torch.device("cuda", 0)
        g = torch.Generator().manual_seed(41)
        self.rows, self.B, self.n = rows, B, n
        self.big_t = [torch.randn(r + 2, 16, generator=g).to(dev) for r in rows]
        self.big_stamp = [torch.zeros(r + 2, dtype=torch.float32, device=dev) for r in rows]
        self.tables = [x[1:-1] for x in self.big_t]
        self.stamp = [x[1:-1] for x in self.big_stamp]
        self.p = torch.randn(N_ARENA, generator=g).to(dev)
        self.idx = torch.zeros(max(B, 1), FS, dtype=torch.int64, device=dev)
        self.leader = torch.zeros(max(B, 1), FS, dtype=torch.int32, device=dev)
        flat = [v for oc in CHUNKS[n] for v in oc]
        self.chunks = torch.tensor(flat if flat else [0], dtype=torch.int64, device=dev)
        self.level = torch.zeros(FS, dtype=torch.float64, device=dev)
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        d = self.d = L.DecoupledDecayDesc()
        d.kind, d.phase, d.B, d.Fs, d.mask, d.lambda_, d.lr_max = L.OP_DECOUPLED_DECAY, 0, B, FS, MASK, LAM, 1e-2
        d.dense_blocks, d.nblocks = dense_blocks, nblocks
        d.idx, d.leader = self.idx.data_ptr(), self.leader.data_ptr()
        tile = 0
        for f in range(FS):
            d.table[f], d.stamp[f], d.rows[f], d.tile_off[f] = self.tables[f].data_ptr(), self.stamp[f].data_ptr(), rows[f], tile
            if (MASK >> f) & 1:
                tile += (rows[f] + 63) // 64
        d.tile_off[FS] = tile
        self.bitmap = torch.zeros(2 * tile, dtype=torch.int32, device=dev)
        d.bitmap, d.p = self.bitmap.data_ptr(), self.p.data_ptr()
        d.n_chunks = len(CHUNKS[n])
        d.chunks = self.chunks.data_ptr() if CHUNKS[n] else None
        d.level, d.lr, d.counter = self.level.data_ptr(), self.lr.data_ptr(), self.counter.data_ptr()

    def launch(self, phase, d=None):
        d = L.DecoupledDecayDesc.from_buffer_copy(self.d if d is None else d)
        if phase is not None:
            d.phase = phase
        rc = L.load().nasrec_decoupled_decay(torch.cuda.current_stream().cuda_stream, C.addressof(d))
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return dict(tables=[x.cpu() for x in self.big_t], stamp=[x.cpu() for x in self.big_stamp], p=self.p.cpu(),
                    level=self.level.cpu(), counter=int(self.counter.cpu()[0]), bitmap=self.bitmap.cpu())


def _same(a, b):
    for k in a:
        if isinstance(a[k], list):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _six_steps(rows, B, **grid):
    """-> dict: the snapshots (start, after every step, after the flush, after a second flush), the fp64 mirror and M of the tables
    and the dense arena, the rows in no batch, and the largest error of the batch's rows behind phase 0 as a fraction of the bar"""
    n = N_OF_B[B]
    dev = _Device(rows, B, n, **grid)
    g = torch.Generator().manual_seed(42)
    snaps = [dev.snapshot()]
    mirror = [t.cpu().double().numpy().copy() for t in dev.tables]
    M = [np.abs(m) for m in mirror]
    pm = dev.p.cpu().double().numpy().copy()
    pM = np.abs(pm)
    sel = _selected(n)
    level, seen, worst0 = 0.0, [set() for _ in range(FS)], 0.0
    for t in range(T):
        lr = LRS[t]
        idx = _ids(rows, B, t, g)
        dev.idx.copy_(idx)
        dev.leader.copy_(_leaders(idx))
        dev.lr.fill_(lr)
        assert dev.launch(0) == 0, L.load().nasrec_last_error()
        # behind phase 0 the batch's rows are current: the mirror's, which decayed every row in every step so far
        for f in (1, 2):
            for r in _touched(idx, rows, f):
                err = np.abs(dev.tables[f][r].cpu().double().numpy() - mirror[f][r])
                bar = decay_bar(t, M[f][r])
                assert (err <= bar).all(), ("phase 0", t, f, r)
                if t:
                    worst0 = max(worst0, float((err / bar).max()))
                seen[f].add(r)
        assert dev.launch(1) == 0, L.load().nasrec_last_error()
        level += math.log1p(-lr * LAM)
        for f in (1, 2):
            mirror[f] *= 1.0 - lr * LAM
            for r in _touched(idx, rows, f):  # the optimizer's stand-in: one fp32 addition to the leader rows
                u = 0.05 * torch.randn(16, generator=g)
                dev.tables[f][r] += u.to(dev.dev)
                mirror[f][r] += u.double().numpy()
            M[f] = np.maximum(M[f], np.abs(mirror[f]))
        u = (0.05 * torch.randn(N_ARENA, generator=g)) * sel
        pm[sel.numpy()] *= 1.0 - lr * LAM
        dev.p += u.to(dev.dev)
        pm += u.double().numpy()
        pM = np.maximum(pM, np.abs(pm))
        snaps.append(dev.snapshot())
        got = snaps[-1]["level"].numpy()
        assert got[0] == 0.0 and abs(got[1] - level) <= 1e-15 and got[1] == got[2] and snaps[-1]["counter"] == 0, (t, got, level)
    assert dev.launch(2) == 0, L.load().nasrec_last_error()
    flushed = dev.snapshot()
    assert dev.launch(2) == 0
    never = [[r for r in range(rows[f]) if r not in seen[f]] for f in range(FS)]
    return dict(snaps=snaps, flushed=flushed, again=dev.snapshot(), mirror=mirror, M=M, pm=pm, pM=pM, sel=sel, never=never, worst0=worst0)


CASES = [(rows, B) for rows in ROW_SETS for B in (1, 3, 64)]


@pytest.fixture(scope="module")
def runs():
    return {case: _six_steps(*case) for case in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "rows%s-B%d" % ("x".join(map(str, c[0])), c[1]))
def test_six_steps_and_a_flush_against_the_dense_decay_in_fp64(runs, case):
    rows, B = case
    r = runs[case]
    snaps, flushed = r["snaps"], r["flushed"]
    worst = r["worst0"]
    for f in (1, 2):
        # before the flush a row outside every batch has its initial bits and a zero stamp
        assert r["never"][f], (f, rows)
        for row in r["never"][f]:
            assert torch.equal(snaps[-1]["tables"][f][row + 1], snaps[0]["tables"][f][row + 1]) and float(snaps[-1]["stamp"][f][row + 1]) == 0.0
        # after it every row is the dense fp64 decay of the recorded history
        err = np.abs(flushed["tables"][f][1:-1].double().numpy() - r["mirror"][f])
        bar = decay_bar(T, r["M"][f])
        assert (err <= bar).all(), ("table", f, float((err / bar).max()))
        worst = max(worst, float((err / bar).max()))
        if r["never"][f]:  # (the flush had something to pay)
            assert not torch.equal(flushed["tables"][f], snaps[-1]["tables"][f])
        # ids -1 and rows[f] wrote nothing: the guard rows keep their bits through every launch
        for key in ("tables", "stamp"):
            for s in snaps + [flushed]:
                assert torch.equal(s[key][f][0], snaps[0][key][f][0]) and torch.equal(s[key][f][-1], snaps[0][key][f][-1]), (key, f)
    # the table outside the mask: weights and stamps untouched
    for s in snaps + [flushed]:
        assert torch.equal(s["tables"][0], snaps[0]["tables"][0]) and torch.equal(s["stamp"][0], snaps[0]["stamp"][0])
    # the dense arena: the selected ranges within the bar, everything else with its bits
    sel = r["sel"]
    if sel.any():
        err = np.abs(flushed["p"].double().numpy() - r["pm"])[sel.numpy()]
        bar = decay_bar(T, r["pM"][sel.numpy()])
        assert (err <= bar).all(), ("dense", float((err / bar).max()))
        worst = max(worst, float((err / bar).max()))
        assert not torch.equal(flushed["p"][sel], snaps[0]["p"][sel])
    assert torch.equal(flushed["p"][~sel], snaps[0]["p"][~sel])
    print("largest error as a fraction of the bar: %.3f" % worst)
    # stamps and levels are back at 0, the counter and the bitmap are left zero, and a second flush changes no bit
    assert all(int((s != 0).sum()) == 0 for s in flushed["stamp"]) and int((flushed["level"] != 0).sum()) == 0
    assert flushed["counter"] == 0 and int(flushed["bitmap"].abs().sum()) == 0
    _same(flushed, r["again"])


def test_a_second_run_and_another_grid_give_the_same_bits(runs):
    case = CASES[1]
    r = runs[case]
    for grid in (dict(), dict(dense_blocks=1, nblocks=2)):
        r2 = _six_steps(*case, **grid)
        for x, y in zip(r["snaps"] + [r["flushed"]], r2["snaps"] + [r2["flushed"]]):
            _same(x, y)


def test_a_row_the_whole_batch_carries_pays_once():
    """the claim: 64 samples with the same id in every field — behind phase 0 the row has paid what it owes exactly once"""
    rows, B = ROW_SETS[0], 64
    dev = _Device(rows, B, 0)
    g = torch.Generator().manual_seed(43)
    level = 0.0
    for t in range(3):  # three steps on other rows move the levels
        idx = torch.stack([torch.randint(0, r // 2, (B,), generator=g) for r in rows], dim=1)
        dev.idx.copy_(idx)
        dev.leader.copy_(_leaders(idx))
        dev.lr.fill_(LRS[t])
        assert dev.launch(0) == 0 and dev.launch(1) == 0, L.load().nasrec_last_error()
        level += math.log1p(-LRS[t] * LAM)
    target = [r - 1 for r in rows]  # (upper half: untouched so far)
    before = dev.snapshot()
    dev.idx.copy_(torch.tensor([target] * B, dtype=torch.int64))
    assert dev.launch(0) == 0, L.load().nasrec_last_error()
    after = dev.snapshot()
    for f in (1, 2):
        w0 = before["tables"][f][target[f] + 1].double().numpy()
        got = after["tables"][f][target[f] + 1].double().numpy()
        assert (np.abs(got - w0 * math.exp(level)) <= decay_bar(1, np.abs(w0))).all(), f
        assert (np.abs(got - w0 * math.exp(2 * level)) > 10 * decay_bar(1, np.abs(w0))).any(), f  # (paying twice is far outside)
        assert float(after["stamp"][f][target[f] + 1]) == float(np.float32(level))
        keep = torch.ones(rows[f] + 2, dtype=torch.bool)
        keep[target[f] + 1] = False
        assert torch.equal(after["tables"][f][keep], before["tables"][f][keep]) and torch.equal(after["stamp"][f][keep], before["stamp"][f][keep])
    assert torch.equal(after["tables"][0], before["tables"][0]) and torch.equal(after["level"], before["level"])
    assert dev.launch(0) == 0  # (current now: a second catch-up writes nothing)
    _same(after, dev.snapshot())


def test_a_step_without_rows_decays_the_dense_ranges_and_moves_no_level():
    dev = _Device(ROW_SETS[0], 3, 1027)
    dev.lr.fill_(LRS[0])
    before = dev.snapshot()
    d = L.DecoupledDecayDesc.from_buffer_copy(dev.d)
    d.B, d.idx, d.leader = 0, None, None
    assert dev.launch(0, d) == 0
    _same(before, dev.snapshot())  # (nothing to catch up: nothing written)
    assert dev.launch(1, d) == 0, L.load().nasrec_last_error()
    after = dev.snapshot()
    sel = _selected(1027)
    want = before["p"][sel] * float(np.float32(1.0 - LRS[0] * LAM))
    assert torch.equal(after["p"][sel], want) and torch.equal(after["p"][~sel], before["p"][~sel])
    for key in ("tables", "stamp"):
        assert all(torch.equal(x, y) for x, y in zip(before[key], after[key])), key
    assert torch.equal(after["level"], before["level"]) and after["counter"] == 0


@pytest.mark.parametrize("what", ["no-table", "no-stamps", "no-levels", "lambda-negative", "lr-lambda-1", "phase-3", "too-many-tables"])
def test_refusals_launch_nothing(what):
    rows = ROW_SETS[0]
    dev = _Device(rows, 3, 1027)
    idx = _ids(rows, 3, 0, torch.Generator().manual_seed(44))
    dev.idx.copy_(idx)
    dev.leader.copy_(_leaders(idx))
    dev.lr.fill_(LRS[0])
    dev.level.fill_(-0.01)  # (every phase would have something to write)
    before = dev.snapshot()
    for phase in ((3, -1) if what == "phase-3" else (0, 1, 2)):
        d = L.DecoupledDecayDesc.from_buffer_copy(dev.d)
        if what == "no-table":
            d.table[2] = None
        elif what == "no-stamps":
            d.stamp[1] = None
        elif what == "no-levels":
            d.level = None
        elif what == "lambda-negative":
            d.lambda_ = -0.1
        elif what == "lr-lambda-1":
            d.lambda_, d.lr_max = 100.0, 1e-2
        elif what == "too-many-tables":
            d.Fs = L.MAX_TABLES + 1
        assert dev.launch(phase, d) == -1, (what, phase)
        assert L.load().nasrec_last_error()
        _same(before, dev.snapshot())
