"""NASREC_OP_OPT_MOMENTS with algo = NASREC_OPTIM_RMSPROP (include/nasrec_hip.h) through the C-ABI, after
test_row_sparse_adam_kernel_gpu.py: six steps with a fixed touch schedule and a flush, against dense torch.optim.RMSprop restated in
fp64 NumPy (every row every step, g = 0 outside the batch) and against the lazy restatement of test_rmsprop_cpu.py for the stamps.

Tables of 1, 65 and 130 rows (64-row tiles: a last tile of 1 and of 2 rows, one exact tile boundary), B = 5 with a duplicate id, a
non-leader pair, the ids -1 and rows[f], a touched row whose summed gradient is zero; dense chunks of 1, 5, 1024 and 1027 floats and a
parameter outside the chunk table; the contiguous gradient rows and a rank layout.  Row 129 of table 2 is touched at steps 1, 2 and 6:
gaps 0 and 3.  The tables start at step counts 2, 0 and 4 with their stamps there."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from test_rmsprop_cpu import lazy_rmsprop_flush, lazy_rmsprop_reference

pytestmark = pytest.mark.gpu

ROWS = [1, 65, 130]
FS, B, T = 3, 5, 6
CHUNKS = [(0, 1, 0), (4, 5, 1), (12, 1024, 2), (1036, 1027, 3)]  # [offset, length, parameter]: float4 pieces and tails
N_DENSE = 2080                                                  # parameter 4 = [2064, 2080): not reached
STEPS0 = [0.0, 3.0, 5.0, 1.0, 7.0, 2.0, 0.0, 4.0]               # dense 0..4, then the three tables
TABLE0 = 5
INC = [0, 1, 2, 3, 5, 6, 7]
ALPHA, EPS, LR = 0.99, 1e-8, 0.01
LR32, EPS32 = float(np.float32(LR)), float(np.float32(EPS))
# ids [B, FS] per step; sample 1 repeats sample 0 in every field (duplicate id, non-leader pair); sample 2's gradient is zero
IDS = [
    [[0, 64, 129], [0, 64, 129], [0, 3, 7], [-1, 65, 130], [0, 63, 128]],
    [[0, 10, 129], [0, 10, 129], [0, 64, 63], [1, -1, 64], [0, 0, 0]],
    [[0, 11, 5], [0, 11, 5], [0, 12, 6], [-1, 65, -1], [0, 13, 7]],
    [[0, 63, 64], [0, 63, 64], [0, 20, 127], [1, 65, 130], [0, 21, 128]],
    [[0, 64, 1], [0, 64, 1], [0, 3, 2], [-1, -1, -1], [0, 30, 3]],
    [[0, 10, 129], [0, 10, 129], [0, 40, 7], [1, 65, 130], [0, 64, 0]],
]
LAYOUTS = {"contiguous": (0, 0), "rank-layout": (1, FS * 16 + 16)}


def _inputs():
    g = torch.Generator().manual_seed(23)
    c = {"tables": [torch.randn(n, 16, generator=g) for n in ROWS], "tv": [torch.rand(n, 16, generator=g) * 0.01 for n in ROWS],
         "p": torch.randn(N_DENSE, generator=g), "v": torch.rand(N_DENSE, generator=g) * 0.01}
    steps = []
    for t in range(T):
        idx = torch.tensor(IDS[t], dtype=torch.int64)
        leader = torch.zeros(B, FS, dtype=torch.int32)
        for f in range(FS):
            seen = set()
            for b in range(B):
                if int(idx[b, f]) not in seen:
                    leader[b, f] = 1
                    seen.add(int(idx[b, f]))
        assert not leader[1].any() and leader[2, 1:].all()
        gsum = torch.randn(B, FS, 16, generator=g)
        gsum[2] = 0.0  # a touched row whose summed gradient is exactly zero
        steps.append(dict(idx=idx, leader=leader, gsum=gsum, g=torch.randn(N_DENSE, generator=g)))
    return c, steps


def _touched(step, coef):
    """{table: {row: clipped summed gradient, fp64}} of one step: leaders with their id in range"""
    out = [dict() for _ in range(FS)]
    for b in range(B):
        for f in range(FS):
            r = int(step["idx"][b, f])
            if step["leader"][b, f] and 0 <= r < ROWS[f]:
                out[f][r] = step["gsum"][b, f].double().numpy() * coef
    return out


class _Device:
    """the arrays of one run on the device and the descriptor over them"""

    def __init__(self, c, layout, max_norm=5.0):
        dev = torch.device("cuda", 0)
        self.rank_B, self.rank_stride = LAYOUTS[layout]
        self.tables = [x.clone().to(dev) for x in c["tables"]]
        self.tv = [x.clone().to(dev) for x in c["tv"]]
        self.stamp = [torch.full((n,), int(STEPS0[TABLE0 + f]), dtype=torch.int32, device=dev) for f, n in enumerate(ROWS)]
        self.p, self.v = c["p"].clone().to(dev), c["v"].clone().to(dev)
        self.g = torch.zeros(N_DENSE, device=dev)
        self.idx = torch.zeros(B, FS, dtype=torch.int64, device=dev)
        self.leader = torch.zeros(B, FS, dtype=torch.int32, device=dev)
        self.gsum = torch.zeros(B * self.rank_stride if self.rank_B else B * FS * 16, device=dev)
        self.steps = torch.tensor(STEPS0, dtype=torch.float32, device=dev)
        self.tab = torch.tensor([v for ch in CHUNKS for v in ch] + INC + [2064, 16], dtype=torch.int64, device=dev)
        self.bitmap = torch.zeros(sum(2 * ((n + 63) // 64) for n in ROWS), dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.partial = torch.tensor([40.0, 60.0], dtype=torch.float32, device=dev)  # norm 10
        self.clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.lr = torch.tensor([LR], dtype=torch.float32, device=dev)
        d = self.d = L.OptMomentsDesc()
        d.kind, d.phase, d.algo = L.OP_OPT_MOMENTS, 0, L.OPTIM_RMSPROP
        d.dense_blocks, d.nblocks = 3, 2
        d.B, d.Fs, d.table_step0 = B, FS, TABLE0
        d.eps, d.beta2 = EPS, ALPHA
        d.clip.kind, d.clip.n_a, d.clip.n_b, d.clip.max_norm = L.OP_CLIP_COEF, 2, 0, max_norm
        d.clip.partial_a, d.clip.out = self.partial.data_ptr(), self.clip_out.data_ptr()
        d.chunks, d.nchunks = self.tab.data_ptr(), len(CHUNKS)
        d.p, d.g, d.v = self.p.data_ptr(), self.g.data_ptr(), self.v.data_ptr()
        d.idx, d.leader, d.gsum = self.idx.data_ptr(), self.leader.data_ptr(), self.gsum.data_ptr()
        d.rank_B, d.rank_stride = self.rank_B, self.rank_stride
        for f in range(FS):  # (the slots of tm carry the stamps; no table owns a tile in phases 0 and 1)
            d.table[f], d.tv[f], d.tm[f], d.rows[f] = self.tables[f].data_ptr(), self.tv[f].data_ptr(), self.stamp[f].data_ptr(), ROWS[f]
        d.bitmap, d.step = self.bitmap.data_ptr(), self.steps.data_ptr()
        d.inc, d.n_inc = self.tab.data_ptr() + 8 * 3 * len(CHUNKS), len(INC)
        d.counter, d.lr, d.coef = self.counter.data_ptr(), self.lr.data_ptr(), self.clip_out.data_ptr()

    def load(self, step):
        self.idx.copy_(step["idx"])
        self.leader.copy_(step["leader"])
        self.g.copy_(step["g"])
        if self.rank_B:
            self.gsum.zero_()
            self.gsum.view(B, self.rank_stride)[:, :FS * 16].copy_(step["gsum"].view(B, FS * 16))
        else:
            self.gsum.copy_(step["gsum"].view(-1))

    def launch(self, d=None):
        rc = L.load().nasrec_opt_moments(torch.cuda.current_stream().cuda_stream, C.addressof(self.d if d is None else d))
        torch.cuda.synchronize()
        return rc

    def flush_desc(self):
        d = L.OptMomentsDesc.from_buffer_copy(self.d)
        d.phase, tile = 2, 0
        for f in range(FS):
            d.tile_off[f] = tile
            tile += (ROWS[f] + 63) // 64
        d.tile_off[FS] = tile
        return d

    def snapshot(self):
        return dict(tables=[x.cpu() for x in self.tables], tv=[x.cpu() for x in self.tv], stamp=[x.cpu() for x in self.stamp], p=self.p.cpu(),
                    v=self.v.cpu(), g=self.g.cpu(), steps=self.steps.cpu(), counter=int(self.counter.cpu()[0]), bitmap=self.bitmap.cpu())


def _same(a, b):
    for k in a:
        if isinstance(a[k], list):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _six_steps(layout):
    """-> [snapshot after each step], the snapshot after the flush, the one after a second flush, the clip coefficient"""
    c, steps = _inputs()
    dev = _Device(c, layout)
    snaps = [dev.snapshot()]
    for step in steps:
        dev.load(step)
        assert dev.launch() == 0, L.load().nasrec_last_error()
        snaps.append(dev.snapshot())
    coef = float(dev.clip_out.cpu()[0])
    fd = dev.flush_desc()
    assert dev.launch(fd) == 0, L.load().nasrec_last_error()
    flushed = dev.snapshot()
    assert dev.launch(fd) == 0
    return c, steps, snaps, flushed, dev.snapshot(), coef


@pytest.fixture(scope="module")
def runs():
    return {k: _six_steps(k) for k in LAYOUTS}


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max() if a.size else 0.0
    assert np.allclose(a, b, rtol=2e-6, atol=2e-7), (what, float(err))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_six_steps_and_a_flush_against_dense_rmsprop_in_fp64(runs, layout):
    c, steps, snaps, flushed, again, coef = runs[layout]
    assert coef == float(np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6)))
    # dense parameters: torch.optim.RMSprop per chunk; the parameter outside the chunk table rests
    p, v = c["p"].double().numpy().copy(), c["v"].double().numpy().copy()
    for step in steps:
        g = step["g"].double().numpy() * coef
        for o, n, _ in CHUNKS:
            sl = slice(o, o + n)
            v[sl] = ALPHA * v[sl] + (1 - ALPHA) * g[sl] * g[sl]
            p[sl] = p[sl] - LR32 * g[sl] / (np.sqrt(v[sl]) + EPS32)
    for o, n, k in CHUNKS:
        _close(flushed["p"][o:o + n], p[o:o + n], ("p", k))
        _close(flushed["v"][o:o + n], v[o:o + n], ("v", k))
    for key in ("p", "v"):
        assert torch.equal(flushed[key][2064:], c[key][2064:]) and torch.equal(flushed[key][1:4], c[key][1:4])
    # tables: dense RMSprop on every row (g = 0 outside the batch) for the flushed state; the lazy restatement for the stamps
    for f in range(FS):
        pd, vd = c["tables"][f].double().numpy().copy(), c["tv"][f].double().numpy().copy()
        pl, vl = pd.copy(), vd.copy()
        count = int(STEPS0[TABLE0 + f])
        stamp = np.full(ROWS[f], count, np.int64)
        for t, step in enumerate(steps):
            touched = _touched(step, coef)[f]
            g = np.zeros_like(pd)
            for r, gr in touched.items():
                g[r] = gr
            vd = ALPHA * vd + (1 - ALPHA) * g * g
            pd = pd - LR32 * g / (np.sqrt(vd) + EPS32)
            count = lazy_rmsprop_reference(pl, vl, stamp, count, touched, ALPHA, EPS32, LR32)
            # before the flush: every row outside the batch keeps its bits in all three arrays; the touched rows are stamped
            rest = torch.ones(ROWS[f], dtype=torch.bool)
            rest[list(touched)] = False
            for key in ("tables", "tv", "stamp"):
                assert torch.equal(snaps[t + 1][key][f][rest], snaps[t][key][f][rest]), (key, f, t)
            assert np.array_equal(snaps[t + 1]["stamp"][f].numpy(), stamp), (f, t)
            _close(snaps[t + 1]["tv"][f], vl, ("tv before the flush", f, t))
        _close(flushed["tables"][f], pd, ("table", f))
        _close(flushed["tv"][f], vd, ("square_avg", f))
        lazy_rmsprop_flush(vl, stamp, count, ALPHA)
        _close(flushed["tv"][f], vl, ("square_avg, lazy restatement", f))
        assert (flushed["stamp"][f] == count).all() and count == STEPS0[TABLE0 + f] + T
        assert torch.equal(flushed["tables"][f], snaps[-1]["tables"][f])  # (the flush moves no weight)
    # the flush had something to pay, the row with gaps 0 and 3 among it; a touched row with a zero gradient decayed and did not move
    assert not torch.equal(flushed["tv"][2], snaps[-1]["tv"][2])
    assert [int(s["stamp"][2][129]) for s in snaps] == [4, 5, 6, 6, 6, 6, 10]
    r = IDS[0][2][1]
    assert torch.equal(snaps[1]["tables"][1][r], c["tables"][1][r]) and not torch.equal(snaps[1]["tv"][1][r], c["tv"][1][r])
    # a second flush changes no bit
    _same(flushed, again)
    # the step counters: every listed parameter once per step, as torch counts; counter and bitmap are left zero
    want = list(STEPS0)
    for k in INC:
        want[k] += T
    assert flushed["steps"].tolist() == want
    assert all(s["counter"] == 0 and int(s["bitmap"].abs().sum()) == 0 for s in snaps + [flushed])


def test_both_layouts_and_a_second_run_give_the_same_bits(runs):
    a, b = runs["contiguous"], runs["rank-layout"]
    for x, y in zip(a[2] + [a[3]], b[2] + [b[3]]):
        _same(x, y)
    rerun = _six_steps("contiguous")
    for x, y in zip(a[2] + [a[3]], rerun[2] + [rerun[3]]):
        _same(x, y)


def test_zero_chunks_leave_the_counting_to_phase_1():
    c, steps = _inputs()
    dev = _Device(c, "contiguous")
    dev.load(steps[0])
    dev.d.wd = 0.05
    dev.d.zero_chunks, dev.d.n_zero = dev.tab.data_ptr() + 8 * (3 * len(CHUNKS) + len(INC)), 1
    assert dev.launch() == 0
    s = dev.snapshot()
    assert s["steps"].tolist() == STEPS0 and s["counter"] == 0 and torch.equal(s["g"], steps[0]["g"])
    d1 = L.OptMomentsDesc.from_buffer_copy(dev.d)
    d1.phase = 1
    assert dev.launch(d1) == 0, L.load().nasrec_last_error()
    s1 = dev.snapshot()
    want = list(STEPS0)
    for k in INC:
        want[k] += 1
    assert s1["steps"].tolist() == want and s1["counter"] == 0
    assert not s1["g"][2064:].any() and torch.equal(s1["g"][:2064], steps[0]["g"][:2064])
    for key in ("tables", "tv", "stamp"):  # phase 1 moves no table row
        assert all(torch.equal(x, y) for x, y in zip(s[key], s1[key])), key


@pytest.mark.parametrize("what", ["no-stamps", "momentum", "sparse_rows", "phase-1-tile"])
def test_refusals_launch_nothing(what):
    c, steps = _inputs()
    dev = _Device(c, "contiguous")
    dev.load(steps[0])
    before = dev.snapshot()
    d = L.OptMomentsDesc.from_buffer_copy(dev.d)
    if what == "no-stamps":
        d.tm[1] = None
    elif what == "momentum":
        d.momentum = 0.9
    elif what == "sparse_rows":
        d.sparse_rows = 1
    else:
        d.phase, d.wd = 1, 0.05
        d.zero_chunks, d.n_zero = dev.tab.data_ptr() + 8 * (3 * len(CHUNKS) + len(INC)), 1
        d.tile_off[FS] = 1
    assert dev.launch(d) == -1
    assert L.load().nasrec_last_error()
    _same(before, dev.snapshot())
