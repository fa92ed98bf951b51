"""NASREC_OP_OPT_MOMENTS with sparse_rows = 1 (row-sparse Adam, include/nasrec_hip.h) through the C-ABI against an fp64 NumPy restatement
of torch.optim.SparseAdam on the touched rows and torch.optim.Adam on the dense chunks.  The shapes of test_fused_optimizers_kernel_gpu.py
(tables of 100 and 70 rows, B = 8 with duplicates and ids at and past the table end, dense chunks of 37 / 32 / 30 floats with their
own step counts, a parameter outside the chunk table, clip active and off) and B = 300, whose rows span ten workgroups.  Every row
outside the batch keeps its bits in W and both moments; the bitmap stays all zero; exactly the listed counters move, once — by the
single phase-0 launch without zero_chunks, by phase 0 + phase 1 with them.  The summed rows in the receive buffer of an all-gather
(two rank chunks with a NaN-filled gap between them) give the bits of the contiguous array."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu

ROWS = [100, 70]
FS = 2
PARAMS = [(0, 37), (40, 62), (104, 13)]      # dense arena: parameter 1 split over two chunks, parameter 2 not reached
CHUNKS = [(0, 37, 0), (40, 32, 1), (72, 30, 1)]
N_DENSE = 120
STEPS0 = [0.0, 3.0, 5.0, 2.0, 0.0]           # dense 0..2, then table 0, table 1
INC = [0, 1, 3, 4]
ZERO = [(112, 6)]
B1, B2, LR = 0.9, 0.999, 0.01
# eps: Adam's default, and one of the size of sqrt(v) (0.03 .. 0.1 here), at which SparseAdam's sqrt(v) + eps and dense Adam's
# sqrt(v) / sqrt(1 - b2^t) + eps give updates that differ by percents at the tables' step counts (t = 3 and 1): far above the bar
EPS_VALUES = [1e-8, 1e-3, 5e-2]


def _case(seed, B):
    g = torch.Generator().manual_seed(seed)
    c = {"tables": [torch.randn(n, 16, generator=g) for n in ROWS], "tm": [torch.randn(n, 16, generator=g) * 0.1 for n in ROWS],
         "tv": [torch.rand(n, 16, generator=g) * 0.01 for n in ROWS], "p": torch.randn(N_DENSE, generator=g),
         "g": torch.randn(N_DENSE, generator=g), "m": torch.randn(N_DENSE, generator=g) * 0.1, "v": torch.rand(N_DENSE, generator=g) * 0.01}
    idx = torch.stack([torch.randint(0, n // 2 if B > 8 else n, (B,), generator=g) for n in ROWS], 1)  # (B = 300: half of each table rests)
    idx[3] = idx[1]          # duplicates: only the first occurrence leads
    idx[6, 1] = idx[0, 1]
    idx[5, 0] = ROWS[0]      # at the table end
    idx[7, 1] = ROWS[1] + 9  # past it
    leader = torch.zeros(B, FS, dtype=torch.int32)
    for f in range(FS):
        seen = set()
        for b in range(B):
            if int(idx[b, f]) not in seen:
                leader[b, f] = 1
                seen.add(int(idx[b, f]))
    c["idx"], c["leader"], c["gsum"] = idx, leader, torch.randn(B, FS, 16, generator=g)
    c["gsum"][2] = 0.0       # a touched row whose summed gradient is exactly zero (sample 2 leads its rows)
    assert leader[2].all()
    return c


RANKS, GAP = 2, 36  # the rank layout: two chunks of B / 2 samples, 36 floats of something else behind each


def _run(c, max_norm, zero, algo=None, sparse=1, phases=None, eps=1e-8, ranked=False):
    dev = torch.device("cuda", 0)
    B = int(c["idx"].shape[0])
    t = {k: ([x.clone().to(dev) for x in v] if isinstance(v, list) else v.clone().to(dev)) for k, v in c.items()}
    rb, stride = B // RANKS, B // RANKS * FS * 16 + GAP
    if ranked:  # (as test_dp_layout_kernel_gpu.py builds its buffer)
        buf = torch.full((RANKS * stride,), float("nan"))
        for r in range(RANKS):
            buf[r * stride:r * stride + rb * FS * 16] = c["gsum"][r * rb:(r + 1) * rb].reshape(-1)
        t["gsum"] = buf.to(dev)
    steps = torch.tensor(STEPS0, dtype=torch.float32, device=dev)
    tab = torch.tensor([v for ch in CHUNKS for v in ch] + INC + [v for z in ZERO for v in z], dtype=torch.int64, device=dev)
    bitmap = torch.zeros(sum(2 * ((n + 63) // 64) for n in ROWS), dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    partial = torch.tensor([40.0, 60.0], dtype=torch.float32, device=dev)  # norm 10
    clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
    lr_dev = torch.tensor([LR], dtype=torch.float32, device=dev)
    d = L.OptMomentsDesc()
    d.kind, d.phase, d.sparse_rows = L.OP_OPT_MOMENTS, 0, sparse
    d.algo = L.OPTIM_ADAM if algo is None else algo
    d.nesterov = 1
    d.dense_blocks, d.nblocks = 2, 3
    d.B, d.Fs, d.table_step0 = B, FS, 3
    d.eps, d.momentum, d.wd = eps, 0.9, (0.05 if zero else 0.0)
    d.beta1, d.beta2 = B1, B2
    d.clip.kind, d.clip.n_a, d.clip.n_b, d.clip.max_norm = L.OP_CLIP_COEF, 2, 0, max_norm
    d.clip.partial_a, d.clip.out = partial.data_ptr(), clip_out.data_ptr()
    d.chunks, d.nchunks = tab.data_ptr(), len(CHUNKS)
    d.p, d.g, d.m, d.v = t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr()
    d.idx, d.leader, d.gsum = t["idx"].data_ptr(), t["leader"].data_ptr(), t["gsum"].data_ptr()
    if ranked:
        d.rank_B, d.rank_stride = rb, stride
    for f in range(FS):  # (no table owns a tile: tile_off stays all zero)
        d.table[f], d.tm[f], d.tv[f], d.rows[f] = t["tables"][f].data_ptr(), t["tm"][f].data_ptr(), t["tv"][f].data_ptr(), ROWS[f]
    d.bitmap, d.step = bitmap.data_ptr(), steps.data_ptr()
    d.inc, d.n_inc = tab.data_ptr() + 8 * 3 * len(CHUNKS), len(INC)
    if zero:
        d.zero_chunks, d.n_zero = tab.data_ptr() + 8 * (3 * len(CHUNKS) + len(INC)), len(ZERO)
    d.counter, d.lr, d.coef = counter.data_ptr(), lr_dev.data_ptr(), clip_out.data_ptr()
    d1 = L.OptMomentsDesc.from_buffer_copy(d)
    d1.phase = 1
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    rcs = []
    for x in ((d, d1) if zero else (d,)) if phases is None else [(d, d1)[k] for k in phases]:
        rcs.append(lib.nasrec_opt_moments(s, C.addressof(x)))
    torch.cuda.synchronize()
    out = {k: ([x.cpu() for x in v] if isinstance(v, list) else v.cpu()) for k, v in t.items()}
    if ranked:
        buf = out["gsum"]
        assert torch.isnan(torch.cat([buf[r * stride + rb * FS * 16:(r + 1) * stride] for r in range(RANKS)])).all(), "the gap was written"
        out["gsum"] = torch.cat([buf[r * stride:r * stride + rb * FS * 16].view(rb, FS, 16) for r in range(RANKS)])
    out["steps"], out["bitmap"], out["counter"], out["clip"], out["rc"] = steps.cpu(), bitmap.cpu(), counter.cpu(), clip_out.cpu(), rcs
    return out


def _adam(p, g, m, v, t, eps):
    """torch.optim.Adam (foreach, not amsgrad / capturable), fp64"""
    p, g, m, v = (np.asarray(x, np.float64).copy() for x in (p, g, m, v))
    m = m + (1 - B1) * (g - m)
    v = B2 * v + (1 - B2) * g * g
    p = p - (LR32 / (1 - B1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - B2 ** t) + eps)
    return p, m, v


def _sparse_adam(p, g, m, v, t, eps):
    """torch.optim.SparseAdam on one row, fp64: eps beside sqrt(v), both bias corrections in the step size"""
    p, g, m, v = (np.asarray(x, np.float64).copy() for x in (p, g, m, v))
    m = m + (1 - B1) * (g - m)
    v = v + (1 - B2) * (g * g - v)
    p = p - LR32 * np.sqrt(1 - B2 ** t) / (1 - B1 ** t) * m / (np.sqrt(v) + eps)
    return p, m, v


LR32 = float(np.float32(LR))


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max() if a.size else 0.0
    assert np.allclose(a, b, rtol=2e-6, atol=2e-7), (what, float(err))


@pytest.mark.parametrize("B", [8, 300])
@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("zero", [False, True], ids=["one-launch", "zero-chunks"])
@pytest.mark.parametrize("eps", EPS_VALUES)
def test_sparse_rows_kernel_against_fp64(B, max_norm, zero, eps):
    c = _case(11, B)
    out = _run(c, max_norm, zero, eps=eps)
    eps = float(np.float32(eps))
    assert out["rc"] == [0] * (2 if zero else 1), (out["rc"], L.load().nasrec_last_error())
    coef = float(out["clip"][0])
    assert abs(float(out["clip"][1]) - 10.0) < 1e-5
    assert coef == (float(np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6))) if max_norm else 1.0)
    for k, (o, n) in enumerate(PARAMS):
        sl = slice(o, o + n)
        if k == 2:
            for key in ("p", "m", "v"):
                assert torch.equal(out[key][sl], c[key][sl])
            continue
        p, m, v = _adam(c["p"][sl], c["g"][sl].double() * coef, c["m"][sl], c["v"][sl], STEPS0[k] + 1, eps)
        _close(out["p"][sl], p, ("p", k))
        _close(out["m"][sl], m, ("m", k))
        _close(out["v"][sl], v, ("v", k))
    if zero:
        assert torch.equal(out["g"][112:118], torch.zeros(6)) and torch.equal(out["g"][:112], c["g"][:112])
    else:
        assert torch.equal(out["g"], c["g"])
    for f in range(FS):
        touched = np.zeros(ROWS[f], bool)
        for b in range(B):
            r = int(c["idx"][b, f])
            if c["leader"][b, f] and 0 <= r < ROWS[f]:
                touched[r] = True
                p, m, v = _sparse_adam(c["tables"][f][r], c["gsum"][b, f].double().numpy() * coef, c["tm"][f][r], c["tv"][f][r], STEPS0[3 + f] + 1, eps)
                _close(out["tables"][f][r], p, ("table", f, r))
                _close(out["tm"][f][r], m, ("tm", f, r))
                _close(out["tv"][f][r], v, ("tv", f, r))
        rest = torch.from_numpy(~touched)
        assert 0 < int(rest.sum()) < ROWS[f]
        for key in ("tables", "tm", "tv"):  # every other row: bit for bit as it was
            assert torch.equal(out[key][f][rest], c[key][f][rest]), (key, f)
    # the touched row with a zero gradient decayed its moments and moved
    r = int(c["idx"][2, 0])
    assert not torch.equal(out["tm"][0][r], c["tm"][0][r]) and not torch.equal(out["tables"][0][r], c["tables"][0][r])
    assert int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0
    want = list(STEPS0)
    for k in INC:
        want[k] += 1
    assert out["steps"].tolist() == want
    again = _run(c, max_norm, zero, eps=eps)
    for key in ("p", "m", "v", "g", "steps"):
        assert torch.equal(out[key], again[key]), key
    for f in range(FS):
        for key in ("tables", "tm", "tv"):
            assert torch.equal(out[key][f], again[key][f]), (key, f)


@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("zero", [False, True], ids=["one-launch", "zero-chunks"])
def test_sparse_rows_kernel_reads_the_rank_layout(max_norm, zero):
    """the B = 8 case with gsum in two rank chunks (rank_B = 4) and a NaN-filled gap between them: every output has the bits of the
    contiguous run, and the gap is neither read nor written"""
    c = _case(11, 8)
    flat, ranked = _run(c, max_norm, zero), _run(c, max_norm, zero, ranked=True)
    assert flat["rc"] == ranked["rc"] == [0] * (2 if zero else 1), (flat["rc"], ranked["rc"], L.load().nasrec_last_error())
    assert set(flat) == set(ranked)
    for key in flat:
        if isinstance(flat[key], list) and key != "rc":
            for f in range(FS):
                assert torch.equal(flat[key][f], ranked[key][f]), (key, f)
        elif key != "rc":
            assert torch.equal(flat[key], ranked[key]), key
    assert any(not torch.equal(a, b) for a, b in zip(flat["tables"], c["tables"]))  # (touched rows moved)


def test_phase_0_leaves_the_counting_to_phase_1_when_there_are_zero_chunks():
    c = _case(11, 8)
    out = _run(c, 5.0, True, phases=[0])
    assert out["rc"] == [0] and out["steps"].tolist() == STEPS0 and int(out["counter"][0]) == 0
    assert torch.equal(out["g"], c["g"])


def test_sparse_rows_is_adam_only_and_has_no_table_pass():
    c = _case(11, 8)
    out = _run(c, 5.0, False, algo=L.OPTIM_SGD)
    assert out["rc"] == [-1] and b"sparse_rows" in L.load().nasrec_last_error()
    for key in ("p", "m", "v"):
        assert torch.equal(out[key], c[key])
    assert all(torch.equal(out["tables"][f], c["tables"][f]) for f in range(FS)) and out["steps"].tolist() == STEPS0
    # a phase 1 without zero_chunks has nothing to do: refused, nothing launched
    out = _run(c, 5.0, False, phases=[1])
    assert out["rc"] == [-1] and out["steps"].tolist() == STEPS0
