"""NASREC_OP_OPT_MOMENTS (Adam and momentum SGD of the fused step, include/nasrec_hip.h) through the C-ABI against an fp64 NumPy
restatement of torch's formulas: small tables whose rows do not fill a tile, duplicate ids (leaders only), ids at and past the table
end, dense chunks whose lengths are not multiples of 4, parameters with different step counts, a parameter outside the chunk table,
the clip active and inactive, weight decay on and off.  The touched-row bitmap is all zero behind the step, the counters of exactly
the listed parameters move, and two runs of the same step give the same bits.  B = 8 leaves one row workgroup partly filled; B = 300
fills ten, the last one partly."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu

ROWS = [100, 70]      # 2 tiles of 64 rows each, neither full at the end
B, FS = 8, 2
# dense arena: three parameters at 16-byte aligned offsets; parameter 1 split over two chunks, parameter 2 not reached
PARAMS = [(0, 37), (40, 62), (104, 13)]
CHUNKS = [(0, 37, 0), (40, 32, 1), (72, 30, 1)]
N_DENSE = 120
STEPS0 = [0.0, 3.0, 5.0, 2.0, 0.0]   # dense 0..2, then table 0, table 1
INC = [0, 1, 3, 4]                    # the reached parameters and the tables
ZERO = [(112, 6)]                     # a range whose gradient phase 1 sets back to zero


def _case(seed, B=B):
    g = torch.Generator().manual_seed(seed)
    c = {"tables": [torch.randn(n, 16, generator=g) for n in ROWS], "tm": [torch.randn(n, 16, generator=g) * 0.1 for n in ROWS],
         "tv": [torch.rand(n, 16, generator=g) * 0.01 for n in ROWS], "p": torch.randn(N_DENSE, generator=g),
         "g": torch.randn(N_DENSE, generator=g), "m": torch.randn(N_DENSE, generator=g) * 0.1, "v": torch.rand(N_DENSE, generator=g) * 0.01}
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in ROWS], 1)
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
    return c


def _run(kind, c, max_norm, wd, lr=0.01, nesterov=True):
    dev = torch.device("cuda", 0)
    B = int(c["idx"].shape[0])
    t = {k: ([x.clone().to(dev) for x in v] if isinstance(v, list) else v.clone().to(dev)) for k, v in c.items()}
    steps = torch.tensor(STEPS0, dtype=torch.float32, device=dev)
    tab = torch.tensor([v for ch in CHUNKS for v in ch] + INC + [v for z in ZERO for v in z], dtype=torch.int64, device=dev)
    words = sum(2 * ((n + 63) // 64) for n in ROWS)
    bitmap = torch.zeros(words, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    partial = torch.tensor([40.0, 60.0], dtype=torch.float32, device=dev)  # norm 10
    clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev)
    d = L.OptMomentsDesc()
    d.kind, d.phase = L.OP_OPT_MOMENTS, 0
    d.algo = L.OPTIM_ADAM if kind == "adam" else L.OPTIM_SGD
    d.nesterov = int(nesterov)
    d.dense_blocks, d.nblocks = 2, 3
    d.B, d.Fs, d.table_step0 = B, FS, 3
    d.reg_mask = 0b01 if wd else 0  # table 1 is not regularised
    d.eps, d.momentum, d.wd = 1e-8, 0.9, wd
    d.beta1, d.beta2 = 0.9, 0.999
    d.clip.kind, d.clip.n_a, d.clip.n_b, d.clip.max_norm = L.OP_CLIP_COEF, 2, 0, max_norm
    d.clip.partial_a, d.clip.out = partial.data_ptr(), clip_out.data_ptr()
    d.chunks, d.nchunks = tab.data_ptr(), len(CHUNKS)
    d.p, d.g, d.m = t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr()
    d.v = t["v"].data_ptr() if kind == "adam" else None
    d.idx, d.leader, d.gsum = t["idx"].data_ptr(), t["leader"].data_ptr(), t["gsum"].data_ptr()
    off = 0
    for f in range(FS):
        d.table[f], d.tm[f], d.rows[f] = t["tables"][f].data_ptr(), t["tm"][f].data_ptr(), ROWS[f]
        if kind == "adam":
            d.tv[f] = t["tv"][f].data_ptr()
        d.tile_off[f] = off
        off += (ROWS[f] + 63) // 64
    d.tile_off[FS] = off
    d.bitmap, d.step = bitmap.data_ptr(), steps.data_ptr()
    d.inc, d.n_inc = tab.data_ptr() + 8 * 3 * len(CHUNKS), len(INC)
    d.zero_chunks, d.n_zero = tab.data_ptr() + 8 * (3 * len(CHUNKS) + len(INC)), len(ZERO)
    d.counter, d.lr, d.coef = counter.data_ptr(), lr_dev.data_ptr(), clip_out.data_ptr()
    d1 = L.OptMomentsDesc.from_buffer_copy(d)
    d1.phase = 1
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    for x in (d, d1):
        L.check(lib.nasrec_opt_moments(s, C.addressof(x)))
    torch.cuda.synchronize()
    out = {k: ([x.cpu() for x in v] if isinstance(v, list) else v.cpu()) for k, v in t.items()}
    out["steps"], out["bitmap"], out["counter"], out["clip"] = steps.cpu(), bitmap.cpu(), counter.cpu(), clip_out.cpu()
    return out


def _ref(kind, p, g, m, v, t, lr, nesterov=True):
    """torch.optim.Adam / SGD (foreach, not amsgrad / capturable; dampening 0), fp64"""
    p, g, m, v = (np.asarray(x, np.float64).copy() for x in (p, g, m, v))
    if kind == "adam":
        b1, b2, eps = 0.9, 0.999, 1e-8
        m = m + (1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        p = p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    else:
        m = 0.9 * m + g
        p = p - lr * ((g + 0.9 * m) if nesterov else m)
    return p, m, v


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max() if a.size else 0.0
    assert np.allclose(a, b, rtol=2e-6, atol=2e-7), (what, float(err))


def _check_against_fp64(kind, max_norm, wd, B):
    c = _case(11, B)
    out = _run(kind, c, max_norm, wd)
    lr = float(np.float32(0.01))
    coef = float(out["clip"][0])
    assert abs(float(out["clip"][1]) - 10.0) < 1e-5
    assert coef == (float(np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6))) if max_norm else 1.0)
    # dense: the chunked parameters with their own step counts; the unreached one unchanged
    for k, (o, n) in enumerate(PARAMS):
        sl = slice(o, o + n)
        if k == 2:
            for key in ("p", "m", "v"):
                assert torch.equal(out[key][sl], c[key][sl])
            continue
        p, m, v = _ref(kind, c["p"][sl], c["g"][sl].double() * coef, c["m"][sl], c["v"][sl], STEPS0[k] + 1, lr)
        _close(out["p"][sl], p, ("p", k))
        _close(out["m"][sl], m, ("m", k))
        if kind == "adam":
            _close(out["v"][sl], v, ("v", k))
    assert torch.equal(out["g"][112:118], torch.zeros(6)) and torch.equal(out["g"][:112], c["g"][:112])
    # every table row: the leader rows with their summed gradient, the others with 0 (or 2 wd W on a regularised table)
    for f in range(FS):
        gt = np.zeros((ROWS[f], 16))
        if wd and f == 0:
            gt = (2 * np.float32(wd) * c["tables"][f].numpy().astype(np.float64)) * coef
        for b in range(B):
            r = int(c["idx"][b, f])
            if c["leader"][b, f] and 0 <= r < ROWS[f]:
                gt[r] = c["gsum"][b, f].double().numpy() * coef
        p, m, v = _ref(kind, c["tables"][f], gt, c["tm"][f], c["tv"][f], STEPS0[3 + f] + 1, lr)
        _close(out["tables"][f], p, ("table", f))
        _close(out["tm"][f], m, ("tm", f))
        if kind == "adam":
            _close(out["tv"][f], v, ("tv", f))
    assert int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0
    want = list(STEPS0)
    for k in INC:
        want[k] += 1
    assert out["steps"].tolist() == want
    # same inputs, same bits
    again = _run(kind, c, max_norm, wd)
    for key in ("p", "m", "v", "steps"):
        assert torch.equal(out[key], again[key]), key
    for f in range(FS):
        assert torch.equal(out["tables"][f], again["tables"][f]) and torch.equal(out["tm"][f], again["tm"][f])


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("wd", [0.0, 0.05], ids=["wd0", "wd"])
def test_opt_moments_kernel_against_fp64(kind, max_norm, wd):
    _check_against_fp64(kind, max_norm, wd, B)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("wd", [0.0, 0.05], ids=["wd0", "wd"])
def test_opt_moments_kernel_against_fp64_ten_row_workgroups(kind, max_norm, wd):
    """B = 300: 2400 row threads fill ten row workgroups, the last one partly; the same tables, fp64 reference and bars, ids at and
    past the table end, duplicates, and the bitmap all zero behind phase 1"""
    _check_against_fp64(kind, max_norm, wd, 300)


def test_sgd_without_nesterov_and_first_step_buffer():
    """plain momentum (d = buf); a zero buffer on a parameter's first step gives buf = g exactly (torch: buf = g.clone())"""
    c = _case(5)
    c["m"].zero_()
    out = _run("sgd", c, 0.0, 0.0, nesterov=False)
    o, n = PARAMS[0]
    assert torch.equal(out["m"][o:o + n], c["g"][o:o + n])
    p, _, _ = _ref("sgd", c["p"][o:o + n], c["g"][o:o + n], c["m"][o:o + n], c["v"][o:o + n], 1, float(np.float32(0.01)), nesterov=False)
    _close(out["p"][o:o + n], p, "p")
