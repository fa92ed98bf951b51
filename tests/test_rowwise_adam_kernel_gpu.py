"""NASREC_OP_OPT_MOMENTS with table_algo = NASREC_TABLE_ALGO_ROWWISE_ADAM (row-sparse Adam with one second moment per table row,
include/nasrec_hip.h) through nasrec_launch against an fp64 NumPy restatement written out here:

    m' = m + (g - m) (1 - b1);   v' = v + (mean(g^2) - v) (1 - b2);   p' = p - lr sqrt(1 - b2^t) / (1 - b1^t) * m' / (sqrt(v') + eps)

on every touched row (g = the leader's summed gradient times the clip coefficient, zero or not), torch.optim.Adam on one dense chunk.
Fs 1 and 26; tables of 1, 5, 300 and 70 000 rows; B 0, 1, 7, 64 and 300, so that B * Fs * 4 threads both fill whole workgroups of 256
(Fs = 1, B = 64) and end inside one; a batch of 7 or more samples holds duplicate ids, the ids -1 and rows[f] (leaders, left unwritten)
and a leader whose summed gradient is exactly zero; the tables' step counts before the step are 0 and 999 (t = 1 and 1000).  The bar
is the kernel bar of test_rowwise_adagrad_kernel_gpu.py (rtol 2e-6, atol 2e-7): one step from fp32 inputs, and the sum of 16 squares
carries at most about 16 * 2^-24 relative error.

tv[f] is handed over inside a guard buffer — rows[f] floats, then NaN — which must come back bit for bit: a kernel that indexed the
second moment as [rows, 16] would read NaN and write into the remainder.  Rows outside the batch keep their bits in table, tm and tv;
the bitmap and the work counter stay zero; the step counters move once; the rank layout (rank_B > 0, NaN between the chunks) gives the
bits of the contiguous layout."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 300, 70000]
BATCHES = [0, 1, 7, 64, 300]
B1, B2, LR, EPS = 0.9, 0.999, 0.01, 1e-8
LR32, EPS32 = float(np.float32(LR)), float(np.float32(EPS))
N_DENSE = 70          # one dense parameter in one chunk, step counter 0; the tables' counters follow
GUARD = 24            # NaN floats behind the rows[f] second moments
GAP = 36              # NaN floats behind every rank chunk of the rank layout


def _rows_of(Fs, size):
    return [size] if Fs == 1 else [SIZES[f % 4] for f in range(Fs)]


def _steps0(Fs, t):
    """step counters before the step: the dense parameter's, then the tables' — t - 1 for Fs = 1, alternating 0 / 999 for Fs = 26"""
    return [4.0] + ([float(t - 1)] if Fs == 1 else [0.0 if (f // 4) % 2 == 0 else 999.0 for f in range(Fs)])


def _case(Fs, size, B, seed=5):
    g = torch.Generator().manual_seed(seed + 97 * Fs + B)
    rows = _rows_of(Fs, size)
    c = {"rows": rows, "tables": [torch.randn(n, 16, generator=g) for n in rows],
         "tm": [torch.randn(n, 16, generator=g) * 0.1 for n in rows], "tv": [],
         "p": torch.randn(N_DENSE, generator=g), "g": torch.randn(N_DENSE, generator=g),
         "m": torch.randn(N_DENSE, generator=g) * 0.1, "v": torch.rand(N_DENSE, generator=g) * 0.01}
    for n in rows:
        buf = torch.full((n + GUARD,), float("nan"))
        buf[:n] = torch.rand(n, generator=g) * 0.01 + 1e-4
        c["tv"].append(buf)
    # ids: the lower half of a table (the upper half rests), so duplicates are common in the small tables
    idx = torch.stack([torch.randint(0, max(1, n // 2), (B,), generator=g) for n in rows], 1) if B else torch.zeros(0, Fs, dtype=torch.int64)
    if B >= 7:
        idx[3] = idx[1]                       # duplicates: only the first occurrence leads
        idx[5] = -1                           # out of range below ...
        idx[6] = torch.tensor(rows)           # ... and at the table end: leaders, left unwritten
    leader = torch.zeros(B, Fs, dtype=torch.int32)
    for f in range(Fs):
        seen = set()
        for b in range(B):
            if int(idx[b, f]) not in seen:
                leader[b, f] = 1
                seen.add(int(idx[b, f]))
    c["idx"], c["leader"], c["gsum"] = idx, leader, torch.randn(B, Fs, 16, generator=g)
    if B >= 7:
        c["gsum"][0] = 0.0                    # sample 0 leads its rows: a touched row whose summed gradient is exactly zero
        assert leader[0].all() and leader[5].all() and leader[6].all() and not leader[3].any()
    return c


def _run(c, steps0, max_norm, rank_B=0, edit=None, phase=0):
    dev = torch.device("cuda", 0)
    rows, Fs = c["rows"], len(c["rows"])
    B = int(c["idx"].shape[0])
    t = {k: ([x.clone().to(dev) for x in v] if isinstance(v, list) and k != "rows" else v.clone().to(dev) if torch.is_tensor(v) else v)
         for k, v in c.items()}
    stride = 0
    if rank_B:
        ranks, stride = B // rank_B, rank_B * Fs * 16 + GAP
        buf = torch.full((ranks * stride,), float("nan"))
        for r in range(ranks):
            buf[r * stride:r * stride + rank_B * Fs * 16] = c["gsum"][r * rank_B:(r + 1) * rank_B].reshape(-1)
        t["gsum"] = buf.to(dev)
    steps = torch.tensor(steps0, dtype=torch.float32, device=dev)
    inc = list(range(1 + Fs))
    tab = torch.tensor([0, N_DENSE, 0] + inc, dtype=torch.int64, device=dev)
    bitmap = torch.zeros(sum(2 * ((n + 63) // 64) for n in rows), dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    partial = torch.tensor([40.0, 60.0], dtype=torch.float32, device=dev)  # norm 10
    clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
    lr_dev = torch.tensor([LR], dtype=torch.float32, device=dev)
    d = L.OptMomentsDesc()
    d.kind, d.phase, d.algo, d.table_algo = L.OP_OPT_MOMENTS, phase, L.OPTIM_ADAM, L.TABLE_ALGO_ROWWISE_ADAM
    d.dense_blocks, d.nblocks = 1, 3
    d.B, d.Fs, d.table_step0 = B, Fs, 1
    d.eps, d.beta1, d.beta2 = EPS, B1, B2
    d.table_eps, d.table_lr_scale = 0.0, 7.0  # (unused by this rule: neither refused nor read)
    d.clip.kind, d.clip.n_a, d.clip.n_b, d.clip.max_norm = L.OP_CLIP_COEF, 2, 0, max_norm
    d.clip.partial_a, d.clip.out = partial.data_ptr(), clip_out.data_ptr()
    d.chunks, d.nchunks = tab.data_ptr(), 1
    d.p, d.g, d.m, d.v = t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr()
    if B:
        d.idx, d.leader, d.gsum = t["idx"].data_ptr(), t["leader"].data_ptr(), t["gsum"].data_ptr()
    d.rank_B, d.rank_stride = rank_B, stride
    for f in range(Fs):  # (no table owns a tile: tile_off stays all zero)
        d.table[f], d.tm[f], d.tv[f], d.rows[f] = t["tables"][f].data_ptr(), t["tm"][f].data_ptr(), t["tv"][f].data_ptr(), rows[f]
    d.bitmap, d.step = bitmap.data_ptr(), steps.data_ptr()
    d.inc, d.n_inc = tab.data_ptr() + 8 * 3, len(inc)
    d.counter, d.lr, d.coef = counter.data_ptr(), lr_dev.data_ptr(), clip_out.data_ptr()
    if edit is not None:
        edit(d)
    lib = L.load()
    rc = lib.nasrec_launch(torch.cuda.current_stream().cuda_stream, C.addressof(d))
    err = lib.nasrec_last_error() if rc else b""
    torch.cuda.synchronize()
    out = {k: ([x.cpu() for x in v] if isinstance(v, list) and k != "rows" else v.cpu() if torch.is_tensor(v) else v) for k, v in t.items()}
    if rank_B:
        buf = out.pop("gsum")
        gaps = torch.cat([buf[r * stride + rank_B * Fs * 16:(r + 1) * stride] for r in range(B // rank_B)])
        assert torch.isnan(gaps).all(), "the gap between the rank chunks was written"
    out.update(steps=steps.cpu(), bitmap=bitmap.cpu(), counter=counter.cpu(), clip=clip_out.cpu(), rc=rc, err=err)
    return out


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.allclose(a, b, rtol=2e-6, atol=2e-7), (what, float(np.abs(a - b).max()) if a.size else 0.0)


def _check(c, out, steps0, max_norm):
    rows, Fs = c["rows"], len(c["rows"])
    B = int(c["idx"].shape[0])
    assert out["rc"] == 0, out["err"]
    coef = float(out["clip"][0])
    assert coef == (float(np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6))) if max_norm else 1.0)
    # the dense chunk: torch.optim.Adam in fp64
    t = steps0[0] + 1
    g = c["g"].double().numpy() * coef
    m = c["m"].double().numpy() + (1 - B1) * (g - c["m"].double().numpy())
    v = B2 * c["v"].double().numpy() + (1 - B2) * g * g
    p = c["p"].double().numpy() - (LR32 / (1 - B1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - B2 ** t) + EPS32)
    _close(out["p"], p, "p")
    _close(out["m"], m, "m")
    _close(out["v"], v, "v")
    assert torch.equal(out["g"], c["g"])
    moved_zero_leader = False
    for f in range(Fs):
        n = rows[f]
        t = steps0[1 + f] + 1
        step_size = LR32 * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
        touched = np.zeros(n, bool)
        for b in range(B):
            r = int(c["idx"][b, f])
            if not (c["leader"][b, f] and 0 <= r < n):
                continue
            touched[r] = True
            g = c["gsum"][b, f].double().numpy() * coef
            m0, v0, p0 = c["tm"][f][r].double().numpy(), float(c["tv"][f][r]), c["tables"][f][r].double().numpy()
            m = m0 + (g - m0) * (1 - B1)
            v = v0 + ((g * g).sum() / 16.0 - v0) * (1 - B2)
            p = p0 - step_size * m / (np.sqrt(v) + EPS32)
            _close(out["tables"][f][r], p, ("table", f, r, t))
            _close(out["tm"][f][r], m, ("tm", f, r, t))
            _close(out["tv"][f][r], v, ("tv", f, r, t))
            if B >= 7 and b == 0:  # the zero-gradient leader decayed m and v and moved
                assert not (g != 0).any()
                assert not torch.equal(out["tables"][f][r], c["tables"][f][r]) and not torch.equal(out["tm"][f][r], c["tm"][f][r])
                assert float(out["tv"][f][r]) < v0
                moved_zero_leader = True
        rest = torch.from_numpy(~touched)
        if B >= 7 or B == 0:
            assert int(rest.sum()) > 0 or n == 1, f
        # rows outside the batch (and behind the ids -1 and rows[f]): bit for bit as they were
        assert _bits(out["tables"][f][rest], c["tables"][f][rest]), ("table", f)
        assert _bits(out["tm"][f][rest], c["tm"][f][rest]), ("tm", f)
        assert _bits(out["tv"][f][:n][rest], c["tv"][f][:n][rest]), ("tv", f)
        assert torch.isnan(out["tv"][f][n:]).all() and _bits(out["tv"][f][n:], c["tv"][f][n:]), ("the guard behind tv was written", f)
        assert bool((out["tv"][f][:n] > 0).all())
    assert moved_zero_leader == (B >= 7)
    assert int(out["bitmap"].abs().sum()) == 0, "a bitmap bit was marked"
    assert int(out["counter"][0]) == 0, "the work counter was left non-zero"
    assert out["steps"].tolist() == [s + 1.0 for s in steps0], "every listed step counter moves exactly once"


CASES = [(1, size, B, t) for size in SIZES for B in BATCHES for t in ((1, 1000) if B in (7, 64) else (1,) if size % 2 else (1000,))] + \
        [(26, 0, B, 0) for B in BATCHES]


@pytest.mark.parametrize("Fs,size,B,t", CASES)
def test_kernel_against_fp64(Fs, size, B, t):
    """every (Fs, table size, B) of the docstring; Fs = 26 carries all four table sizes and both step counts at once"""
    c = _case(Fs, size, B)
    steps0 = _steps0(Fs, t)
    assert {0.0, 999.0} <= set(steps0[1:]) if Fs == 26 else steps0[1] == t - 1
    max_norm = 0.0 if B == 7 else 5.0
    out = _run(c, steps0, max_norm)
    _check(c, out, steps0, max_norm)
    again = _run(c, steps0, max_norm)
    for key in ("p", "m", "v", "steps"):
        assert torch.equal(out[key], again[key]), key
    for f in range(Fs):
        for key in ("tables", "tm", "tv"):
            assert _bits(out[key][f], again[key][f]), (key, f)


def test_thread_counts_cover_whole_and_partial_workgroups():
    counts = {(Fs, B): B * Fs * 4 for Fs in (1, 26) for B in BATCHES}
    assert any(n and n % 256 == 0 for n in counts.values()) and any(n % 256 for n in counts.values())
    assert max(counts.values()) > 256 * 100  # (Fs = 26, B = 300: 122 row workgroups)


@pytest.mark.parametrize("Fs,size,B,rank_B", [(1, 300, 1, 1), (1, 5, 7, 1), (1, 70000, 64, 32), (26, 0, 7, 1), (26, 0, 64, 16), (26, 0, 300, 100)])
def test_rank_layout_gives_the_bits_of_the_contiguous_layout(Fs, size, B, rank_B):
    c = _case(Fs, size, B)
    steps0 = _steps0(Fs, 1000)
    flat, ranked = _run(c, steps0, 5.0), _run(c, steps0, 5.0, rank_B=rank_B)
    assert flat["rc"] == ranked["rc"] == 0, (flat["err"], ranked["err"])
    _check(c, ranked, steps0, 5.0)
    for key in ("p", "m", "v", "g", "steps", "bitmap", "counter", "clip"):
        assert _bits(flat[key], ranked[key]), key
    for f in range(Fs):
        for key in ("tables", "tm", "tv"):
            assert _bits(flat[key][f], ranked[key][f]), (key, f)
    assert any(not torch.equal(a, b) for a, b in zip(flat["tables"], c["tables"]))  # (touched rows moved)


def _set(**kw):
    def edit(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return edit


def _drop(field, f):
    def edit(d):
        getattr(d, field)[f] = None
    return edit


def _own_a_tile(d):
    d.tile_off[1] = 2
    d.n_zero, d.zero_chunks = 1, d.chunks


REFUSALS = {
    "not-adam": (_set(algo=L.OPTIM_SGD), 0, b"table_algo"),
    "rmsprop": (_set(algo=L.OPTIM_RMSPROP), 0, b"table_algo"),
    "sparse-rows": (_set(sparse_rows=1), 0, b"sparse_rows"),
    "reg-mask": (_set(reg_mask=1), 0, b"reg_mask"),
    "no-tm": (_drop("tm", 0), 0, b"tm"),
    "no-tv": (_drop("tv", 0), 0, b"tv"),
    "no-table": (_drop("table", 0), 0, b"table"),
    "no-counter": (_set(counter=None), 0, b"counter"),
    "phase-1-tile": (_own_a_tile, 1, b"table_algo"),
    "phase-1-without-zero-chunks": (_set(), 1, b"table_algo"),
    "phase-2": (_set(), 2, b"phase"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_field_and_launch_nothing(what):
    edit, phase, word = REFUSALS[what]
    c = _case(1, 300, 7)
    steps0 = _steps0(1, 1)
    out = _run(c, steps0, 5.0, edit=edit, phase=phase)
    assert out["rc"] == -1, (out["rc"], out["err"])
    assert word in out["err"] and b"opt_moments" in out["err"], out["err"]
    for key in ("p", "m", "v", "g"):
        assert torch.equal(out[key], c[key]), key
    for key in ("tables", "tm", "tv"):
        assert _bits(out[key][0], c[key][0]), key
    assert out["steps"].tolist() == steps0 and out["clip"].tolist() == [0.0, 0.0] and int(out["counter"][0]) == 0


def test_a_positive_table_eps_is_not_required():
    """the one refusal of the row-wise Adagrad rule this rule drops: table_eps is unused, so 0 and a negative value both run"""
    c = _case(1, 300, 7)
    for teps in (0.0, -1.0):
        out = _run(c, _steps0(1, 1), 5.0, edit=_set(table_eps=teps))
        _check(c, out, _steps0(1, 1), 5.0)
