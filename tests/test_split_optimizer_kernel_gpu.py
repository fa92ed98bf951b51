"""NASREC_OP_OPT_MOMENTS with table_algo = NASREC_TABLE_ALGO_ADAGRAD (the split optimizer, include/nasrec_hip.h) through the C-ABI against an
fp64 NumPy restatement: torch.optim.Adam on the dense chunks, torch.optim.Adagrad with the learning rate float32(LR) * float32(scale) and
table_eps on the touched rows.  The shapes of test_row_sparse_adam_kernel_gpu.py (tables of 100 and 70 rows, B = 8 with duplicates and
ids at and past the table end, B = 300 over several row workgroups, dense chunks of 37 / 32 / 30 floats with their own step counts, a
parameter outside the chunk table, clip active and off, with and without zero_chunks) and its bar (rtol 2e-6, atol 2e-7).  Every row
outside the batch keeps its bits in W and tv (Adagrad's sum); tm is NaN-filled and comes back bit for bit (never read, never written);
the touched row whose summed gradient is exactly zero keeps its bits — the opposite of row-sparse Adam; bitmap and counter stay zero;
exactly the listed counters move, once.  Every refusal names its field and leaves every array as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from test_row_sparse_adam_kernel_gpu import B1, B2, CHUNKS, FS, GAP, INC, LR, LR32, PARAMS, RANKS, ROWS, STEPS0, ZERO, _adam, _case, _close

pytestmark = pytest.mark.gpu

SCALES = [1.0, 160.0]
TABLE_EPS = [1e-2, 1e-6]


def _split_case(B):
    """_case of the row-sparse Adam kernel test with tm NaN-filled: the mode has no first moment on the tables"""
    c = _case(11, B)
    c["tm"] = [torch.full_like(t, float("nan")) for t in c["tm"]]
    return c


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run(c, max_norm, zero, scale=1.0, table_eps=1e-2, phases=None, ranked=False, edit=None):
    """one optimizer step through nasrec_opt_moments; edit(d): change the phase-0 descriptor before the launches (the refusals)"""
    dev = torch.device("cuda", 0)
    B = int(c["idx"].shape[0])
    t = {k: ([x.clone().to(dev) for x in v] if isinstance(v, list) else v.clone().to(dev)) for k, v in c.items()}
    rb, stride = B // RANKS, B // RANKS * FS * 16 + GAP
    if ranked:
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
    d.kind, d.phase, d.algo = L.OP_OPT_MOMENTS, 0, L.OPTIM_ADAM
    d.table_algo, d.table_eps, d.table_lr_scale = L.TABLE_ALGO_ADAGRAD, table_eps, scale
    d.dense_blocks, d.nblocks = 2, 3
    d.B, d.Fs, d.table_step0 = B, FS, 3
    d.eps, d.wd = 1e-8, (0.05 if zero else 0.0)
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
    if edit is not None:
        edit(d)
    d1 = L.OptMomentsDesc.from_buffer_copy(d)
    d1.phase = 1
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    rcs = []
    for x in ((d, d1) if zero else (d,)) if phases is None else [(d, d1)[k] for k in phases]:
        rcs.append(lib.nasrec_opt_moments(s, C.addressof(x)))
    err = lib.nasrec_last_error()
    torch.cuda.synchronize()
    out = {k: ([x.cpu() for x in v] if isinstance(v, list) else v.cpu()) for k, v in t.items()}
    if ranked:
        buf = out["gsum"]
        assert torch.isnan(torch.cat([buf[r * stride + rb * FS * 16:(r + 1) * stride] for r in range(RANKS)])).all(), "the gap was written"
        out["gsum"] = torch.cat([buf[r * stride:r * stride + rb * FS * 16].view(rb, FS, 16) for r in range(RANKS)])
    out["steps"], out["bitmap"], out["counter"], out["clip"], out["rc"], out["err"] = \
        steps.cpu(), bitmap.cpu(), counter.cpu(), clip_out.cpu(), rcs, err
    return out


def _adagrad(p, g, s, tlr, eps):
    """torch.optim.Adagrad (lr_decay 0, weight_decay 0) on one row, fp64"""
    p, g, s = (np.asarray(x, np.float64).copy() for x in (p, g, s))
    s = s + g * g
    p = p - tlr * (g / (np.sqrt(s) + eps))
    return p, s


def _untouched(out, c):
    """every array an optimizer step could write has the bits it started with"""
    ok = all(torch.equal(out[k], c[k]) for k in ("p", "m", "v", "g")) and out["steps"].tolist() == STEPS0
    ok = ok and all(torch.equal(out[k][f], c[k][f]) for k in ("tables", "tv") for f in range(FS))
    ok = ok and all(_same_bits(out["tm"][f], c["tm"][f]) for f in range(FS))
    return ok and int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0


@pytest.mark.parametrize("B", [8, 300])
@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("zero", [False, True], ids=["one-launch", "zero-chunks"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("table_eps", TABLE_EPS)
def test_split_kernel_against_fp64(B, max_norm, zero, scale, table_eps):
    c = _split_case(B)
    out = _run(c, max_norm, zero, scale, table_eps)
    assert out["rc"] == [0] * (2 if zero else 1), (out["rc"], out["err"])
    coef = float(out["clip"][0])
    assert abs(float(out["clip"][1]) - 10.0) < 1e-5
    assert coef == (float(np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6))) if max_norm else 1.0)
    eps = float(np.float32(1e-8))
    for k, (o, n) in enumerate(PARAMS):
        sl = slice(o, o + n)
        if k == 2:  # (outside the chunk table)
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
    tlr = float(np.float32(LR) * np.float32(scale))
    teps = float(np.float32(table_eps))
    for f in range(FS):
        touched = np.zeros(ROWS[f], bool)
        for b in range(B):
            r = int(c["idx"][b, f])
            if c["leader"][b, f] and 0 <= r < ROWS[f]:
                touched[r] = True
                p, s = _adagrad(c["tables"][f][r], c["gsum"][b, f].double().numpy() * coef, c["tv"][f][r], tlr, teps)
                _close(out["tables"][f][r], p, ("table", f, r))
                _close(out["tv"][f][r], s, ("sum", f, r))
        rest = torch.from_numpy(~touched)
        assert 0 < int(rest.sum()) < ROWS[f]
        for key in ("tables", "tv"):  # every other row: bit for bit as it was
            assert torch.equal(out[key][f][rest], c[key][f][rest]), (key, f)
        assert _same_bits(out["tm"][f], c["tm"][f]), ("tm was written", f)
        assert torch.isnan(out["tm"][f]).all()
    # the touched row with an exactly zero summed gradient stays where it is, weights and sum (row-sparse Adam moves it)
    for f in range(FS):
        r = int(c["idx"][2, f])
        assert 0 <= r < ROWS[f]
        assert torch.equal(out["tables"][f][r], c["tables"][f][r]) and torch.equal(out["tv"][f][r], c["tv"][f][r]), f
    assert any(not torch.equal(out["tables"][f], c["tables"][f]) for f in range(FS))  # (the others moved)
    assert int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0
    want = list(STEPS0)
    for k in INC:
        want[k] += 1
    assert out["steps"].tolist() == want
    again = _run(c, max_norm, zero, scale, table_eps)
    for key in ("p", "m", "v", "g", "steps"):
        assert torch.equal(out[key], again[key]), key
    for f in range(FS):
        for key in ("tables", "tv"):
            assert torch.equal(out[key][f], again[key][f]), (key, f)


def test_the_table_rate_is_the_scaled_one():
    """scale 160 against scale 1 on the same inputs: the dense chunks have the same bits, the touched rows do not"""
    c = _split_case(8)
    a, b = _run(c, 5.0, False, 1.0), _run(c, 5.0, False, 160.0)
    for key in ("p", "m", "v"):
        assert torch.equal(a[key], b[key]), key
    assert all(torch.equal(a["tv"][f], b["tv"][f]) for f in range(FS))
    assert all(not torch.equal(a["tables"][f], b["tables"][f]) for f in range(FS))


@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("zero", [False, True], ids=["one-launch", "zero-chunks"])
def test_split_kernel_reads_the_rank_layout(max_norm, zero):
    """the B = 8 case with gsum in two rank chunks (rank_B = 4) and a NaN-filled gap between them: every output has the bits of the
    contiguous run, and the gap is neither read nor written"""
    c = _split_case(8)
    flat, ranked = _run(c, max_norm, zero, 160.0), _run(c, max_norm, zero, 160.0, ranked=True)
    assert flat["rc"] == ranked["rc"] == [0] * (2 if zero else 1), (flat["rc"], ranked["rc"], flat["err"], ranked["err"])
    assert set(flat) == set(ranked)
    for key in flat:
        if key in ("rc", "err"):
            continue
        if isinstance(flat[key], list):
            for f in range(FS):
                assert _same_bits(flat[key][f], ranked[key][f]), (key, f)
        else:
            assert _same_bits(flat[key], ranked[key]), key
    assert any(not torch.equal(a, b) for a, b in zip(flat["tables"], c["tables"]))  # (touched rows moved)


def test_phase_0_leaves_the_counting_to_phase_1_when_there_are_zero_chunks():
    c = _split_case(8)
    out = _run(c, 5.0, True, phases=[0])
    assert out["rc"] == [0] and out["steps"].tolist() == STEPS0 and int(out["counter"][0]) == 0
    assert torch.equal(out["g"], c["g"])


def _set(**kw):
    def edit(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return edit


def _own_a_tile(d):
    d.tile_off[1], d.tile_off[2] = 2, 4


REFUSALS = {
    "not-adam": (_set(algo=L.OPTIM_SGD), [0], False, b"table_algo"),
    "rmsprop": (_set(algo=L.OPTIM_RMSPROP), [0], False, b"table_algo"),
    "sparse-rows": (_set(sparse_rows=1), [0], False, b"sparse_rows"),
    "table-eps-zero": (_set(table_eps=0.0), [0], False, b"table_eps"),
    "table-eps-negative": (_set(table_eps=-1e-2), [0], False, b"table_eps"),
    "reg-mask": (_set(reg_mask=1), [0], False, b"reg_mask"),
    "reg-mask-phase-1": (_set(reg_mask=2), [1], True, b"reg_mask"),
    "phase-1-tile": (_own_a_tile, [1], True, b"table_algo"),
    "phase-1-without-zero-chunks": (_set(), [1], False, b"table_algo"),
    "unknown-table-algo": (_set(table_algo=2), [0], False, b"table_algo"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_field_and_launch_nothing(what):
    edit, phases, zero, word = REFUSALS[what]
    c = _split_case(8)
    out = _run(c, 5.0, zero, 160.0, phases=phases, edit=edit)
    assert out["rc"] == [-1], (out["rc"], out["err"])
    assert word in out["err"] and b"opt_moments" in out["err"], out["err"]
    assert _untouched(out, c)
    assert out["clip"].tolist() == [0.0, 0.0]
