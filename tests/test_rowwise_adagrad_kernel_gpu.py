"""NASREC_OP_OPT_MOMENTS with table_algo = NASREC_TABLE_ALGO_ROWWISE_ADAGRAD (row-wise Adagrad on the tables of the split optimizer,
include/nasrec_hip.h) through the C-ABI against an fp64 NumPy restatement: torch.optim.Adam on the dense chunks and, on a touched row,
s' = s + sum(g^2) / 16, p' = p - tlr * g / (sqrt(s') + eps) with tlr = float32(LR) * float32(scale).  The shapes, the cases and the bar
(rtol 2e-6, atol 2e-7) of test_split_optimizer_kernel_gpu.py: tables of 100 and 70 rows (partial wavefronts, active quads between
inactive ones), B = 8 with duplicates and ids at and past the table end, B = 300 over several row workgroups, clip active and off, with
and without zero_chunks, scale 1 and 160, table_eps 1e-2 and 1e-6, the rank layout with its NaN gap.  The sum of 16 non-negative fp32
squares carries at most about 16 * 2^-24 ~ 1e-6 relative error, inside the bar; the W statement is the element-wise one's.

The accumulators are handed over in a guard buffer: tv[f] points at 16 * rows[f] floats of which the first rows[f] are the accumulators
(positive) and the rest NaN, which must come back bit for bit — a kernel that indexed the state as [rows, 16] would read NaN and write
into the remainder, inside the allocation.  Every row outside the batch keeps its bits in W and its accumulator, and so does the touched
row whose summed gradient is exactly zero; tm (NaN) is never touched; bitmap and counter stay zero; exactly the listed step counters
move; a second run gives the same bits; the dense chunks have the bits of the element-wise split on the same inputs.  Every refusal
returns -1, names its field and leaves every array as it was, and table_algo = 2 stays unknown."""
import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from test_row_sparse_adam_kernel_gpu import CHUNKS, FS, INC, LR, PARAMS, ROWS, STEPS0, _adam, _close  # noqa: F401
from test_split_optimizer_kernel_gpu import SCALES, TABLE_EPS, _own_a_tile, _run, _same_bits, _set, _split_case

pytestmark = pytest.mark.gpu


def _rowwise_case(B):
    """the split kernel test's case with tv[f] as the guard buffer: [rows, 16] floats whose first `rows` are the row accumulators"""
    c = _split_case(B)
    g = torch.Generator().manual_seed(23)
    for f, n in enumerate(ROWS):
        buf = torch.full((n, 16), float("nan"))
        buf.view(-1)[:n] = torch.rand(n, generator=g) * 0.01 + 1e-4
        c["tv"][f] = buf
    return c


def _rowwise(edit=None):
    def both(d):
        d.table_algo = L.TABLE_ALGO_ROWWISE_ADAGRAD
        if edit is not None:
            edit(d)
    return both


def _sums(c_or_out, f):
    return c_or_out["tv"][f].view(-1)[:ROWS[f]]


def _guard_intact(out, c):
    return all(_same_bits(out["tv"][f].view(-1)[ROWS[f]:], c["tv"][f].view(-1)[ROWS[f]:])
               and bool(torch.isnan(out["tv"][f].view(-1)[ROWS[f]:]).all()) for f in range(FS))


def _untouched(out, c):
    """every array an optimizer step could write has the bits it started with"""
    ok = all(torch.equal(out[k], c[k]) for k in ("p", "m", "v", "g")) and out["steps"].tolist() == STEPS0
    ok = ok and all(torch.equal(out["tables"][f], c["tables"][f]) for f in range(FS))
    ok = ok and all(_same_bits(out[k][f], c[k][f]) for k in ("tm", "tv") for f in range(FS))
    return ok and int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0


def test_the_constant():
    assert L.TABLE_ALGO_ROWWISE_ADAGRAD == 3 and L.load().nasrec_abi_version() == 17


@pytest.mark.parametrize("B", [8, 300])
@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("zero", [False, True], ids=["one-launch", "zero-chunks"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("table_eps", TABLE_EPS)
def test_rowwise_kernel_against_fp64(B, max_norm, zero, scale, table_eps):
    c = _rowwise_case(B)
    out = _run(c, max_norm, zero, scale, table_eps, edit=_rowwise())
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
    # the dense chunks: the bits of the element-wise split on the same inputs
    elementwise = _run(_split_case(B), max_norm, zero, scale, table_eps)
    for key in ("p", "m", "v", "g", "steps"):
        assert torch.equal(out[key], elementwise[key]), key
    tlr = float(np.float32(LR) * np.float32(scale))
    teps = float(np.float32(table_eps))
    assert _guard_intact(out, c), "the remainder of the guard buffer was written: the state is indexed as [rows, 16]"
    for f in range(FS):
        touched = np.zeros(ROWS[f], bool)
        s0, s1 = _sums(c, f).double().numpy(), _sums(out, f)
        for b in range(B):
            r = int(c["idx"][b, f])
            if c["leader"][b, f] and 0 <= r < ROWS[f]:
                touched[r] = True
                g = c["gsum"][b, f].double().numpy() * coef
                s = s0[r] + (g * g).sum() / 16.0
                p = c["tables"][f][r].double().numpy() - tlr * (g / (np.sqrt(s) + teps))
                _close(out["tables"][f][r], p, ("table", f, r))
                _close(s1[r], s, ("sum", f, r))
        rest = torch.from_numpy(~touched)
        assert 0 < int(rest.sum()) < ROWS[f]
        # every other row: bit for bit as it was
        assert torch.equal(out["tables"][f][rest], c["tables"][f][rest]), ("tables", f)
        assert _same_bits(s1[rest], _sums(c, f)[rest]), ("sum", f)
        assert _same_bits(out["tm"][f], c["tm"][f]), ("tm was written", f)
        assert torch.isnan(out["tm"][f]).all()
        assert bool((s1 > 0).all())
    # the touched row with an exactly zero summed gradient stays where it is, weights and accumulator
    for f in range(FS):
        r = int(c["idx"][2, f])
        assert 0 <= r < ROWS[f]
        assert torch.equal(out["tables"][f][r], c["tables"][f][r]) and _same_bits(_sums(out, f)[r:r + 1], _sums(c, f)[r:r + 1]), f
    assert any(not torch.equal(out["tables"][f], c["tables"][f]) for f in range(FS))  # (the others moved)
    assert any(not torch.equal(_sums(out, f), _sums(c, f)) for f in range(FS))
    assert int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0
    want = list(STEPS0)
    for k in INC:
        want[k] += 1
    assert out["steps"].tolist() == want
    again = _run(c, max_norm, zero, scale, table_eps, edit=_rowwise())
    for key in ("p", "m", "v", "g", "steps"):
        assert torch.equal(out[key], again[key]), key
    for f in range(FS):
        assert torch.equal(out["tables"][f], again["tables"][f]), f
        assert _same_bits(out["tv"][f], again["tv"][f]), f


def test_one_accumulator_divides_the_whole_row():
    """the 16 elements of a touched row move by g[e] times ONE factor: (p - p') / g is the same number across the row to fp32 rounding,
    which the element-wise rule (16 accumulators) does not give"""
    c = _rowwise_case(8)
    out = _run(c, 0.0, False, 160.0, 1e-2, edit=_rowwise())
    assert out["rc"] == [0], out["err"]
    b, f = 0, 0
    r = int(c["idx"][b, f])
    assert c["leader"][b, f] and 0 <= r < ROWS[f]
    big = c["gsum"][b, f].abs() > 0.1  # (the quotient of a small g magnifies the rounding of p - p')
    assert int(big.sum()) >= 8
    ratio = ((c["tables"][f][r].double() - out["tables"][f][r].double()) / c["gsum"][b, f].double())[big]
    assert float((ratio.max() - ratio.min()) / ratio.mean().abs()) < 1e-4
    want = float(np.float32(LR) * np.float32(160.0)) / (float(_sums(out, f)[r].double().sqrt()) + float(np.float32(1e-2)))
    assert abs(float(ratio.mean()) - want) < 1e-4 * want


@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("zero", [False, True], ids=["one-launch", "zero-chunks"])
def test_rowwise_kernel_reads_the_rank_layout(max_norm, zero):
    """the B = 8 case with gsum in two rank chunks (rank_B = 4) and a NaN-filled gap between them: every output has the bits of the
    contiguous run, and the gap is neither read nor written"""
    c = _rowwise_case(8)
    flat = _run(c, max_norm, zero, 160.0, edit=_rowwise())
    ranked = _run(c, max_norm, zero, 160.0, ranked=True, edit=_rowwise())
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
    assert _guard_intact(ranked, c)


def test_phase_0_leaves_the_counting_to_phase_1_when_there_are_zero_chunks():
    c = _rowwise_case(8)
    out = _run(c, 5.0, True, phases=[0], edit=_rowwise())
    assert out["rc"] == [0] and out["steps"].tolist() == STEPS0 and int(out["counter"][0]) == 0
    assert torch.equal(out["g"], c["g"])


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
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_field_and_launch_nothing(what):
    edit, phases, zero, word = REFUSALS[what]
    c = _rowwise_case(8)
    out = _run(c, 5.0, zero, 160.0, phases=phases, edit=_rowwise(edit))
    assert out["rc"] == [-1], (out["rc"], out["err"])
    assert word in out["err"] and b"opt_moments" in out["err"], out["err"]
    assert _untouched(out, c)
    assert out["clip"].tolist() == [0.0, 0.0]


def test_table_algo_2_is_still_unknown():
    c = _rowwise_case(8)
    out = _run(c, 5.0, False, 160.0, phases=[0], edit=_set(table_algo=2))
    assert out["rc"] == [-1] and b"table_algo 2" in out["err"], (out["rc"], out["err"])
    assert _untouched(out, c)
