"""bf16 embedding tables through the C-ABI (include/nasrec_hip.h): the gather's bf16 form (nasrec_embed_desc_t.table_dtype = 1), alone and
riding on the staging launch, and NASREC_OP_OPT_MOMENTS with table_algo = NASREC_TABLE_ALGO_ROWWISE_ADAGRAD_BF16.

Nothing here has a tolerance.  The gather widens exactly (bits << 16).  The update is the fp32 row-wise kernel's arithmetic on the widened
row followed by a pure integer rule, so the bf16 kernel's tables must equal utils/optim.stochastic_round_bf16 of what the fp32 row-wise
kernel leaves on the widened tables, bit for bit, and its accumulators, dense chunks, step counters and gradients must be that run's bits.
The cases are test_rowwise_adagrad_kernel_gpu.py's: tables of 100 and 70 rows, B = 8 with duplicates, an exactly-zero summed gradient and
ids at and past the table end, B = 300 over several row workgroups, clip on and off, with and without zero_chunks, scale 1 and 160,
table_eps 1e-2 and 1e-6, the rank layout.

Every bf16 table is handed over in a buffer the size of the fp32 table whose second half holds a sentinel pattern, and the accumulators
in that test's NaN guard buffer: both halves come back bit for bit, which a kernel that indexed rows at 64 bytes would not do."""
import ctypes as C

import pytest
import torch

import test_split_optimizer_kernel_gpu as SK
from nasrec_amd import _lib as L
from nasrec_amd.utils.optim import stochastic_round_bf16
from test_row_sparse_adam_kernel_gpu import FS, INC, ROWS, STEPS0
from test_rowwise_adagrad_kernel_gpu import _guard_intact, _rowwise, _rowwise_case, _sums
from test_split_optimizer_kernel_gpu import SCALES, TABLE_EPS, _own_a_tile, _run, _same_bits, _set

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789
SENTINEL = 0x7A5C  # (as bf16 a large finite number; as the upper half of an fp32 row it would be read and rewritten)


def _i16(x):
    return x.contiguous().view(torch.int16)


def _bf16_case(B):
    """(the row-wise kernel test's case on the WIDENED tables, the same case with every table as bf16 in a guard buffer [rows, 32]:
    flat, its first rows * 16 elements are the table, the rest SENTINEL)"""
    ref = _rowwise_case(B)
    narrow = [t.to(torch.bfloat16) for t in ref["tables"]]
    narrow[0][1, :6] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 3.0e38, -3.0e38]).to(torch.bfloat16)  # zeros, denormals, the largest binade
    ref["tables"] = [t.float() for t in narrow]
    c = dict(ref)
    c["tables"] = []
    for n, t in zip(ROWS, narrow):
        buf = torch.full((n, 32), SENTINEL, dtype=torch.int16).view(torch.bfloat16)
        buf.view(-1)[:n * 16] = t.reshape(-1)
        c["tables"].append(buf)
    return ref, c


def _bf16(edit=None, seed=SEED):
    def both(d):
        d.table_algo = L.TABLE_ALGO_ROWWISE_ADAGRAD_BF16
        for f in range(L.MAX_TABLES):
            d.tm[f] = None
        d.sr_seed = seed
        if edit is not None:
            edit(d)
    return both


def _table(out_or_c, f):
    return out_or_c["tables"][f].view(-1)[:ROWS[f] * 16].view(ROWS[f], 16)


def _sentinel_intact(out, f):
    return bool((_i16(out["tables"][f].view(-1)[ROWS[f] * 16:]) == SENTINEL).all())


def _check_against_fp32(ref, c, out32, out, steps0=STEPS0, seed=SEED):
    for key in ("p", "m", "v", "g", "steps", "bitmap", "counter", "clip"):
        assert _same_bits(out[key].float(), out32[key].float()), key
    moved = 0
    for f in range(FS):
        assert _same_bits(out["tv"][f], out32["tv"][f]), ("sum", f)
        assert _sentinel_intact(out, f), "the second half of the table buffer was written: rows are indexed at 64 bytes"
        t = int(steps0[3 + f]) + 1
        want = stochastic_round_bf16(out32["tables"][f], seed, t, f, torch.arange(ROWS[f]))
        assert torch.equal(_i16(_table(out, f)), _i16(want)), ("table", f)
        same = (_i16(_table(out, f)) == _i16(_table(c, f))).all(dim=1)
        same32 = (out32["tables"][f].view(torch.int32) == ref["tables"][f].view(torch.int32)).all(dim=1)
        assert bool(same[same32].all())  # (a row the fp32 rule left alone keeps its bf16 bits: untouched rows, the zero gradient)
        moved += int((~same).sum())
    assert _guard_intact(out, c)
    assert moved > 0
    assert int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0


@pytest.mark.parametrize("B", [8, 300])
@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("zero", [False, True], ids=["one-launch", "zero-chunks"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("table_eps", TABLE_EPS)
def test_update_is_the_fp32_kernel_then_the_reference_rounding(B, max_norm, zero, scale, table_eps):
    ref, c = _bf16_case(B)
    # (zero_chunks: phase 0 alone on both sides — phase 1 never touches a table of this rule, and refuses bf16 ones)
    out32 = _run(ref, max_norm, zero, scale, table_eps, phases=[0], edit=_rowwise())
    out = _run(c, max_norm, zero, scale, table_eps, phases=[0], edit=_bf16())
    assert out32["rc"] == [0] and out["rc"] == [0], (out32["err"], out["err"])
    _check_against_fp32(ref, c, out32, out)
    want = list(STEPS0)
    if not zero:
        for k in INC:
            want[k] += 1
    assert out["steps"].tolist() == want
    # the touched row with an exactly zero summed gradient, and the rounding really rounds: some weight went up and some went down
    for f in range(FS):
        r = int(c["idx"][2, f])
        assert torch.equal(_i16(_table(out, f)[r]), _i16(_table(c, f)[r]))
    nearest = [out32["tables"][f].to(torch.bfloat16) for f in range(FS)]
    assert any(not torch.equal(_i16(nearest[f]), _i16(_table(out, f))) for f in range(FS)), "round to nearest, not stochastic"
    again = _run(c, max_norm, zero, scale, table_eps, phases=[0], edit=_bf16())
    for f in range(FS):
        assert torch.equal(_i16(again["tables"][f]), _i16(out["tables"][f])) and _same_bits(again["tv"][f], out["tv"][f])


@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
def test_update_reads_the_rank_layout(max_norm):
    ref, c = _bf16_case(8)
    out32 = _run(ref, max_norm, False, 160.0, ranked=True, edit=_rowwise())
    out = _run(c, max_norm, False, 160.0, ranked=True, edit=_bf16())
    assert out32["rc"] == [0] and out["rc"] == [0], (out32["err"], out["err"])
    _check_against_fp32(ref, c, out32, out)
    flat = _run(c, max_norm, False, 160.0, edit=_bf16())
    for f in range(FS):
        assert torch.equal(_i16(flat["tables"][f]), _i16(out["tables"][f]))


def test_the_rounding_depends_on_the_device_step_counter_and_the_seed(monkeypatch):
    ref, c = _bf16_case(300)
    outs = {}
    for s in (4.0, 5.0):
        steps = [0.0, 3.0, 5.0, s, s]
        monkeypatch.setattr(SK, "STEPS0", steps)
        out32 = _run(ref, 5.0, False, 160.0, edit=_rowwise())
        out = outs[s] = _run(c, 5.0, False, 160.0, edit=_bf16())  # (the SAME descriptor: only the device counter differs)
        assert out32["rc"] == [0] and out["rc"] == [0], (out32["err"], out["err"])
        _check_against_fp32(ref, c, out32, out, steps0=steps)
        assert out["steps"].tolist() == [1.0, 4.0, 5.0, s + 1, s + 1]
    for f in range(FS):
        assert not torch.equal(_i16(outs[4.0]["tables"][f]), _i16(outs[5.0]["tables"][f])), f
        assert _same_bits(outs[4.0]["tv"][f], outs[5.0]["tv"][f])
    other = _run(c, 5.0, False, 160.0, edit=_bf16(seed=SEED + 1))
    out32 = _run(ref, 5.0, False, 160.0, edit=_rowwise())
    _check_against_fp32(ref, c, out32, other, steps0=[0.0, 3.0, 5.0, 5.0, 5.0], seed=SEED + 1)
    assert any(not torch.equal(_i16(other["tables"][f]), _i16(outs[5.0]["tables"][f])) for f in range(FS))


def _set_tm(f):
    def edit(d):
        d.tm[f] = d.tv[0]
    return edit


REFUSALS = {
    "not-adam": (_set(algo=L.OPTIM_SGD), [0], False, b"table_algo"),
    "rmsprop": (_set(algo=L.OPTIM_RMSPROP), [0], False, b"table_algo"),
    "sparse-rows": (_set(sparse_rows=1), [0], False, b"sparse_rows"),
    "table-eps-zero": (_set(table_eps=0.0), [0], False, b"table_eps"),
    "table-eps-negative": (_set(table_eps=-1e-2), [0], False, b"table_eps"),
    "reg-mask": (_set(reg_mask=1), [0], False, b"reg_mask"),
    "tm-expected": (_set_tm(1), [0], False, b"tm"),
    "tm-expected-beyond-Fs": (_set_tm(L.MAX_TABLES - 1), [0], False, b"tm"),
    "phase-1": (_set(), [1], True, b"phase"),
    "phase-1-tile": (_own_a_tile, [1], True, b"phase"),
    "phase-1-without-zero-chunks": (_set(), [1], False, b"phase"),
    "phase-2": (_set(phase=2), [0], False, b"phase"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_field_and_launch_nothing(what):
    edit, phases, zero, word = REFUSALS[what]
    ref, c = _bf16_case(8)
    out = _run(c, 5.0, zero, 160.0, phases=phases, edit=_bf16(edit))
    assert out["rc"] == [-1], (out["rc"], out["err"])
    assert word in out["err"] and b"opt_moments" in out["err"], out["err"]
    for key in ("p", "m", "v", "g"):
        assert torch.equal(out[key], c[key]), key
    for f in range(FS):
        assert torch.equal(_i16(out["tables"][f]), _i16(c["tables"][f])) and _same_bits(out["tv"][f], c["tv"][f])
    assert out["steps"].tolist() == STEPS0 and int(out["bitmap"].abs().sum()) == 0 and int(out["counter"][0]) == 0
    assert out["clip"].tolist() == [0.0, 0.0]


def test_table_algo_2_is_still_unknown_and_5_is_too():
    ref, c = _bf16_case(8)
    for v in (2, 5):
        out = _run(c, 5.0, False, 160.0, phases=[0], edit=_bf16(_set(table_algo=v)))
        assert out["rc"] == [-1] and ("table_algo %d" % v).encode() in out["err"], (out["rc"], out["err"])


# ------------------------------------------------------------------------------------------------------------------ the gather
def _patterns(n, seed):
    """[n, 16] bf16 holding every class of pattern: +-0, denormals, +-inf, NaNs (quiet, signalling, payloads), the extremes, ordinary"""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-32768, 32768, (n, 16), generator=g, dtype=torch.int64)
    special = [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0x7FFF, 0xFFFF, 0x7F7F, 0xFF7F, 0x0080]
    bits[0] = torch.tensor([s - 65536 if s >= 32768 else s for s in special])
    return bits.to(torch.int16).view(torch.bfloat16)


def _gather(tables, idx, dtype_code, stage, out_fill=float("nan")):
    dev = torch.device("cuda", 0)
    B, Fs = idx.shape
    tabs = [t.to(dev) for t in tables]
    ids = idx.to(dev)
    out = torch.full((B, Fs, 16), out_fill, device=dev)
    oob = torch.zeros(1, dtype=torch.int32, device=dev)
    g = L.EmbedDesc()
    g.kind, g.B, g.Fs, g.table_dtype = L.OP_EMBED_GATHER, B, Fs, dtype_code
    g.idx, g.out, g.oob = ids.data_ptr(), out.data_ptr(), oob.data_ptr()
    for f in range(Fs):
        g.table[f], g.rows[f] = tabs[f].data_ptr(), tabs[f].shape[0]
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    if not stage:
        rc = lib.nasrec_embedding_gather(s, C.addressof(g))
        staged = None
    else:
        int_src = torch.arange(B * 3, dtype=torch.float32, device=dev).view(B, 3)
        int_dst, cat_dst = torch.zeros_like(int_src), torch.zeros_like(ids)
        st = L.StageDesc()
        st.kind, st.B, st.Fd, st.Fs = L.OP_STAGE_INPUTS, B, 3, Fs
        st.int_src, st.int_dst, st.cat_src, st.cat_dst = int_src.data_ptr(), int_dst.data_ptr(), ids.data_ptr(), cat_dst.data_ptr()
        st.gather = g
        st.gather.idx = None  # (ignored: the ids are cat_src)
        rc = lib.nasrec_launch(s, C.addressof(st))
        staged = (int_src, int_dst, ids, cat_dst)
    err = lib.nasrec_last_error()
    torch.cuda.synchronize()
    if staged is not None and rc == 0:
        assert torch.equal(staged[0], staged[1]) and torch.equal(staged[2], staged[3])
    return rc, err, out.cpu(), int(oob.cpu()[0])


def _ids(B, rows, bad, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in rows], 1)
    idx[0] = torch.tensor([n - 1 for n in rows])  # the last row
    if bad:
        idx[B // 2, 0] = rows[0]          # at the table end
        idx[B - 1, -1] = rows[-1] + 9     # past it
        if B > 2:
            idx[1, 0] = -1
    return idx


@pytest.mark.parametrize("stage", [False, True], ids=["stand-alone", "on-the-staging-launch"])
@pytest.mark.parametrize("bad", [False, True], ids=["ids-in-range", "ids-at-and-past-the-end"])
@pytest.mark.parametrize("Fs", [1, 3])
@pytest.mark.parametrize("B", [1, 3, 256, 257])
def test_gather_widens_exactly(B, Fs, bad, stage):
    rows = [1, 70, 100][:Fs] if Fs == 3 else [70]
    tables = [_patterns(n, 40 + n) for n in rows]
    idx = _ids(B, rows, bad, 7 * B + Fs)
    rc, err, out, oob = _gather(tables, idx, L.TABLE_DTYPE_BF16, stage)
    assert rc == 0, err
    want = torch.zeros(B, Fs, 16)
    ok = torch.zeros(B, Fs, dtype=torch.bool)
    for f in range(Fs):
        ok[:, f] = (idx[:, f] >= 0) & (idx[:, f] < rows[f])
        want[ok[:, f], f] = tables[f].float()[idx[ok[:, f], f]]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    # (the widening itself, spelled out: the 16 bits in the upper half, zeros below)
    assert torch.equal(out.view(torch.int32)[ok] >> 16, torch.stack([tables[f].view(torch.int16)[idx[:, f].clamp(0, rows[f] - 1)] for f in range(Fs)], 1)[ok].to(torch.int32))
    assert bool(((out.view(torch.int32) & 0xFFFF) == 0).all())
    assert oob == int(not bool(ok.all()))
    assert bool(ok.all()) != bad


def test_gather_of_a_one_row_table():
    tables = [_patterns(1, 3)]
    for B in (1, 257):
        rc, err, out, oob = _gather(tables, torch.zeros(B, 1, dtype=torch.int64), L.TABLE_DTYPE_BF16, False)
        assert rc == 0 and oob == 0 and torch.equal(out.view(torch.int32), tables[0].float().expand(B, 16).reshape(B, 1, 16).contiguous().view(torch.int32))


@pytest.mark.parametrize("stage", [False, True], ids=["stand-alone", "on-the-staging-launch"])
def test_an_unknown_table_dtype_is_refused_with_nothing_written(stage):
    tables = [_patterns(70, 1)]
    for code in (2, -1):
        rc, err, out, oob = _gather(tables, _ids(8, [70], False, 1), code, stage)
        assert rc == -1 and b"table_dtype" in err, (rc, err)
        assert bool(torch.isnan(out).all()) and oob == 0


@pytest.mark.parametrize("stage", [False, True], ids=["stand-alone", "on-the-staging-launch"])
@pytest.mark.parametrize("B", [3, 257])
def test_table_dtype_0_is_the_fp32_gather(B, stage):
    g = torch.Generator().manual_seed(2)
    rows = [70, 100]
    tables = [torch.randn(n, 16, generator=g) for n in rows]
    tables[0][0, :4] = torch.tensor([0.0, -0.0, float("inf"), 1e-42])
    idx = _ids(B, rows, True, B)
    rc, err, out, oob = _gather(tables, idx, L.TABLE_DTYPE_F32, stage)
    assert rc == 0 and oob == 1, err
    want = torch.zeros(B, 2, 16)
    for f in range(2):
        ok = (idx[:, f] >= 0) & (idx[:, f] < rows[f])
        want[ok, f] = tables[f][idx[ok, f]]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
