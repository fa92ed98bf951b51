"""NASREC_OP_COWCLIP (include/nasrec_hip.h; csrc/cowclip.hip) through the C-ABI against an fp64 NumPy restatement of the rule:
G = coef ||g||, T = cnt max(r ||w||, zeta), a row with G > T is scaled by T / G, every other row keeps its bits.  Tables of 100, 70 and
1 rows (Fs = 3) or the first alone (Fs = 1); B = 1, 3 (one id three times: cnt = 3 triples the threshold), 8 (duplicates, ids at -1,
at the table end and past it), 64 / 65 (Fs = 1: exactly one row workgroup, and one pair more) and 300 (several workgroups); the global
clip active and off; (r, zeta) = (1, 1e-5), (0.05, 1e-5), (1, 0.5) (zeta wins); from five touched rows on, one with an all-zero
gradient, one with all-zero weights and one whose gradient holds a NaN.  The bar on clipped rows is the split optimizer kernel test's
(rtol 2e-6, atol 2e-7): the rule adds one square root, one division and one product per element, a few ulp each.

The gradients are sized from the thresholds: row k gets G = phi_k T with phi_k drawn log-uniformly from [1/4, 1/1.5] or [1.5, 4], so in
fp64 every case has clipped and unclipped rows and no row within 1e-3 of its threshold (asserted below): no decision is ambiguous."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu

ROWS3 = [100, 70, 1]
RZ = [(1.0, 1e-5), (0.05, 1e-5), (1.0, 0.5)]
NAN_BITS = 0x7FC00ABC  # what the non-leader rows of gsum hold
SHAPES = [(1, 3), (3, 3), (8, 3), (64, 3), (65, 3), (300, 3), (8, 1), (64, 1), (65, 1), (300, 1)]


def _coef(max_norm):
    """clip_coef_wave on partials 40 + 60: total 10"""
    return float(np.float32(max_norm) / (np.float32(10.0) + np.float32(1e-6))) if max_norm else 1.0


def _ids(B, rows, rng):
    n = np.array(rows, np.int64)
    if B == 1:
        return (n // 2)[None, :].copy()
    if B == 3:
        return np.repeat(np.minimum(5, n - 1)[None, :], 3, axis=0)
    if B == 8:  # duplicates, -1, the last row, one past it
        cols = []
        for m in rows:
            cols.append([2, 2, m - 1, -1, m, 7, 11, 13] if m > 13 else [0, 0, m - 1, -1, m, 0, 0, 0])
        return np.array(cols, np.int64).T.copy()
    idx = np.stack([rng.integers(0, m, size=B) for m in rows], axis=1).astype(np.int64)
    idx[1, :] = idx[0, :]  # (at least one duplicate per field)
    idx[B // 2, 0] = -1
    idx[B // 2 + 1, 0] = rows[0]
    return idx


def _case(B, Fs, max_norm, r, zeta, seed=5):
    rng = np.random.default_rng(seed + 1000 * B + Fs)
    rows = ROWS3[:Fs]
    idx = _ids(B, rows, rng)
    leader = np.zeros((B, Fs), np.int32)
    for f in range(Fs):
        seen = set()
        for b in range(B):
            if int(idx[b, f]) not in seen:  # (an id outside the table has a leader too: the kernel must skip it)
                seen.add(int(idx[b, f]))
                leader[b, f] = 1
    tables = [(0.05 * rng.standard_normal((m, 16))).astype(np.float32) for m in rows]
    cnt = [np.bincount(idx[:, f][(idx[:, f] >= 0) & (idx[:, f] < rows[f])], minlength=rows[f]).astype(np.int64) for f in range(Fs)]
    touched = [(b, f) for b in range(B) for f in range(Fs) if leader[b, f] and 0 <= idx[b, f] < rows[f]]
    special = {}
    if len(touched) >= 5:
        special = {"zero_g": touched[1], "zero_w": touched[2], "nan": touched[3]}
        b, f = special["zero_w"]
        tables[f][idx[b, f]] = 0.0
    coef = _coef(max_norm)
    r32, z32 = float(np.float32(r)), float(np.float32(zeta))
    gsum = np.full((B, Fs, 16), np.nan, np.float32)
    gsum.view(np.uint32)[...] = NAN_BITS
    k = 0
    for (b, f) in touched:
        w = tables[f][idx[b, f]].astype(np.float64)
        T = cnt[f][idx[b, f]] * max(r32 * np.sqrt((w * w).sum()), z32)
        if B == 3:
            phi = [3.0, 0.5, 0.5][k % 3]  # (0.5 of three times the threshold: over it with cnt = 1)
        elif k % 2 == 0:
            phi = float(np.exp(rng.uniform(np.log(1.5), np.log(4.0))))
        else:
            phi = float(np.exp(-rng.uniform(np.log(1.5), np.log(4.0))))
        if (b, f) == special.get("zero_w"):
            phi = 2.5
        u = rng.standard_normal(16)
        u /= np.sqrt((u * u).sum())
        gsum[b, f] = (u * (phi * T / coef)).astype(np.float32)
        k += 1
    if special:
        b, f = special["zero_g"]
        gsum[b, f] = 0.0
        b, f = special["nan"]
        gsum[b, f, 3] = np.nan
    return {"B": B, "Fs": Fs, "rows": rows, "idx": idx, "leader": leader, "tables": tables, "gsum": gsum, "cnt": cnt, "touched": touched,
            "special": special, "max_norm": max_norm, "coef": coef, "r": r, "zeta": zeta}


def _restate(c, cnt_override=None):
    """the rule in fp64 on the fp32 inputs -> (gsum fp64, clipped flags by pair, ratios G / T, rows where zeta won)"""
    out = c["gsum"].astype(np.float64)
    r32, z32 = float(np.float32(c["r"])), float(np.float32(c["zeta"]))
    clipped, ratio, zeta_won = {}, {}, 0
    for (b, f) in c["touched"]:
        row = c["idx"][b, f]
        g, w = c["gsum"][b, f].astype(np.float64), c["tables"][f][row].astype(np.float64)
        n = c["cnt"][f][row] if cnt_override is None else cnt_override
        rw = r32 * np.sqrt((w * w).sum())
        zeta_won += rw < z32
        G, T = c["coef"] * np.sqrt((g * g).sum()), n * max(rw, z32)
        ratio[(b, f)] = G / T
        clipped[(b, f)] = bool(G > T)
        if G > T:
            out[b, f] = g * (T / G)
    return out, clipped, ratio, zeta_won


def _check_case(c):
    """what keeps the test from hiding a failure: both kinds of rows in every case, and no decision near its threshold"""
    _, clipped, ratio, zeta_won = _restate(c)
    assert any(clipped.values()) and not all(clipped.values()), "a case needs clipped and unclipped rows"
    for k, v in ratio.items():
        assert np.isnan(v) or abs(v - 1.0) > 1e-3, (k, v)
    if c["zeta"] == 0.5:  # (weights of 0.05 N(0, 1): every row's norm is far below 0.5)
        assert zeta_won == len(c["touched"])
    else:  # (only the row of zero weights falls back to zeta)
        assert zeta_won == (1 if c["special"] else 0)
    if c["special"]:
        assert not clipped[c["special"]["zero_g"]] and clipped[c["special"]["zero_w"]] and not clipped[c["special"]["nan"]]
        assert np.isnan(ratio[c["special"]["nan"]])


def _run(c, phases=(0, 1), edit=None, cnt0=None, stat=True):
    dev = torch.device("cuda", 0)
    B, Fs = c["B"], c["Fs"]
    idx, leader = torch.from_numpy(c["idx"]).to(dev), torch.from_numpy(c["leader"]).to(dev)
    gsum = torch.from_numpy(c["gsum"]).to(dev)
    tables = [torch.from_numpy(t).to(dev) for t in c["tables"]]
    cnt = [torch.zeros(m, dtype=torch.int32, device=dev) if cnt0 is None else torch.from_numpy(cnt0[f].astype(np.int32)).to(dev)
           for f, m in enumerate(c["rows"])]
    partial = torch.tensor([40.0, 60.0], dtype=torch.float32, device=dev)
    clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    d = L.CowClipDesc()
    d.kind, d.B, d.Fs, d.r, d.zeta = L.OP_COWCLIP, B, Fs, c["r"], c["zeta"]
    d.idx, d.leader, d.gsum = idx.data_ptr(), leader.data_ptr(), gsum.data_ptr()
    for f in range(Fs):
        d.table[f], d.cnt[f], d.rows[f] = tables[f].data_ptr(), cnt[f].data_ptr(), c["rows"][f]
    d.clip.kind, d.clip.n_a, d.clip.n_b, d.clip.max_norm = L.OP_CLIP_COEF, 2, 0, c["max_norm"]
    d.clip.partial_a, d.clip.out = partial.data_ptr(), clip_out.data_ptr()
    d.stat = st.data_ptr() if stat else None
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    rcs, errs = [], []
    for ph in phases:
        x = L.CowClipDesc.from_buffer_copy(d)
        x.phase = ph
        if edit is not None:
            edit(x)
        rcs.append(lib.nasrec_launch(s, C.addressof(x)))
        errs.append(lib.nasrec_last_error() if rcs[-1] else b"")
    torch.cuda.synchronize()
    return {"rc": rcs, "err": errs, "gsum": gsum.cpu().numpy(), "tables": [t.cpu().numpy() for t in tables], "idx": idx.cpu().numpy(),
            "leader": leader.cpu().numpy(), "cnt": [x.cpu().numpy() for x in cnt], "clip": clip_out.cpu().numpy(), "stat": st.cpu().numpy()}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _inputs_untouched(out, c):
    assert np.array_equal(out["idx"], c["idx"]) and np.array_equal(out["leader"], c["leader"])
    for f in range(c["Fs"]):
        assert np.array_equal(_bits(out["tables"][f]), _bits(c["tables"][f])), f


@pytest.mark.parametrize("B,Fs", SHAPES)
@pytest.mark.parametrize("max_norm", [5.0, 0.0], ids=["clip-active", "clip-off"])
@pytest.mark.parametrize("r,zeta", RZ)
def test_cowclip_kernel_against_fp64(B, Fs, max_norm, r, zeta):
    c = _case(B, Fs, max_norm, r, zeta)
    _check_case(c)
    want, clipped, _, _ = _restate(c)
    out = _run(c)
    assert out["rc"] == [0, 0], (out["rc"], out["err"])
    assert float(out["clip"][0]) == c["coef"] and abs(float(out["clip"][1]) - 10.0) < 1e-5
    assert (c["coef"] < 1.0) == bool(max_norm)
    got = out["gsum"]
    for b in range(B):
        for f in range(Fs):
            if clipped.get((b, f)):
                err = np.abs(got[b, f].astype(np.float64) - want[b, f])
                bound = 2e-7 + 2e-6 * np.abs(want[b, f])
                assert (err <= bound).all(), ((b, f), float((err / bound).max()))
                assert not np.array_equal(_bits(got[b, f]), _bits(c["gsum"][b, f]))
            else:  # unclipped leaders, the NaN row, the zero row, ids outside the table, every non-leader row (the NaN pattern)
                assert np.array_equal(_bits(got[b, f]), _bits(c["gsum"][b, f])), (b, f)
    _inputs_untouched(out, c)
    assert all(int(np.abs(x).sum()) == 0 for x in out["cnt"]), "the scratch must be all zero again"
    assert out["stat"].tolist() == [len(c["touched"]), sum(clipped.values())]
    again = _run(c)
    assert np.array_equal(_bits(again["gsum"]), _bits(got)) and again["stat"].tolist() == out["stat"].tolist()
    nostat = _run(c, stat=False)
    assert nostat["rc"] == [0, 0] and np.array_equal(_bits(nostat["gsum"]), _bits(got)) and nostat["stat"].tolist() == [0, 0]


@pytest.mark.parametrize("B,Fs", SHAPES)
def test_phase_0_counts_the_in_range_ids(B, Fs):
    c = _case(B, Fs, 5.0, 1.0, 1e-5)
    out = _run(c, phases=(0,))
    assert out["rc"] == [0], (out["rc"], out["err"])
    for f in range(Fs):
        col = c["idx"][:, f]
        assert np.array_equal(out["cnt"][f], np.bincount(col[(col >= 0) & (col < c["rows"][f])], minlength=c["rows"][f])), f
    assert np.array_equal(_bits(out["gsum"]), _bits(c["gsum"])) and out["clip"].tolist() == [0.0, 0.0] and out["stat"].tolist() == [0, 0]
    _inputs_untouched(out, c)


def test_the_count_scales_the_threshold():
    """B = 3, one id three times: the rows at half of cnt = 3 thresholds pass; restated with cnt = 1 they would be clipped"""
    c = _case(3, 3, 5.0, 1.0, 1e-5)
    assert all(int(c["cnt"][f].max()) == 3 for f in range(3))
    want3, clipped3, _, _ = _restate(c)
    want1, clipped1, _, _ = _restate(c, cnt_override=1)
    assert sum(clipped3.values()) == 1 and sum(clipped1.values()) == 3
    out = _run(c)
    assert out["rc"] == [0, 0] and out["stat"].tolist() == [3, 1]
    for (b, f) in c["touched"]:
        if clipped3[(b, f)]:
            assert np.allclose(out["gsum"][b, f], want3[b, f], rtol=2e-6, atol=2e-7)
            assert not np.allclose(out["gsum"][b, f], want1[b, f], rtol=1e-2, atol=0)  # (a third of it)
        else:
            assert np.array_equal(_bits(out["gsum"][b, f]), _bits(c["gsum"][b, f]))
            assert not np.allclose(c["gsum"][b, f], want1[b, f], rtol=1e-2, atol=0)


def test_an_empty_batch_is_an_empty_launch():
    c = _case(8, 3, 5.0, 1.0, 1e-5)
    out = _run(c, edit=lambda d: setattr(d, "B", 0))
    assert out["rc"] == [0, 0], out["err"]
    assert np.array_equal(_bits(out["gsum"]), _bits(c["gsum"])) and out["stat"].tolist() == [0, 0] and out["clip"].tolist() == [0.0, 0.0]
    assert all(int(np.abs(x).sum()) == 0 for x in out["cnt"])


def _set(**kw):
    def edit(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return edit


def _drop(name, f):
    def edit(d):
        getattr(d, name)[f] = None
    return edit


def _no_clip_out(d):
    d.clip.out = None


REFUSALS = {
    "Fs-too-large": (_set(Fs=L.MAX_TABLES + 1), (0, 1), b"Fs"),
    "Fs-negative": (_set(Fs=-1), (0, 1), b"Fs"),
    "B-negative": (_set(B=-1), (0, 1), b"B = -1"),
    "idx": (_set(idx=None), (0, 1), b"idx"),
    "leader": (_set(leader=None), (1,), b"leader"),
    "gsum": (_set(gsum=None), (1,), b"gsum"),
    "cnt": (_drop("cnt", 1), (0, 1), b"cnt[1]"),
    "table": (_drop("table", 2), (1,), b"table[2]"),
    "r-negative": (_set(r=-0.5), (0, 1), b"r "),
    "zeta-zero": (_set(zeta=0.0), (0, 1), b"zeta"),
    "zeta-negative": (_set(zeta=-1e-5), (0, 1), b"zeta"),
    "zeta-nan": (_set(zeta=float("nan")), (0, 1), b"zeta"),
    "phase": (_set(phase=2), (1,), b"phase"),
    "clip-out": (_no_clip_out, (1,), b"clip"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_field_and_launch_nothing(what):
    edit, phases, word = REFUSALS[what]
    c = _case(8, 3, 5.0, 1.0, 1e-5)
    for ph in phases:
        out = _run(c, phases=(ph,), edit=edit, cnt0=c["cnt"])
        assert out["rc"] == [-1], (out["rc"], out["err"])
        assert word in out["err"][0] and b"cowclip" in out["err"][0], out["err"]
        assert np.array_equal(_bits(out["gsum"]), _bits(c["gsum"]))
        _inputs_untouched(out, c)
        assert all(np.array_equal(out["cnt"][f], c["cnt"][f]) for f in range(3))
        assert out["clip"].tolist() == [0.0, 0.0] and out["stat"].tolist() == [0, 0]
