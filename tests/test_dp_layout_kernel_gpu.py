"""Phase 0 of NASREC_OP_WEIGHT_DECAY and of NASREC_OP_OPT_MOMENTS read a leader's summed row where the data-parallel dedup leaves it: in
one contiguous [B, Fs, 16] array (rank_B = 0), or in the receive buffer of the row-gradient all-gather, whose per-rank chunks of rank_B
samples lie rank_stride floats apart with the packed dense-gradient tail between them (include/nasrec_hip.h).  The same rows in either
layout give the same bits: parameters, gradients, moments, the clip's partial sums, the row bitmap; the gap is never read or written."""
import ctypes as C

import pytest
import torch

from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu
ROWS = [100, 70, 33]
B, FS, RANKS, GAP = 8, 3, 2, 36  # two ranks of 4 samples; 36 floats of something else behind each rank's rows
N_DENSE = 200


def _case():
    g = torch.Generator().manual_seed(5)
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in ROWS], 1)
    idx[5] = idx[1]          # a duplicate across the two ranks' halves: only sample 1 leads
    idx[6, 2] = idx[0, 2]
    idx[7, 0] = ROWS[0]      # out of range
    leader = torch.zeros(B, FS, dtype=torch.int32)
    for f in range(FS):
        seen = set()
        for b in range(B):
            if int(idx[b, f]) not in seen:
                leader[b, f] = 1
                seen.add(int(idx[b, f]))
    return dict(idx=idx, leader=leader, gsum=torch.randn(B, FS, 16, generator=g), tables=[torch.randn(n, 16, generator=g) for n in ROWS],
                tm=[torch.randn(n, 16, generator=g) * 0.1 for n in ROWS], tv=[torch.rand(n, 16, generator=g) * 0.01 for n in ROWS],
                p=torch.randn(N_DENSE, generator=g), g=torch.randn(N_DENSE, generator=g), m=torch.randn(N_DENSE, generator=g) * 0.1,
                v=torch.rand(N_DENSE, generator=g) * 0.01)


def _rows_buffer(gsum, ranked):
    """(device buffer, (rank_B, rank_stride)): the rows contiguous, or per rank behind each other with a NaN-filled gap"""
    dev = torch.device("cuda", 0)
    if not ranked:
        return gsum.clone().to(dev), (0, 0)
    rb = B // RANKS
    stride = rb * FS * 16 + GAP
    buf = torch.full((RANKS * stride,), float("nan"))
    for r in range(RANKS):
        buf[r * stride:r * stride + rb * FS * 16] = gsum[r * rb:(r + 1) * rb].reshape(-1)
    return buf.to(dev), (rb, stride)


def _unpack(buf, layout):
    if layout[0] == 0:
        return buf.cpu().view(B, FS, 16)
    rb, stride = layout
    cpu = buf.cpu()
    assert torch.isnan(torch.cat([cpu[r * stride + rb * FS * 16:(r + 1) * stride] for r in range(RANKS)])).all(), "the gap was written"
    return torch.cat([cpu[r * stride:r * stride + rb * FS * 16].view(rb, FS, 16) for r in range(RANKS)])


def _weight_decay_phase0(c, ranked):
    dev = torch.device("cuda", 0)
    nblocks, wd = 4, 0.05
    tables = [t.clone().to(dev) for t in c["tables"]]
    p, gd = c["p"].clone().to(dev), c["g"].clone().to(dev)
    gsum, layout = _rows_buffer(c["gsum"], ranked)
    idx, leader = c["idx"].to(dev), c["leader"].to(dev)
    add, setc = [(0, 50), (100, 30)], [(60, 20), (150, 7)]
    chunks = torch.tensor([v for ch in add + setc for v in ch], dtype=torch.int64, device=dev)
    bitmap = torch.zeros(sum(2 * ((n + 63) // 64) for n in ROWS), dtype=torch.int32, device=dev)
    part = torch.zeros(2 * nblocks, dtype=torch.float64, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    clip_partial = torch.zeros(1, dtype=torch.float32, device=dev)
    l2 = torch.zeros(1, dtype=torch.float64, device=dev)
    d = L.WeightDecayDesc()
    d.kind, d.phase, d.nblocks, d.B, d.Fs, d.wd, d.eps = L.OP_WEIGHT_DECAY, 0, nblocks, B, FS, wd, 1e-2
    d.idx, d.leader, d.gsum = idx.data_ptr(), leader.data_ptr(), gsum.data_ptr()
    d.rank_B, d.rank_stride = layout
    t = 0
    for f in range(FS):
        d.table[f], d.rows[f], d.tile_off[f] = tables[f].data_ptr(), ROWS[f], t
        if f != 1:  # table 1 is not regularised
            d.reg_mask |= 1 << f
            t += (ROWS[f] + 63) // 64
    d.tile_off[FS] = t
    d.bitmap, d.p, d.g = bitmap.data_ptr(), p.data_ptr(), gd.data_ptr()
    d.add_chunks, d.n_add = chunks.data_ptr(), len(add)
    d.set_chunks, d.n_set = chunks.data_ptr() + 8 * 2 * len(add), len(setc)
    d.block_part, d.counter, d.clip_partial, d.l2_sumsq = part.data_ptr(), counter.data_ptr(), clip_partial.data_ptr(), l2.data_ptr()
    L.check(L.load().nasrec_weight_decay(torch.cuda.current_stream().cuda_stream, C.addressof(d)))
    torch.cuda.synchronize()
    return dict(gsum=_unpack(gsum, layout), g=gd.cpu(), tables=[x.cpu() for x in tables], bitmap=bitmap.cpu(), clip=clip_partial.cpu(),
                l2=l2.cpu())


def _moments_phase0(c, ranked, kind):
    dev = torch.device("cuda", 0)
    tables, tm, tv = ([x.clone().to(dev) for x in c[k]] for k in ("tables", "tm", "tv"))
    p, gd, m, v = (c[k].clone().to(dev) for k in ("p", "g", "m", "v"))
    gsum, layout = _rows_buffer(c["gsum"], ranked)
    idx, leader = c["idx"].to(dev), c["leader"].to(dev)
    trip = [(0, 37, 0), (40, 32, 1), (72, 30, 1)]
    tab = torch.tensor([x for ch in trip for x in ch], dtype=torch.int64, device=dev)
    steps = torch.tensor([0.0, 3.0, 5.0, 2.0, 0.0, 1.0], dtype=torch.float32, device=dev)  # dense 0..2, tables at table_step0 = 3
    bitmap = torch.zeros(sum(2 * ((n + 63) // 64) for n in ROWS), dtype=torch.int32, device=dev)
    partial = torch.tensor([40.0, 60.0], dtype=torch.float32, device=dev)  # norm 10: the clip binds at 5
    clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
    lr = torch.tensor([0.01], dtype=torch.float32, device=dev)
    d = L.OptMomentsDesc()
    d.kind, d.phase = L.OP_OPT_MOMENTS, 0
    d.algo = L.OPTIM_ADAM if kind == "adam" else L.OPTIM_SGD
    d.nesterov, d.dense_blocks, d.nblocks = 1, 2, 3
    d.B, d.Fs, d.table_step0 = B, FS, 3
    d.eps, d.momentum, d.beta1, d.beta2 = 1e-8, 0.9, 0.9, 0.999
    d.clip.kind, d.clip.n_a, d.clip.n_b, d.clip.max_norm = L.OP_CLIP_COEF, 2, 0, 5.0
    d.clip.partial_a, d.clip.out = partial.data_ptr(), clip_out.data_ptr()
    d.chunks, d.nchunks = tab.data_ptr(), len(trip)
    d.p, d.g, d.m = p.data_ptr(), gd.data_ptr(), m.data_ptr()
    d.v = v.data_ptr() if kind == "adam" else None
    d.idx, d.leader, d.gsum = idx.data_ptr(), leader.data_ptr(), gsum.data_ptr()
    d.rank_B, d.rank_stride = layout
    off = 0
    for f in range(FS):
        d.table[f], d.tm[f], d.rows[f], d.tile_off[f] = tables[f].data_ptr(), tm[f].data_ptr(), ROWS[f], off
        if kind == "adam":
            d.tv[f] = tv[f].data_ptr()
        off += (ROWS[f] + 63) // 64
    d.tile_off[FS] = off
    d.bitmap, d.step, d.lr, d.coef = bitmap.data_ptr(), steps.data_ptr(), lr.data_ptr(), clip_out.data_ptr()
    L.check(L.load().nasrec_opt_moments(torch.cuda.current_stream().cuda_stream, C.addressof(d)))
    torch.cuda.synchronize()
    return dict(gsum=_unpack(gsum, layout), tables=[x.cpu() for x in tables], tm=[x.cpu() for x in tm], tv=[x.cpu() for x in tv],
                p=p.cpu(), m=m.cpu(), v=v.cpu(), bitmap=bitmap.cpu(), clip=clip_out.cpu())


def _same(a, b, what=""):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _same(a[k], b[k], what + "." + k)
    elif isinstance(a, list):
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, i))
    else:
        assert torch.equal(a, b), what


def test_weight_decay_phase0_reads_the_rank_layout():
    c = _case()
    flat, ranked = _weight_decay_phase0(c, False), _weight_decay_phase0(c, True)
    _same(flat, ranked)
    assert not torch.equal(flat["gsum"], c["gsum"])  # (the leaders' rows did change: 2 wd W was added in place)
    assert float(flat["clip"]) != 0.0 and int(flat["bitmap"].abs().sum()) > 0


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_opt_moments_phase0_reads_the_rank_layout(kind):
    c = _case()
    flat, ranked = _moments_phase0(c, False, kind), _moments_phase0(c, True, kind)
    _same(flat, ranked)
    assert any(not torch.equal(a, b) for a, b in zip(flat["tables"], c["tables"]))  # (touched rows moved)


def test_launchers_refuse_a_rank_layout_that_does_not_hold_the_rows():
    d = L.WeightDecayDesc()
    d.kind, d.phase, d.nblocks, d.B, d.Fs = L.OP_WEIGHT_DECAY, 0, 1, B, FS
    dummy = torch.zeros(16, dtype=torch.float64, device="cuda")
    d.block_part = d.counter = d.clip_partial = d.l2_sumsq = dummy.data_ptr()
    d.rank_B, d.rank_stride = 4, 4 * FS * 16 - 4  # chunks closer than the rows they hold
    lib = L.load()
    assert lib.nasrec_weight_decay(torch.cuda.current_stream().cuda_stream, C.addressof(d)) != 0
