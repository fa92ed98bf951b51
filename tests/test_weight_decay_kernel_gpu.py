"""NASREC_OP_WEIGHT_DECAY through the C-ABI against fp64 torch (include/nasrec_hip.h): small tables whose rows do not fill a tile,
duplicate ids, out-of-range ids, a table outside the regularised set, dense ranges the backward reached and ones it did not; phase 1
with the clip active and inactive.  And the fused step against the torch route where the clip binds, at batch sizes that take each
of the optimizer programs (B <= 256 and 512: the two-halves dedup; 4096: the one-launch dedup + merge)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd.supernet.supernet import SuperNet, ops_config_lib
from nasrec_amd.utils import train_utils as TU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(d):
    lib = L.load()
    L.check(lib.nasrec_weight_decay(torch.cuda.current_stream().cuda_stream, C.addressof(d)))


@pytest.mark.parametrize("coef", [1.0, 0.37])
def test_weight_decay_kernel_against_fp64(coef):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    wd, lr, eps, nblocks = 0.05, 0.1, 1e-2, 4
    rows = [100, 70, 33]   # 2, 2 and 1 tiles of 64 rows, none full at the end
    reg = [0, 2]           # table 1 is not regularised (no_reg_param_name)
    B, Fs = 8, 3
    tables = [torch.randn(n, 16, generator=g).to(dev) for n in rows]
    state = [torch.rand(n, 16, generator=g).to(dev) for n in rows]
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in rows], 1)
    idx[3] = idx[1]          # duplicates: only the first occurrence leads
    idx[6, 2] = idx[0, 2]
    idx[5, 0] = rows[0]      # out of range (one past the end)
    idx[7, 2] = -1           # out of range (negative)
    leader = torch.zeros(B, Fs, dtype=torch.int32)
    for f in range(Fs):
        seen = set()
        for b in range(B):
            v = int(idx[b, f])
            if v not in seen:
                leader[b, f] = 1
                seen.add(v)
    gsum = torch.randn(B, Fs, 16, generator=g)
    n_dense = 200
    p = torch.randn(n_dense, generator=g)
    gd = torch.randn(n_dense, generator=g)
    add, setc = [(0, 50), (100, 30)], [(60, 20), (150, 7)]
    chunks = torch.tensor([v for c in add + setc for v in c], dtype=torch.int64, device=dev)
    words = sum(2 * ((n + 63) // 64) for n in rows)
    bitmap = torch.zeros(words, dtype=torch.int32, device=dev)
    part = torch.zeros(2 * nblocks, dtype=torch.float64, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    clip_partial = torch.zeros(1, dtype=torch.float32, device=dev)
    l2 = torch.zeros(1, dtype=torch.float64, device=dev)
    lr_dev = torch.tensor([lr], device=dev)
    coef_dev = torch.tensor([coef, 0.0], device=dev)
    idx_d, leader_d, gsum_d, p_d, g_d = idx.to(dev), leader.to(dev), gsum.clone().to(dev), p.clone().to(dev), gd.clone().to(dev)
    t0 = [t.cpu().double() for t in tables]
    s0 = [t.cpu().double() for t in state]

    d = L.WeightDecayDesc()
    d.kind, d.phase, d.nblocks, d.B, d.Fs, d.wd, d.eps = L.OP_WEIGHT_DECAY, 0, nblocks, B, Fs, wd, eps
    d.idx, d.leader, d.gsum = idx_d.data_ptr(), leader_d.data_ptr(), gsum_d.data_ptr()
    t = 0
    for f in range(Fs):
        d.table[f], d.state[f], d.rows[f], d.tile_off[f] = tables[f].data_ptr(), state[f].data_ptr(), rows[f], t
        if f in reg:
            d.reg_mask |= 1 << f
            t += (rows[f] + 63) // 64
    d.tile_off[Fs] = t
    d.bitmap, d.p, d.g = bitmap.data_ptr(), p_d.data_ptr(), g_d.data_ptr()
    d.add_chunks, d.n_add = chunks.data_ptr(), len(add)
    d.set_chunks, d.n_set = chunks.data_ptr() + 8 * 2 * len(add), len(setc)
    d.block_part, d.counter, d.clip_partial, d.l2_sumsq = part.data_ptr(), counter.data_ptr(), clip_partial.data_ptr(), l2.data_ptr()
    d.lr, d.coef = lr_dev.data_ptr(), coef_dev.data_ptr()
    _launch(d)
    torch.cuda.synchronize()

    # ---- phase 0 against fp64
    pd, gd64 = p.double(), gd.double()
    g_want = gd64.clone()
    ex, ssum = 0.0, 0.0
    for o, n in add:
        g_want[o:o + n] = gd64[o:o + n] + 2 * wd * pd[o:o + n]
        ex += float((g_want[o:o + n] ** 2 - gd64[o:o + n] ** 2).sum())
        ssum += float((pd[o:o + n] ** 2).sum())
    for o, n in setc:
        g_want[o:o + n] = 2 * wd * pd[o:o + n]
        ex += float((g_want[o:o + n] ** 2).sum())
        ssum += float((pd[o:o + n] ** 2).sum())
    assert torch.allclose(g_d.cpu().double(), g_want, rtol=1e-6, atol=1e-7)
    g_after0 = g_d.cpu().clone()
    touched = [set() for _ in range(Fs)]
    gs_want = gsum.double().clone()
    for b in range(B):
        for f in range(Fs):
            r = int(idx[b, f])
            if f in reg and leader[b, f] and 0 <= r < rows[f]:
                touched[f].add(r)
                gs_want[b, f] = gsum[b, f].double() + 2 * wd * t0[f][r]
                ex += float((gs_want[b, f] ** 2 - gsum[b, f].double() ** 2).sum())
    assert torch.allclose(gsum_d.cpu().double(), gs_want, rtol=1e-6, atol=1e-7)  # out-of-range and unregularised rows untouched
    for f in reg:
        ssum += float((t0[f] ** 2).sum())
        untouched = [r for r in range(rows[f]) if r not in touched[f]]
        ex += float(((2 * wd * t0[f][untouched]) ** 2).sum())
    assert abs(float(l2) - ssum) <= 1e-6 * ssum
    assert abs(float(clip_partial) - ex) <= 1e-5 * abs(ex), (float(clip_partial), ex)
    assert int(counter) == 0
    bits = bitmap.cpu().numpy().view(np.uint32)
    for f in range(Fs):
        base = 2 * d.tile_off[f]
        for r in range(rows[f]):
            marked = bool((bits[base + r // 32] >> (r % 32)) & 1) if f in reg else False
            assert marked == (r in touched[f]), (f, r)

    # ---- phase 1: Adagrad of the untouched rows with g = 2 wd W * coef; bitmap and set-chunk gradients back at zero
    d1 = L.WeightDecayDesc.from_buffer_copy(d)
    d1.phase = 1
    _launch(d1)
    torch.cuda.synchronize()
    assert int(bitmap.abs().sum()) == 0
    for o, n in setc:
        assert int((g_d[o:o + n] != 0).sum()) == 0
    for o, n in add:
        assert torch.equal(g_d[o:o + n].cpu(), g_after0[o:o + n])
    for f in range(Fs):
        got_t, got_s = tables[f].cpu().double(), state[f].cpu().double()
        want_t, want_s = t0[f].clone(), s0[f].clone()
        if f in reg:
            un = torch.tensor([r for r in range(rows[f]) if r not in touched[f]])
            gg = 2 * wd * t0[f][un] * coef
            want_s[un] = s0[f][un] + gg * gg
            want_t[un] = t0[f][un] - lr * gg / (want_s[un].sqrt() + eps)
        assert torch.allclose(got_s, want_s, rtol=1e-6, atol=1e-7), f
        assert torch.allclose(got_t, want_t, rtol=1e-6, atol=1e-7), f
        if f not in reg or touched[f]:
            keep = sorted(touched[f]) if f in reg else list(range(rows[f]))
            assert torch.equal(got_t[keep], t0[f][keep]) and torch.equal(got_s[keep], s0[f][keep])


def _fixed_model(tables, dev):
    choice = json.load(open(os.path.join(ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_autoctr_best_1shot.json")))
    torch.manual_seed(4)
    return SuperNet(num_blocks=choice["num_blocks"], ops_config=ops_config_lib[choice["config"]], use_layernorm=False, num_embeddings=tables,
                    sparse_input_size=26, path_sampling_strategy="fixed-path", fixed=True, fixed_choice=choice).to(dev)


@pytest.mark.parametrize("B", [16, 512, 4096])
def test_fused_weight_decay_with_a_binding_clip_equals_the_torch_route(B):
    """clip 0.05, wd 1e-2 (the L2 gradient's norm, ~0.6 over the 26 capped tables, dominates the BCE one): the L2 term's share of the
    norm decides the coefficient (< 1, read back from the engine), at batch sizes that take
    the two-halves dedup (16, 512) and the one-launch dedup + merge (4096); 3 steps against autograd on BCE + get_l2_loss,
    clip_grad_norm_ and torch.optim.Adagrad"""
    dev = torch.device("cuda", 0)
    from nasrec_amd.utils.config import NUM_EMBEDDINGS_CRITEO
    tables = [min(n, 997) for n in NUM_EMBEDDINGS_CRITEO]
    wd, clip, lr = 1e-2, 0.05, 0.05
    g = torch.Generator().manual_seed(9)
    batches = [(torch.log(torch.randint(0, 1000, (B, 13), generator=g).float() + 1).to(dev),
                torch.stack([torch.randint(0, n, (B,), generator=g) for n in tables], 1).to(dev),
                (torch.rand(B, generator=g) < 0.25).float().to(dev)) for _ in range(3)]
    base = _fixed_model(tables, dev)
    with torch.no_grad():
        base(batches[0][0], batches[0][1])
    base.apply(TU.init_weights)
    import copy
    res, coefs = [], []
    for fused in (True, False):
        m = copy.deepcopy(base)
        opt = torch.optim.Adagrad(m.parameters(), lr=lr, eps=1e-2)
        if fused:
            m._ensure_engine(batches[0][0])
            m.engine_bind_optimizer(opt)
        for int_x, cat_x, y in batches:
            if fused:
                m.engine_train_step(int_x, cat_x, y, lr=lr, clip=clip, eps=1e-2, weight_decay=wd)
                coefs.append(float(m._engine.clip_out[0]))
            else:
                opt.zero_grad()
                loss = torch.nn.functional.binary_cross_entropy_with_logits(m(int_x, cat_x).view(-1), y) + TU.get_l2_loss(m, wd, None, gpu=0)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(m.parameters(), clip)
                opt.step()
        if fused:
            m.engine_sync_optimizer_steps(opt)
        torch.cuda.synchronize()
        res.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                    {n: opt.state[p]["sum"].detach().cpu().clone() for n, p in m.named_parameters()}))
    assert all(c < 0.9 for c in coefs), coefs
    (pa, sa), (pb, sb) = res
    for k in pa:
        assert torch.allclose(pa[k], pb[k], rtol=0, atol=2e-5), (k, float((pa[k] - pb[k]).abs().max()))
    for k in sa:
        assert torch.allclose(sa[k], sb[k], rtol=1e-3, atol=1e-9), (k, float((sa[k] - sb[k]).abs().max()))
