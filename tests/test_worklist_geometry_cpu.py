"""The launcher's own geometry (csrc/worklist.hip wl_item_geometry / wl_gemm_geometry) on every case of tests/wl_cases.py, without a
device, by its two host-only routes: nasrec_worklist_item_geometry, the query schedule.item_bytes / gemm_capable decide by (they state
no condition of the kernels themselves), and nasrec_persist_prepare with items == NULL, a dry pass that writes each item's geometry
back into host_items.  Neither dereferences a descriptor's pointers.  Checked: the scheduler accepts a descriptor exactly when the
launcher does, the two routes give the same geometry, it names the body the case was written for (the table in the docstring of
tests/test_worklist_items_gpu.py lists the same pairs) and the query's `body` says the same as the test's own decoding of geom, every
body of the two kernels has a case, and every route refuses what has no body."""
import ctypes as C

import pytest
import torch

import wl_cases as W
from nasrec_amd import _lib as L
from nasrec_amd import plan as P
from nasrec_amd import schedule as S

PART_NAME = {L.WL_WHOLE: "whole", L.WL_MAIN: "main", L.WL_EPI: "epi"}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def raw_bytes(d):
    """what an item of this descriptor would carry, whether or not schedule.item_bytes accepts it"""
    if isinstance(d, L.GemmDesc):
        return C.string_at(C.addressof(d), L.GemmDesc.seg.offset + max(0, min(d.nseg, L.MAX_SEGS)) * C.sizeof(L.GemmSeg))
    if isinstance(d, L.ReduceRowsDesc):
        r = L.WlReduce()
        r.kind, r.R, r.C, r.ld, r.in_, r.ndst = d.kind, d.R, d.C, d.ld, d.in_, d.ndst
        for q in range(min(d.ndst, L.WL_REDUCE_DST)):
            r.dst[q], r.dst_off[q], r.dst_len[q] = d.dst[q], d.dst_off[q], d.dst_len[q]
        return C.string_at(C.addressof(r), C.sizeof(r))
    return C.string_at(C.addressof(d), C.sizeof(d))


def dry(lib, kind, part, blob, blob_bytes=None):
    """-> (return code, item with first / nblk / geom filled in, message) of the launcher's geometry pass on a one-item launch"""
    items = (L.PersistItem * 1)()
    items[0].kind, items[0].part, items[0].off = kind, part, 0
    hb = C.create_string_buffer(blob, max(len(blob), 16))
    d = L.PersistDesc()
    d.kind, d.n, d.blob_bytes = L.OP_PERSIST, 1, len(blob) if blob_bytes is None else blob_bytes
    d.host_items, d.host_blob = C.addressof(items), C.addressof(hb)
    rc = lib.nasrec_persist_prepare(C.addressof(d))
    return rc, items[0], lib.nasrec_last_error().decode(errors="replace")


def query(lib, kind, part, blob, nbytes=None):
    """-> (return code, L.WlGeometry, message) of nasrec_worklist_item_geometry: the same rule asked directly"""
    g = L.WlGeometry()
    rc = lib.nasrec_worklist_item_geometry(kind, part, blob, len(blob) if nbytes is None else nbytes, C.byref(g))
    return rc, g, lib.nasrec_last_error().decode(errors="replace")


@pytest.fixture(scope="module")
def built():
    return {c.name: c.build("cpu") for c in W.CASES}


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_python_accepts_the_case_exactly_when_the_launcher_does_and_the_geometry_names_its_body(lib, built, case):
    b = built[case.name]
    bodies = []
    for part in b.parts:
        got = S.item_bytes(S.Node(b.desc, PART_NAME[part]))
        rc, it, msg = dry(lib, b.desc.kind, part, raw_bytes(b.desc))
        assert (got is not None) == (rc == 0), (case.name, part, rc, msg)
        assert rc == 0, msg
        assert got == raw_bytes(b.desc)
        assert it.nblk >= 1
        rq, g, msg = query(lib, b.desc.kind, part, raw_bytes(b.desc))
        assert rq == 0, msg
        assert (g.nblk, list(g.geom)) == (it.nblk, list(it.geom)), (case.name, part)
        assert W.BODY_ENUM_NAME[g.body] == W.body_enum_name(b.desc.kind, part, it.geom), (case.name, part, g.body)
        assert g.big == (1 if b.desc.kind == L.OP_MHA_BWD else 0)
        bodies.append(W.body_of(b.desc.kind, part, it.geom))
    assert bodies[-1] == case.body, (case.name, bodies)
    if case.gemm:
        assert P.gemm_route(b.desc)[0] == L.GEMM_ROUTE_GENERAL  # (the items promise the bits of the general template only)
        if len(b.parts) == 2:
            assert bodies[0].startswith("T"), bodies  # (a main pass runs on a tile body)


def test_every_body_of_the_two_kernels_has_a_case():
    have = {c.body for c in W.CASES}
    assert have == set(W.ALL_BODIES), (sorted(set(W.ALL_BODIES) - have), sorted(have - set(W.ALL_BODIES)))


def test_the_table_in_the_gpu_modules_docstring_is_the_case_table():
    import test_worklist_items_gpu as G
    rows = {}
    for line in G.__doc__.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] == "->":
            rows[parts[0]] = parts[2]
    assert rows == {c.name: c.body for c in W.CASES}


def _gemm(am, bm, cm, segs, zmode, splitk=1, ws=True):
    d = L.GemmDesc()
    d.kind, d.amode, d.bmode, d.cmode, d.nseg, d.zmode, d.dims_in_use, d.splitk = L.OP_GEMM, am, bm, cm, len(segs), zmode, -1, splitk
    if ws:
        d.workspace = 0x1000
    for q, sd in enumerate(segs):
        s = d.seg[q]
        s.A, s.B, s.C = 0x1000, 0x2000, 0x3000
        s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.Mvalid = 48, 40, 64, 64, 64, 64, 48
        for k, v in sd.items():
            setattr(s, k, v)
    d._wl_force = True  # (routing aside: what is asked is whether the worklist kernel has a body)
    return d


def _refusals():
    out = []

    def tri(k1):
        d = L.DotTriDesc()
        d.kind, d.B, d.k1, d.ld_out, d.T, d.out = L.OP_DOT_TRI_FWD, 4, k1, k1 * (k1 - 1) // 2, 0x1000, 0x2000
        return d
    out += [("dot_tri_k47", tri(47), "whole"), ("dot_tri_k1", tri(1), "whole")]

    def mha(kind, N, saved):
        d = L.MhaDesc()
        d.kind, d.B, d.N, d.ldx, d.ldo, d.dims_in_use = kind, 4, N, N * 16, N * 16, -1
        d.x, d.out, d.dout, d.dx, d.dparams_partial, d.saved = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, (0x6000 if saved else None)
        for q in range(12):
            d.params[q] = 0x10000 * (q + 1)
        return d
    out += [("mha_n65", mha(L.OP_MHA_FWD, 65, True), "whole"), ("mha_bwd_without_saved", mha(L.OP_MHA_BWD, 16, False), "whole")]
    r = L.ReduceRowsDesc()
    r.kind, r.R, r.C, r.ld, r.in_, r.ndst = L.OP_REDUCE_ROWS, 8, 64, 64, 0x1000, 17
    for q in range(17):
        r.dst[q], r.dst_off[q], r.dst_len[q] = 0x2000 + 64 * q, 3 * q, 3
    out.append(("reduce_rows_17_destinations", r, "whole"))

    def dedup(B, cap):
        d = L.DedupIdsDesc()
        d.kind, d.B, d.Fs, d.cap = L.OP_DEDUP_IDS, B, 5, cap
        d.idx, d.leader, d.order, d.lists, d.counts = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
        return d
    out += [("dedup_b257", dedup(257, 256), "whole"), ("dedup_cap512", dedup(200, 512), "whole")]
    out += [("dedup_b0", dedup(0, 256), "whole"), ("dedup_33_fields", dedup(200, 256), "whole")]
    out[-1][1].Fs = L.MAX_TABLES + 1

    def final(kind):
        f = L.FinalDesc()
        f.kind, f.B, f.nseg, f.grad_scale = kind, 8, 1, 0.125
        f.w, f.bias, f.logits, f.y, f.loss, f.dlogits_out, f.dw, f.dbias = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000
        f.seg[0], f.dseg[0], f.width[0], f.ld[0] = 0x9000, 0xa000, 32, 32
        return f
    out += [("final_fused_batch_slices", final(L.OP_FINAL_FUSED), "whole"), ("final_fused_gradient_without_input", final(L.OP_FINAL_FUSED), "whole"),
            ("final_bwd_fused_loss_without_logits", final(L.OP_FINAL_BWD), "whole")]
    out[-3][1].nsplit = 4
    out[-2][1].seg[0] = None
    out[-1][1].logits = None
    out.append(("gemm_rc_kc", _gemm(L.AM_RC, L.AM_KC, L.CM_PLAIN, [{}], 0), "whole"))
    out.append(("gemm_balanced", _gemm(L.AM_KC, L.AM_KC, L.CM_PLAIN, [{}], 0, splitk=L.SPLITK_BALANCED), "whole"))
    out.append(("gemm_splitk3_as_whole", _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}], 1, splitk=3), "whole"))
    out.append(("gemm_splitk1_as_main", _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}], 1, splitk=1), "main"))
    out.append(("gemm_splitk1_as_epi", _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}], 1, splitk=1), "epi"))
    out.append(("gemm_splitk3_without_workspace", _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}], 1, splitk=3, ws=False), "main"))
    out.append(("gemm_segments_disagree_on_mvalid", _gemm(L.AM_KC, L.AM_KC, L.CM_PLAIN, [{}, dict(Mvalid=40)], 0), "whole"))
    out.append(("gemm_segments_disagree_on_mask", _gemm(L.AM_KC, L.AM_RC, L.CM_PLAIN, [{}, dict(Aaux=0x7000)], 0), "whole"))
    out.append(("gemm_segments_disagree_on_ones_col", _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}, dict(ones_col=1)], 0), "whole"))
    return out


_PART = {"whole": L.WL_WHOLE, "main": L.WL_MAIN, "epi": L.WL_EPI}


@pytest.mark.parametrize("name,d,part", _refusals(), ids=[r[0] for r in _refusals()])
def test_both_sides_refuse_what_has_no_body(lib, name, d, part):
    """host-side refusals before any launch: the launcher returns non-zero with a message by either route, the scheduler returns None"""
    assert S.item_bytes(S.Node(d, part)) is None
    rc, _, msg = dry(lib, d.kind, _PART[part], raw_bytes(d))
    assert rc != 0 and msg, (name, rc, msg)
    rq, _, msg_q = query(lib, d.kind, _PART[part], raw_bytes(d))
    assert rq == rc and msg_q == msg, (name, rq, msg_q)


def test_the_valid_forms_of_the_refused_descriptors_are_accepted(lib):
    """... so that each refusal above is the one its name says"""
    f = L.FinalDesc()
    f.B, f.nseg, f.grad_scale = 8, 1, 0.125
    f.w, f.bias, f.logits, f.y, f.loss, f.dlogits_out, f.dw, f.dbias = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000
    f.seg[0], f.dseg[0], f.width[0], f.ld[0] = 0x9000, 0xa000, 32, 32
    dd = L.DedupIdsDesc()
    dd.kind, dd.B, dd.Fs, dd.cap = L.OP_DEDUP_IDS, 200, 5, 256
    dd.idx, dd.leader, dd.order, dd.lists, dd.counts = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    for kind, d, part in [(L.OP_FINAL_FUSED, f, "whole"), (L.OP_FINAL_BWD, f, "whole"), (L.OP_DEDUP_IDS, dd, "whole"),
                          (L.OP_GEMM, _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}], 1, splitk=3), "main"),
                          (L.OP_GEMM, _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}], 1, splitk=3), "epi"),
                          (L.OP_GEMM, _gemm(L.AM_KC, L.AM_KC, L.CM_PLAIN, [{}, {}], 0), "whole")]:
        d.kind = kind
        assert S.item_bytes(S.Node(d, part)) == raw_bytes(d)
        rc, it, msg = dry(lib, kind, _PART[part], raw_bytes(d))
        assert rc == 0 and it.nblk >= 1, msg
        rq, g, msg = query(lib, kind, _PART[part], raw_bytes(d))
        assert rq == 0 and (g.nblk, list(g.geom)) == (it.nblk, list(it.geom)), msg


def test_a_descriptor_that_runs_past_the_blob_is_refused(lib):
    """item_bytes has no blob to run past (the packers size their blobs by the bytes it returns): the launcher's side of the refusal,
    for a GEMM descriptor cut inside its segments and for a plain descriptor cut short — and the intact ones pass"""
    g = _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}, {}, {}], 1)
    whole = raw_bytes(g)
    assert S.item_bytes(S.Node(g)) == whole and len(whole) == L.GemmDesc.seg.offset + 3 * C.sizeof(L.GemmSeg)
    assert dry(lib, g.kind, L.WL_WHOLE, whole)[0] == 0
    rc, _, msg = dry(lib, g.kind, L.WL_WHOLE, whole, blob_bytes=len(whole) - C.sizeof(L.GemmSeg))
    assert rc != 0 and "blob" in msg
    f = L.FmDesc()
    f.kind, f.B, f.N, f.ldx, f.ld_ix, f.x, f.ix = L.OP_FM_FWD, 4, 8, 128, 16, 0x1000, 0x2000
    assert dry(lib, f.kind, L.WL_WHOLE, raw_bytes(f))[0] == 0
    rc, _, msg = dry(lib, f.kind, L.WL_WHOLE, raw_bytes(f), blob_bytes=C.sizeof(L.FmDesc) - 16)
    assert rc != 0 and "blob" in msg
    # ... the query is told the same lengths
    assert query(lib, g.kind, L.WL_WHOLE, whole)[0] == 0 and query(lib, f.kind, L.WL_WHOLE, raw_bytes(f))[0] == 0
    for kind, blob, n in [(g.kind, whole, len(whole) - C.sizeof(L.GemmSeg)), (g.kind, whole, 16), (f.kind, raw_bytes(f), C.sizeof(L.FmDesc) - 16)]:
        rc, _, msg = query(lib, kind, L.WL_WHOLE, blob, nbytes=n)
        assert rc != 0 and "blob" in msg
    # ... and the same refusal from the level launch's own finalize (nothing is launched: the geometry fails first)
    w = L.WorklistDesc()
    w.kind, w.n = L.OP_WORKLIST, 1
    w.item[0].kind, w.item[0].part, w.item[0].off = g.kind, L.WL_WHOLE, L.WL_BLOB_BYTES - 16 * ((len(whole) - 1) // 16)
    buf = torch.zeros(C.sizeof(L.WorklistDesc), dtype=torch.uint8)
    dv = L.WorklistDevDesc()
    g8 = _gemm(L.AM_RC, L.AM_RC, L.CM_PLAIN, [{}] * 8, 1)
    C.memmove(C.addressof(w) + L.WorklistDesc.blob.offset + w.item[0].off, raw_bytes(g8), L.WL_BLOB_BYTES - w.item[0].off)
    assert lib.nasrec_worklist_prepare(C.addressof(w), buf.data_ptr(), C.addressof(dv)) != 0
    assert "blob" in lib.nasrec_last_error().decode()


def test_the_dot_product_limit_is_what_the_shared_lds_buffer_holds(lib):
    """k1 = 46 is the largest DotProduct core whose four per-wavefront tiles and gradient rows fit WL_LDS_FLOATS, and it is where the
    launcher draws the line"""
    def floats(k1):
        return 4 * (k1 * W.TRI_LD + ((k1 * (k1 - 1) // 2 + 3) & ~3))
    assert floats(46) <= W.WL_LDS_FLOATS < floats(47)
    for kind in (L.OP_DOT_TRI_FWD, L.OP_DOT_TRI_BWD):
        d = L.DotTriDesc()
        d.kind, d.B, d.T, d.out, d.dout, d.dT = kind, 4, 0x1000, 0x2000, 0x3000, 0x4000
        for k1, accepted in ((46, True), (47, False)):
            d.k1, d.ld_out = k1, k1 * (k1 - 1) // 2
            rc, g, msg = query(lib, kind, L.WL_WHOLE, raw_bytes(d))
            assert (rc == 0) == accepted and (accepted or "LDS" in msg), (kind, k1, rc, msg)
            assert (S.item_bytes(S.Node(d)) is not None) == accepted


def _layernorm_and_act_bwd():
    ln = L.LayerNormDesc()
    ln.kind, ln.mode, ln.R, ln.D, ln.ldx, ln.ldy, ln.dims_in_use, ln.eps = L.OP_LAYERNORM_FWD, L.AM_KC, 8, 32, 32, 32, -1, 1e-5
    ln.x, ln.w, ln.b, ln.y, ln.stats = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    ab = L.ActBwdDesc()
    ab.kind, ab.mode, ab.R, ab.D, ab.ld_dy, ab.ld_z, ab.ld_dz, ab.act, ab.dims_in_use = L.OP_ACT_BWD, L.AM_KC, 8, 32, 32, 32, 32, L.ACT_RELU, -1
    ab.dy, ab.z, ab.dz = 0x1000, 0x2000, 0x3000
    return [ln, ab]


def test_the_query_refuses_a_kind_without_a_body_with_a_message_and_sets_no_error_on_acceptance(lib):
    f = L.FmDesc()
    f.kind, f.B, f.N, f.ldx, f.ld_ix, f.x, f.ix = L.OP_FM_FWD, 4, 8, 128, 16, 0x1000, 0x2000
    for d in _layernorm_and_act_bwd():
        rc, _, msg = query(lib, d.kind, L.WL_WHOLE, raw_bytes(d))
        assert rc != 0 and "kind %d" % d.kind in msg and "no body" in msg, (rc, msg)
        assert S.item_bytes(S.Node(d)) is None
        # an accepted item leaves the message of the refusal before it in place: acceptance writes no error
        rc, g, after = query(lib, f.kind, L.WL_WHOLE, raw_bytes(f))
        assert rc == 0 and g.nblk == 1 and g.body == L.WL_BODY_KIND and after == msg


def test_a_node_derives_its_footprints_when_asked_and_not_before(monkeypatch):
    """plan._flush_ln_reduce hangs the reductions' Nodes on the worklist for reports: they answer reads / writes = desc_io of the
    reduction, and nothing calls desc_io on the per-step path that only builds the launch"""
    calls = []
    real = S.desc_io
    monkeypatch.setattr(S, "desc_io", lambda d, part="whole": (calls.append(d), real(d, part))[1])
    jobs = []
    for k in range(3):
        r = L.ReduceRowsDesc()
        r.kind, r.R, r.C, r.ld, r.in_, r.ndst = L.OP_REDUCE_ROWS, 8, 64, 64, 0x10000 * (k + 1), 2
        for q in range(2):
            r.dst[q], r.dst_off[q], r.dst_len[q] = 0x100000 * (k + 1) + 0x1000 * q, 32 * q, 32
        jobs.append(r)

    class Ctx:
        ln_reduce, out = list(jobs), []
        emit = out.append
    P._flush_ln_reduce(Ctx)
    (w,) = Ctx.out
    assert isinstance(w, L.WorklistDesc) and w.n == 3 and [n.desc for n in w.nodes] == jobs and all(type(n) is S.Node for n in w.nodes)
    assert calls == []
    for n, r in zip(w.nodes, jobs):
        want_r, want_w = real(r)
        for got, want in ((n.reads, want_r), (n.writes, want_w)):
            assert [(a.ptr, a.rows, a.width, a.stride) for a in got] == [(a.ptr, a.rows, a.width, a.stride) for a in want] and want
    assert calls == jobs  # (once per node: asked again, the node answers from what it kept)
    assert all(n.reads is n.reads for n in w.nodes) and calls == jobs
