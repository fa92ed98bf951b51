"""Chained same-target input gradients without a device: the scheduling pass (schedule.chain_accumulates) on synthetic programs and on
the batch-256 plan of the bench network, and the launcher's geometry of the chained item (csrc/worklist.hip wl_chain_geometry) through
nasrec_worklist_item_geometry.  Descriptors here carry made-up addresses: nothing follows a pointer."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nasrec_amd import _lib as L  # noqa: E402
from nasrec_amd import schedule as S  # noqa: E402

CFG = os.path.join(ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_xlarge_best_1shot.json")
MB = 1 << 24  # spacing of the made-up buffers
NB = 8        # samples
MS = (26, 72, 64)


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(autouse=True)
def _chain_on(monkeypatch):
    monkeypatch.setattr(S, "CHAIN", True)


def dx(w, dy, cs, K=32, acc=1, Ms=MS, N=NB * 16, splitk=1, ldc=None, mask=0):
    """a token-axis input gradient W^T dy over the input segments `cs` (one problem each): weights at buffer w, dy at buffer dy"""
    d = L.GemmDesc()
    d.kind, d.amode, d.bmode, d.cmode, d.zmode, d.nseg, d.dims_in_use, d.splitk = L.OP_GEMM, L.AM_RC, L.AM_TOKR, L.CM_TOKJ, 1, len(cs), -1, splitk
    if splitk > 1:
        d.workspace = 60 * MB
    off = 0
    for q, c in enumerate(cs):
        s = d.seg[q]
        s.A, s.B, s.C = w * MB + 4 * off, dy * MB, c * MB
        s.Baux = (dy + 1) * MB if mask else None
        s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.Mvalid, s.accumulate = Ms[q], N, K, sum(Ms), K * 16, (ldc or Ms[q]) * 16, Ms[q], acc
        off += Ms[q]
    return d


def fill(buf, floats=64 * NB * 16):
    m = L.MemsetDesc()
    m.kind, m.ptr, m.bytes = L.OP_MEMSET, buf * MB, 4 * floats
    return m


def chained(descs):
    return [d for d in descs if getattr(d, "_chain", 0)]


def program(P, Q, between=(), q_late=False):
    """dy of P is written at level 0, so P sits at level 1; Q's dy is written once (ready at level 1) or twice (q_late: ready at level 2)"""
    return [fill(10), fill(20)] + ([fill(20)] if q_late else []) + [P] + list(between) + [Q]


def test_an_eligible_pair_becomes_one_node_with_the_union_of_both_footprints():
    P, Q = dx(1, 10, (30, 31, 32), K=32, acc=0), dx(2, 20, (30, 31, 32), K=39, mask=1)
    before = [bytes(P), bytes(Q)]
    prog = program(P, Q)
    out = S.chain_accumulates(prog)
    assert [bytes(P), bytes(Q)] == before and len(out) == len(prog) - 1  # the plan's descriptors are left alone
    (m,) = chained(out)
    assert m._chain == 3 and m.nseg == 6 and m._chain_of == (P, Q)
    assert [(m.seg[q].M, m.seg[q].K, m.seg[q].accumulate) for q in range(6)] == [(M, 32, 0) for M in MS] + [(M, 39, 1) for M in MS]
    n, np_, nq = S.expand(out)[out.index(m)], S.Node(P), S.Node(Q)
    assert n.part == "chain"
    key = lambda accs: sorted({(a.ptr, a.rows, a.width, a.stride) for a in accs})  # noqa: E731
    assert key(n.reads) == key(np_.reads + nq.reads) and key(n.writes) == key(np_.writes + nq.writes)
    # one level fewer, and the chained node always travels as an item of part NASREC_WL_CHAIN
    assert S.assign_levels(S.expand(out)) == S.assign_levels(S.expand(prog)) - 1
    packed, nl = S.pack(out)
    parts = [(w.item[k].part, nd.part) for w in packed if isinstance(w, L.WorklistDesc) for k, nd in enumerate(w.nodes) if nd.desc is m]
    assert parts == [(L.WL_CHAIN, "chain")] and not any(d is m for d in packed)


def test_a_third_writer_joins_the_chain_while_the_problems_fit():
    P, Q, R = dx(1, 10, (30, 31)), dx(2, 20, (30, 31), K=39), dx(3, 40, (30, 31), K=64)
    out = S.chain_accumulates([fill(10), fill(20), fill(40), P, Q, R])
    (m,) = chained(out)
    assert m._chain == 2 and m.nseg == 6 and m._chain_of == (P, Q, R) and len(out) == 4
    # c h <= NASREC_MAX_SEGS: three problems per member leave room for two members only
    P, Q, R = dx(1, 10, (30, 31, 32)), dx(2, 20, (30, 31, 32), K=39), dx(3, 40, (30, 31, 32), K=64)
    out = S.chain_accumulates([fill(10), fill(20), fill(40), P, Q, R])
    (m,) = chained(out)
    assert m._chain_of == (P, Q) and R in out
    five = tuple(range(30, 35))
    P, Q = dx(1, 10, five, Ms=(16,) * 5), dx(2, 20, five, Ms=(16,) * 5)
    assert chained(S.chain_accumulates(program(P, Q))) == []


def test_q_moves_up_or_p_moves_down_past_what_lies_between():
    one = (26,)
    other = dx(5, 50, (45,), Ms=one)
    P, Q = dx(1, 10, (30,), Ms=one), dx(2, 20, (30,), Ms=one)
    out = S.chain_accumulates(program(P, Q, between=[other]))
    assert len(chained(out)) == 1 and out.index(chained(out)[0]) < out.index(other)  # nothing between feeds Q: it moves up to P
    # Q's operand is written between the two, so Q cannot move; nothing between waits for P (at level 2), which moves down to Q
    feeds_q = fill(20)
    out = S.chain_accumulates([fill(10), fill(10), P, feeds_q, Q])
    assert len(chained(out)) == 1 and out.index(chained(out)[0]) == out.index(feeds_q) + 1 and len(out) == 4
    # ... unless something between also overwrites one of P's operands: neither may pass, the pair stays
    prog = [fill(10), fill(10), P, feeds_q, fill(10), Q]
    assert S.chain_accumulates(prog) is prog


@pytest.mark.parametrize("what", ["reader_between", "q_ready_later", "other_c", "other_m", "other_n", "other_ldc", "q_overwrites", "splitk", "k_above_64",
                                  "other_count", "weight_mask"])
def test_pairs_the_pass_leaves_alone(what):
    P, Q = dx(1, 10, (30, 31, 32)), dx(2, 20, (30, 31, 32), K=39)
    between, late = [], False
    if what == "reader_between":
        r = dx(4, 30, (44,), Ms=(26,), K=26)  # reads P's first output as its dy
        r.seg[0].ldb = 26 * 16
        between = [r]
    elif what == "q_ready_later":
        late = True
    elif what == "other_c":
        Q = dx(2, 20, (30, 31, 33), K=39)
    elif what == "other_m":
        Q = dx(2, 20, (30, 31, 32), K=39, Ms=(26, 72, 48), ldc=72)
        P = dx(1, 10, (30, 31, 32), ldc=72)
    elif what == "other_n":
        Q = dx(2, 20, (30, 31, 32), K=39, N=(NB - 1) * 16)
    elif what == "other_ldc":
        Q = dx(2, 20, (30, 31, 32), K=39, ldc=80)
    elif what == "q_overwrites":
        Q = dx(2, 20, (30, 31, 32), K=39, acc=0)
    elif what == "splitk":
        Q = dx(2, 20, (30, 31, 32), K=39, splitk=2)
    elif what == "k_above_64":
        Q = dx(2, 20, (30, 31, 32), K=65)
    elif what == "other_count":
        Q = dx(2, 20, (30, 31), K=39)
    elif what == "weight_mask":
        Q.seg[1].Aaux = 70 * MB
    prog = program(P, Q, between, late)
    out = S.chain_accumulates(prog)
    assert chained(out) == [] and all(a is b for a, b in zip(out, prog)) and len(out) == len(prog)


def test_the_knob_turns_the_pass_off(monkeypatch):
    prog = program(dx(1, 10, (30, 31, 32)), dx(2, 20, (30, 31, 32), K=39))
    monkeypatch.setattr(S, "CHAIN", False)
    assert S.chain_accumulates(prog) is prog


# ---- the launcher's geometry ---------------------------------------------------------------------------------------------------------
def _blob(d):
    return C.string_at(C.addressof(d), L.GemmDesc.seg.offset + max(0, min(d.nseg, L.MAX_SEGS)) * C.sizeof(L.GemmSeg))


def _query(lib, d, part):
    g = L.WlGeometry()
    b = _blob(d)
    rc = lib.nasrec_worklist_item_geometry(d.kind, part, b, len(b), C.byref(g))
    return rc, g, lib.nasrec_last_error().decode(errors="replace")


def _legal(Ms=MS, Ks=(32, 39), acc0=0, masks=(0, 1)):
    cs = tuple(range(30, 30 + len(Ms)))
    m = dx(1, 10, cs, K=Ks[0], acc=acc0, Ms=Ms, mask=masks[0])
    for k, K in enumerate(Ks[1:]):
        m = S._merged_chain(m, dx(2 + k, 20 + 2 * k, cs, K=K, Ms=Ms, mask=masks[1 + k]))
        assert m is not None
    return m


@pytest.mark.parametrize("Ms,Ks", [(MS, (32, 39)), ((26,), (8, 64)), ((17, 1), (1, 16, 64)), ((64, 64, 64, 64), (64, 64))])
def test_geometry_accepts_legal_chains_with_the_plain_items_units(lib, Ms, Ks):
    m = _legal(Ms, Ks, masks=(0,) * len(Ks))
    rc, g, msg = _query(lib, m, L.WL_CHAIN)
    assert rc == 0, msg
    rp, gp, msg = _query(lib, m._chain_of[0], L.WL_WHOLE)
    assert rp == 0 and gp.body == L.WL_BODY_TOKEN_DX, msg
    assert g.body == L.WL_BODY_TOKEN_DX_CHAIN and g.nblk == gp.nblk and g.geom[0] == gp.geom[0] == sum((M + 15) // 16 for M in Ms)
    assert g.geom[1] == len(Ms) and g.big == 0
    # as an ordinary launch the same bytes are no token-dx item of twice the units, and a plain item is no chain
    assert _query(lib, m._chain_of[0], L.WL_CHAIN)[0] != 0


def _set(field, value, seg=None):
    def f(m):
        setattr(m if seg is None else m.seg[seg], field, value)
    return f


ILLEGAL = {
    "splitk": _set("splitk", 2), "not_zmode": _set("zmode", 0), "binding_a": _set("amode", L.AM_KC), "binding_b": _set("bmode", L.AM_RC),
    "binding_c": _set("cmode", L.CM_PLAIN), "weight_mask": _set("Aaux", 70 * MB, 4), "other_m": _set("M", 25, 3), "other_n": _set("N", 16 * NB - 16, 5),
    "other_ldc": _set("ldc", 27 * 16, 3), "other_c": _set("C", 47 * MB, 4), "second_member_overwrites": _set("accumulate", 0, 4),
    "n_not_whole_samples": lambda m: [setattr(m.seg[q], "N", 16 * NB - 8) for q in range(6)], "k_above_64": _set("K", 65, 5),
    "ones_col": _set("ones_col", 1, 1), "row_predicate": _set("Mvalid", 20, 0), "bias": _set("bias", 71 * MB), "activation": _set("act", L.ACT_RELU),
    "dims_in_use": _set("dims_in_use", 8), "pre_add": _set("pre_add", 72 * MB), "gate": _set("mul_nseg", 1), "save_z": _set("save_z", 73 * MB),
    "save_act": _set("save_act", 74 * MB), "no_second_writer": lambda m: [setattr(m.seg[q], "C", (50 + q) * MB) for q in range(3, 6)],
    "unequal_chains": _set("nseg", 5), "too_many_problems": _set("nseg", L.MAX_SEGS + 1), "no_output": lambda m: [setattr(m.seg[q], "C", None) for q in (0, 3)],
}


@pytest.mark.parametrize("what", list(ILLEGAL))
def test_geometry_refuses_every_illegal_chain_with_an_error(lib, what):
    m = _legal()
    assert _query(lib, m, L.WL_CHAIN)[0] == 0
    ILLEGAL[what](m)
    rc, g, msg = _query(lib, m, L.WL_CHAIN)
    assert rc != 0 and msg.startswith("worklist:"), (what, msg)
    assert S.item_geometry(m.kind, "chain", _blob(m)) is None


def test_the_persistent_form_refuses_a_chained_item(lib):
    m = _legal()
    items = (L.PersistItem * 1)()
    items[0].kind, items[0].part, items[0].off = m.kind, L.WL_CHAIN, 0
    b = _blob(m)
    hb = C.create_string_buffer(b, len(b))
    d = L.PersistDesc()
    d.kind, d.n, d.blob_bytes = L.OP_PERSIST, 1, len(b)
    d.host_items, d.host_blob = C.addressof(items), C.addressof(hb)
    assert lib.nasrec_persist_prepare(C.addressof(d)) != 0 and b"chained" in lib.nasrec_last_error()


def test_a_dead_member_is_legal(lib):
    m = _legal()
    m.seg[4].A = None
    m.seg[0].K = 0
    assert _query(lib, m, L.WL_CHAIN)[0] == 0


# ---- the bench network's plan ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    import show_levels as SL
    return SL.build_cpu_plan(CFG, 256, 13, 26)


def _shapes(d):
    return [(d.seg[q].M, d.seg[q].N, d.seg[q].K) for q in range(d.nseg)]


def test_the_batch_256_backward_loses_a_level_to_two_chained_items(plan, monkeypatch):
    bwd = list(plan.bwd)
    before = [bytes(d) for d in bwd]
    monkeypatch.setattr(S, "CHAIN", False)
    off, nl_off = S.pack(S.chain_accumulates(bwd))
    monkeypatch.setattr(S, "CHAIN", True)
    prog = S.chain_accumulates(bwd)
    on, nl_on = S.pack(prog)
    assert nl_on == nl_off - 1 and len(on) == len(off) - 1
    assert [bytes(d) for d in bwd] == before and all(not hasattr(d, "_chain") for d in bwd)  # (the planner's descriptors are what they were)
    raw = [(26, 4096), (72, 4096), (64, 4096)]
    assert [_shapes(d) for d in chained(prog)] == [[(M, N, 32) for M, N in raw] + [(M, N, 39) for M, N in raw], [(26, 4096, 8), (26, 4096, 64)]]
    items = [(w.item[k].part, n.desc) for w in on if isinstance(w, L.WorklistDesc) for k, n in enumerate(w.nodes) if n.part == "chain"]
    assert [p for p, _ in items] == [L.WL_CHAIN] * 2 and [d for _, d in items] == chained(prog)
    # every operator is still there exactly once
    members = [m for d in chained(prog) for m in d._chain_of]
    assert len(members) == 4 and sorted(id(d) for d in bwd) == sorted([id(d) for d in prog if not getattr(d, "_chain", 0)] + [id(m) for m in members])
    nodes = S.expand_for_worklists(prog)
    S.assign_levels(nodes)
    for i, a in enumerate(nodes):
        for j in range(i):
            if S._depends(a, nodes[j]):
                assert a.level > nodes[j].level


def test_the_planner_emits_what_it_emitted(monkeypatch):
    """the pass lives at scheduling time: the forms harvested from plan.py's output do not depend on it"""
    import op_forms as F

    def forms():
        got = {}
        for label, cfg, choice in F.plans():
            if label == "fixed:" + os.path.basename(CFG):
                fwd, bwd = F.compile_host(cfg, choice, 256, True)
                S.chain_accumulates(fwd + bwd)  # (running the pass over a plan's programs changes none of their descriptors)
                for d in fwd + bwd:
                    if d.kind in F.FORM_FN:
                        got.setdefault(F.form_of(d), 0)
                        got[F.form_of(d)] += 1
        return got
    monkeypatch.setattr(S, "CHAIN", False)
    off = forms()
    monkeypatch.setattr(S, "CHAIN", True)
    assert forms() == off and off
