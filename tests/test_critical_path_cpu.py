"""The critical path of the batch-256 step of ea_criteo_kaggle_xlarge_best_1shot.json (descriptors only, nothing is launched):

  * schedule.order_two_term_accumulates lets the 16-wide Linear that is added onto the one-pass 780-deep product go first,
  * engine._fuse_head folds the last dense Linear and its input gradient into NASREC_OP_FINAL_FUSED,

and the joint forward + backward DAG has 20 dependency levels where it had 23.  Both passes leave alone what they must."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nasrec_amd import _lib as L  # noqa: E402
from nasrec_amd import schedule as S  # noqa: E402
from nasrec_amd.engine import SupernetEngine  # noqa: E402

B = 256
CFG = os.path.join(ROOT, "nasrec_amd", "configs", "criteo", "ea_criteo_kaggle_xlarge_best_1shot.json")


class _List(list):
    pass


@pytest.fixture(scope="module")
def plan():
    """(forward list, backward list with the loss folded into the final-logit backward, that descriptor): what engine.compile hands
    to _fuse_final"""
    import show_levels
    ctx = show_levels.build_cpu_plan(CFG, B, 13, 26)
    fwd, bwd = _List(ctx.fwd), list(ctx.bwd)
    ffwd = next(d for d in fwd if isinstance(d, L.FinalDesc))
    fi = next(i for i, d in enumerate(bwd) if isinstance(d, L.FinalDesc))
    fused = L.FinalDesc.from_buffer_copy(bwd[fi])
    y, loss, dlog = ctx.alloc(B), ctx.alloc(1), ctx.alloc(B)
    fused.logits, fused.y, fused.loss, fused.dlogits_out, fused.grad_scale = ffwd.logits, y.data_ptr(), loss.data_ptr(), dlog.data_ptr(), 1.0 / B
    bwd[fi] = fused
    fwd._keep = (ctx, y, loss, dlog)
    return fwd, bwd, fused


def _levels(descs):
    nodes = S.expand(descs)
    return S.assign_levels(nodes), nodes


def _shape(d):
    s = d.seg[0]
    return (s.M, s.N, s.K)


def test_the_joint_program_has_twenty_levels(plan):
    fwd, bwd, fused = plan
    jf, jb = SupernetEngine._fuse_final(fwd, bwd, fused)
    assert _levels(jf + jb)[0] == 23  # as planned before: every one of levels 1-18 held by a single operator
    f2 = S.order_two_term_accumulates(fwd)
    jf, jb = SupernetEngine._fuse_final(f2, bwd, fused)
    assert _levels(jf + jb)[0] == 22
    hf, hb = SupernetEngine._fuse_head(jf, jb)
    assert _levels(hf + hb)[0] == 20
    assert len(hf) == len(jf) - 1 and len(hb) == len(jb) - 1
    # the two products are gone, the rest is what it was
    gone = [d for d in jf + jb if not any(d is e for e in hf + hb) and isinstance(d, L.GemmDesc)]
    assert sorted(_shape(d) for d in gone) == [(256, 16, 128), (256, 128, 16)]
    head = next(d for d in hf if isinstance(d, L.FinalDesc))
    lin = next(d for d in gone if _shape(d) == (256, 128, 16))
    dx = next(d for d in gone if _shape(d) == (256, 16, 128))
    assert head.kind == L.OP_FINAL_FUSED and (head.head_K, head.head_N) == (16, 128)
    assert (head.head_x, head.head_w, head.head_bias, head.head_pre, head.head_y) == (lin.seg[0].A, lin.seg[0].B, lin.bias, lin.pre_add, lin.seg[0].C)
    assert head.head_pre and head.seg[head.head_seg] == head.head_y and head.ld[head.head_seg] == head.head_ldy == lin.seg[0].ldc
    assert (head.head_dx, head.head_lddx, head.head_dx_accumulate) == (dx.seg[0].C, dx.seg[0].ldc, int(dx.seg[0].accumulate != 0))
    assert dx.seg[0].A == head.dseg[head.head_seg]
    # the worklist kernel has a body for it, and the forward-only joint program without the dx half has 21 levels
    assert S.item_bytes(S.Node(head)) is not None
    no_dx = [d for d in jb if d is not dx]
    only_fwd_half, kept = SupernetEngine._fuse_head(jf, no_dx)
    assert kept == no_dx and not next(d for d in only_fwd_half if isinstance(d, L.FinalDesc)).head_dx


def test_the_one_pass_product_accumulates_onto_the_sixteen_wide_linear(plan):
    fwd, _, _ = plan
    f2 = S.order_two_term_accumulates(fwd)
    assert len(f2) == len(fwd) and f2 is not fwd
    before = {_shape(d): (i, d.beta) for i, d in enumerate(fwd) if isinstance(d, L.GemmDesc) and d.nseg == 1 and _shape(d) in ((256, 768, 780), (256, 768, 16))}
    after = {_shape(d): (i, d.beta) for i, d in enumerate(f2) if isinstance(d, L.GemmDesc) and d.nseg == 1 and _shape(d) in ((256, 768, 780), (256, 768, 16))}
    assert before[(256, 768, 780)][1] == 0 and before[(256, 768, 16)][1] == 1 and before[(256, 768, 780)][0] < before[(256, 768, 16)][0]
    assert after[(256, 768, 780)][1] == 1 and after[(256, 768, 16)][1] == 0 and after[(256, 768, 16)][0] < after[(256, 768, 780)][0]
    big = f2[after[(256, 768, 780)][0]]
    from nasrec_amd import plan as P
    assert P.gemm_route(big)[0] == L.GEMM_ROUTE_KSLICE  # still the one-pass kernel, now with beta = 1
    # everything else is the same object in the same relative order; a second application changes nothing
    assert [d for d in f2 if any(d is e for e in fwd)] == [d for d in fwd if any(d is e for e in f2)]
    assert sum(1 for d in f2 if not any(d is e for e in fwd)) == 2
    assert S.order_two_term_accumulates(f2) is f2
    # the levels: the 16-wide Linear one level in front of the product, where it was one behind
    lv = {_shape(n.desc): n.level for n in _levels(f2)[1] if isinstance(n.desc, L.GemmDesc) and n.desc.nseg == 1}
    assert lv[(256, 768, 16)] < lv[(256, 768, 780)]


# ---- synthetic programs: addresses are plain numbers, nothing is dereferenced ----------------------------------------------------------
def _gemm(A, Bw, Cp, M, N, K, beta=0, **kw):
    g = L.GemmDesc()
    g.kind, g.amode, g.bmode, g.cmode, g.nseg, g.dims_in_use, g.beta = L.OP_GEMM, L.AM_KC, L.AM_KC, L.CM_PLAIN, 1, -1, beta
    s = g.seg[0]
    s.A, s.B, s.C, s.M, s.N, s.K, s.lda, s.ldb, s.ldc = A, Bw, Cp, M, N, K, K, K, N
    for k, v in kw.items():
        setattr(g, k, v)
    return g


MB = 1 << 20
X0, X1, X2, X3, CC, WW = (0x10000000 + i * MB for i in range(6))


def _chain(n_terms, **kw):
    """x1 = f(x0) (level 0), x2 = f(x1) (level 1), x3 = f(x2) (level 2); C = x3 W (level 3) + x1 W' (+ x2 W'' with three terms)"""
    prog = [_gemm(X0, WW, X1, 64, 16, 16), _gemm(X1, WW + 4096, X2, 64, 16, 16), _gemm(X2, WW + 8192, X3, 64, 16, 16),
            _gemm(X3, WW + 12288, CC, 64, 32, 16, beta=0), _gemm(X1, WW + 16384, CC, 64, 32, 16, beta=1, **kw)]
    if n_terms == 3:
        prog.append(_gemm(X2, WW + 20480, CC, 64, 32, 16, beta=1))
    return prog


def test_two_terms_swap_and_three_terms_keep_their_order():
    two = _chain(2)
    out = S.order_two_term_accumulates(two)
    assert [d.seg[0].A for d in out] == [X0, X1, X2, X1, X3] and [d.beta for d in out[3:]] == [0, 1]
    assert _levels(two)[0] == 5 and _levels(out)[0] == 4
    assert all(a is b for a, b in zip(out[:3], two[:3])) and two[3].beta == 0 and two[4].beta == 1  # (the input is not edited)
    three = _chain(3)
    assert S.order_two_term_accumulates(three) is three


@pytest.mark.parametrize("kw", [dict(act=L.ACT_RELU), dict(dims_in_use=8), dict(save_z=0x30000000), dict(save_act=0x30000000),
                                dict(pre_add=0x30000000), dict(splitk=2, workspace=0x38000000)], ids=lambda kw: next(iter(kw)))
def test_a_pair_with_more_than_a_plain_epilogue_keeps_its_order(kw):
    prog = _chain(2, **kw)
    assert S.order_two_term_accumulates(prog) is prog


def test_a_reader_between_the_two_terms_keeps_their_order():
    prog = _chain(2)
    prog.insert(4, _gemm(CC, WW + 24576, 0x30000000, 64, 16, 32))
    assert S.order_two_term_accumulates(prog) is prog


def test_a_pair_whose_second_term_is_ready_no_earlier_keeps_its_order():
    prog = [_gemm(X0, WW, X1, 64, 16, 16), _gemm(X1, WW + 12288, CC, 64, 32, 16, beta=0), _gemm(X1, WW + 16384, CC, 64, 32, 16, beta=1)]
    assert S.order_two_term_accumulates(prog) is prog


# ---- what the head fold refuses ----------------------------------------------------------------------------------------------------------
def _joint(plan):
    fwd, bwd, fused = plan
    return SupernetEngine._fuse_final(S.order_two_term_accumulates(fwd), bwd, fused)


def _swap(descs, old, new):
    return [new if d is old else d for d in descs]


def _head_linear(jf):
    return next(d for d in jf if isinstance(d, L.GemmDesc) and d.nseg == 1 and _shape(d) == (256, 128, 16))


def test_token_strided_final_segments_keep_the_unfused_descriptors(plan):
    """last_n_blocks_out = 2: the sparse outputs of the last blocks meet the final weights token by token (tok_stride != 0)"""
    jf, jb = _joint(plan)
    both = next(d for d in jf if isinstance(d, L.FinalDesc))
    strided = L.FinalDesc.from_buffer_copy(both)
    strided.tok_stride[1] = 32
    jf2 = _swap(jf, both, strided)
    hf, hb = SupernetEngine._fuse_head(jf2, jb)
    assert hf is jf2 and hb is jb


@pytest.mark.parametrize("edit", ["act", "mask", "save_act", "mul", "two_k_segments", "K33", "beta"])
def test_a_head_linear_that_is_more_than_a_plain_product_keeps_the_unfused_descriptors(plan, edit):
    jf, jb = _joint(plan)
    lin = _head_linear(jf)
    g = L.GemmDesc.from_buffer_copy(lin)
    if edit == "act":
        g.act = L.ACT_RELU
    elif edit == "mask":
        g.dims_in_use = 64
    elif edit == "save_act":
        g.save_act = 0x30000000
    elif edit == "mul":
        g.mul_nseg, g.mul_ptr[0], g.mul_width[0], g.mul_ld[0] = 1, 0x30000000, 128, 128
    elif edit == "two_k_segments":
        g.nseg = 2
        C.memmove(C.addressof(g.seg[1]), C.addressof(g.seg[0]), C.sizeof(L.GemmSeg))
    elif edit == "K33":
        g.seg[0].K = g.seg[0].lda = g.seg[0].ldb = 33
    else:
        g.beta = 1
    jf2 = _swap(jf, lin, g)
    hf, hb = SupernetEngine._fuse_head(jf2, jb)
    assert hf is jf2 and hb is jb


def test_another_forward_reader_of_y_keeps_the_unfused_descriptors(plan):
    jf, jb = _joint(plan)
    lin = _head_linear(jf)
    reader = _gemm(lin.seg[0].C, WW, 0x30000000, 256, 16, 128)
    reader.seg[0].lda = lin.seg[0].ldc
    jf2 = list(jf) + [reader]
    hf, hb = SupernetEngine._fuse_head(jf2, jb)
    assert hf is jf2 and hb is jb


def test_an_input_gradient_with_a_mask_leaves_the_forward_half_only(plan):
    jf, jb = _joint(plan)
    dx = next(d for d in jb if isinstance(d, L.GemmDesc) and d.zmode and d.nseg == 1 and _shape(d) == (256, 16, 128))
    m = L.GemmDesc.from_buffer_copy(dx)
    m.seg[0].Aaux = 0x30000000
    jb2 = _swap(jb, dx, m)
    hf, hb = SupernetEngine._fuse_head(jf, jb2)
    head = next(d for d in hf if isinstance(d, L.FinalDesc))
    assert head.head_x and not head.head_dx and hb == jb2 and len(hf) == len(jf) - 1
    assert _levels(hf + hb)[0] == 21


# ---- footprints ---------------------------------------------------------------------------------------------------------------------------
def test_desc_io_of_a_headed_operator_lists_the_linear_and_its_input_gradient(plan):
    jf, jb = _joint(plan)
    hf, _ = SupernetEngine._fuse_head(jf, jb)
    head = next(d for d in hf if isinstance(d, L.FinalDesc))
    plain = next(d for d in jf if isinstance(d, L.FinalDesc))
    R, W = S.desc_io(head)
    R0, W0 = S.desc_io(plain)
    key = lambda a: (a.ptr, a.rows, a.width, a.stride)
    new_r = {key(a) for a in R} - {key(a) for a in R0}
    new_w = {key(a) for a in W} - {key(a) for a in W0}
    acc = lambda p, rows, w, ld: key(S.Acc(p, rows, w, ld))
    want_r = {acc(head.head_x, B, 16, head.head_ldx), acc(head.head_w, 128, 16, head.head_ldw), acc(head.head_bias, 1, 128, 128),
              acc(head.head_pre, B, 128, head.head_ldy)}
    dxk = acc(head.head_dx, B, 16, head.head_lddx)
    if head.head_dx_accumulate:
        want_r.add(dxk)
    assert new_r == want_r
    assert new_w == {acc(head.head_y, B, 128, head.head_ldy), dxk}
    # y is written here, no longer read from memory
    assert acc(head.head_y, B, 128, head.head_ldy) in {key(a) for a in R0} and acc(head.head_y, B, 128, head.head_ldy) not in {key(a) for a in R}


def test_the_binding_matches_the_library():
    lib = L.load()  # (the layout check of load() covers nasrec_final_desc_t: 80 bytes of head fields)
    sizes = (C.c_int32 * 64)()
    n = lib.nasrec_desc_sizes(sizes, 64)
    assert C.sizeof(L.FinalDesc) in list(sizes[:n]) and C.sizeof(L.FinalDesc) == 464
    assert L.FinalDesc.head_x.offset == 384 and L.FinalDesc.head_seg.offset == 460
