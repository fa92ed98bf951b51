"""What the plan compiler emits, held against what the kernel tests set.

form_of(desc) names the properties of an operator descriptor that select code or addressing in its kernel (the bodies of
csrc/attention_tok.h, csrc/interact_bodies.h, csrc/interact.hip, csrc/norm_loss_opt.hip, csrc/final_bodies.h): a bucket boundary sits
where the body branches, a stride is "tight" when it equals the width of the data and "wide" otherwise, a pointer counts as set or NULL.
harvest() compiles launch plans on the host (made-up addresses stand in for the device's buffers: the compiler only takes addresses,
nothing is launched) — the fixed sub-networks of nasrec_amd/configs, the full-path supernets of both search spaces, a SiLU supernet and sampled
sub-paths — and returns one example descriptor per form.  tests/test_op_forms_cpu.py asks that every harvested form is the form of
a kernel case (tests/wl_cases.py, tests/test_op_forms_gpu.py), so that a planner change that starts emitting a form no kernel test
sets is noticed.  NASREC_OP_GEMM has a form too (_gemm: kernel family, tile configuration or launcher branch, binding, segments,
split-K class, the epilogue's predicates; 324 forms in the harvest); tests/test_gemm_forms_cpu.py holds the table of
tests/gemm_cases.py against those.

Plain Python: nothing here touches a GPU."""
import glob
import json
import os

import numpy as np
import torch

from nasrec_amd import _lib as L
from nasrec_amd import plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_NAME = {getattr(L, k): k[3:].lower() for k in dir(L) if k.startswith("OP_")}
E = 16


def _w(ld, tight):
    return "tight" if ld == tight else "wide"


def _mha(d):
    N = d.N
    bwd = d.kind == L.OP_MHA_BWD
    nb = (N + 15) >> 4
    if d.dims_in_use < 0 or d.dims_in_use >= N:  # (a mask of N tokens or more masks nothing: qn = N, no lane is behind it)
        dims, masked_block = "none", False
    elif d.dims_in_use == 0:
        dims, masked_block = "zero", True
    else:  # a block of 16 tokens that is masked as a whole takes the key-only path of both bodies
        dims, masked_block = "mid", d.dims_in_use <= 16 * (nb - 1)
    return (KIND_NAME[d.kind], "blocks%d" % nb, "full_block" if N % 16 == 0 else "ragged_block", "ldx_" + _w(d.ldx, N * E), "ldo_" + _w(d.ldo, N * E),
            "dims_" + dims, "masked_block" if masked_block else "no_masked_block", "saved" if d.saved else "unsaved",
            "shared_partials" if (bwd and d.partial_ld > 0) else "own_partials")


def _fm(d):
    fwd = d.kind == L.OP_FM_FWD
    nbucket = "n<=4" if d.N <= 4 else ("n<=32" if d.N <= 32 else "n>32")  # (four token rows per load instruction, eight loads per trip)
    return (KIND_NAME[d.kind], "add" if (fwd and d.add) else "no_add", "accumulate" if d.accumulate else "overwrite", "ldx_" + _w(d.ldx, d.N * E),
            "ld_ix_" + _w(d.ld_ix, E), nbucket)


def _dot_tri(d):
    k1 = d.k1
    return (KIND_NAME[d.kind], "blocks%d" % ((k1 + 15) >> 4), "full_block" if k1 % 16 == 0 else "ragged_block", "ld_out_" + _w(d.ld_out, k1 * (k1 - 1) // 2))


def _covered(n, ranges):
    hit = np.zeros(max(n, 0), dtype=bool)
    for off, w in ranges:
        hit[max(off, 0):max(off + w, 0)] = True
    return bool(hit.all())


def _gate(d):
    segs = []
    for q in range(d.nseg):
        dr = bool(d.dr_ptr[q])
        segs.append(("dr" if dr else "no_dr", "acc" if (dr and d.dr_accumulate[q]) else "set", "r" if d.r_ptr[q] else "no_r"))
    # (an element meets the ONE segment that holds its column: which kinds of segment occur matters, not their order)
    gap = not _covered(d.D, [(d.r_off[q], d.r_width[q]) for q in range(d.nseg)])
    return (KIND_NAME[d.kind], "nseg%d" % d.nseg, tuple(sorted(set(segs))), "ld_dout_" + _w(d.ld_dout, d.D), "ld_g_" + _w(d.ld_g, d.D),
            "ld_dz_" + _w(d.ld_dz, d.D), "gap" if gap else "no_gap")


def _copy(d):
    segs = []
    for q in range(d.nseg):
        segs.append(("seg" if d.seg[q] else "null", "acc" if (d.reverse and d.seg[q] and d.seg_accumulate[q]) else "set"))
    W = max([d.off[q] + d.width[q] for q in range(d.nseg)] + [0])
    gap = not _covered(W, [(d.off[q], d.width[q]) for q in range(d.nseg)])
    return (KIND_NAME[d.kind], "reverse" if d.reverse else "forward", "accumulate" if (d.accumulate and not d.reverse) else "overwrite",
            tuple(sorted(set(segs))), "gap" if gap else "no_gap")


def reduce_tiers(R):
    """which of the three loops of reduce_rows_block some lane runs: (256-row trips, 64-row trips, single rows)"""
    t256 = t64 = t1 = False
    for rq in range(16):
        r = rq
        while r + 240 < R:
            r, t256 = r + 256, True
        while r + 48 < R:
            r, t64 = r + 64, True
        if r < R:
            t1 = True
    return t256, t64, t1


def _reduce(d):
    R = d.R
    tier = "r<16" if R < 16 else ("r16-63" if R < 64 else ("r64-255" if R < 256 else "r>=256"))
    ndst = "ndst1" if d.ndst == 1 else ("ndst2-16" if d.ndst <= L.WL_REDUCE_DST else "ndst17-48")  # (16: what the compact item form holds)
    null = any(not d.dst[q] for q in range(d.ndst))
    gap = not _covered(d.C, [(d.dst_off[q], d.dst_len[q]) for q in range(d.ndst)])
    return (KIND_NAME[d.kind], tier, "remainder" if (R >= 256 and R % 256) else "no_remainder", ndst, "ld_" + _w(d.ld, d.C),
            "null_dst" if null else "no_null_dst", "gap" if gap else "no_gap")


def _act_bwd(d):
    tight = d.D if d.mode == L.AM_KC else d.D * E
    return (KIND_NAME[d.kind], {L.AM_KC: "kc", L.AM_TOKR: "tokr"}[d.mode], {L.ACT_NONE: "none", L.ACT_RELU: "relu", L.ACT_SILU: "silu", L.ACT_SIGMOID: "sigmoid"}[d.act],
            "dims" if d.dims_in_use >= 0 else "no_dims", "ld_dy_" + _w(d.ld_dy, tight), "ld_z_" + _w(d.ld_z, tight), "ld_dz_" + _w(d.ld_dz, tight))


def _rowsum(d):
    tight = d.R if d.mode == L.AM_RC else d.R * E
    return (KIND_NAME[d.kind], {L.AM_RC: "rc", L.AM_TOKK: "tokk"}[d.mode], "aux" if d.aux else "no_aux", "rvalid<R" if d.rvalid < d.R else "rvalid=R",
            "ld_" + _w(d.ld, tight))


def _memset(d):
    if d.chunks:
        return (KIND_NAME[d.kind], "chunked")
    n = d.bytes >> 2
    if (d.bytes & 3) or ((d.ptr or 0) & 15):
        return (KIND_NAME[d.kind], "flat", "runtime_memset")
    # (16-byte stores, a scalar tail, and a grid-stride loop once 2048 workgroups no longer cover the range)
    return (KIND_NAME[d.kind], "flat", "kernel", "tail" if n & 3 else "no_tail", "strided" if (n >> 2) > 2048 * 256 else "one_pass")


def _const_i64(d):
    return (KIND_NAME[d.kind], "n<=256" if d.n <= 256 else "n>256")  # (one workgroup of 256 threads walks the values)


def _scale(d):
    return (KIND_NAME[d.kind], "strided" if d.n > 2048 * 256 else "one_pass", "in_place" if d.x == d.y else "out_of_place")


def _final(d):
    segs = []
    for q in range(d.nseg):
        ds = bool(d.dseg[q]) and d.kind != L.OP_FINAL_FWD
        segs.append(("seg" if d.seg[q] else "null", "dseg" if ds else "no_dseg", "acc" if (ds and d.dseg_accumulate[q]) else "set",
                     "tok_stride" if d.tok_stride[q] else "contiguous"))
    bwd = d.kind == L.OP_FINAL_BWD
    return (KIND_NAME[d.kind], "nseg%d" % d.nseg, tuple(sorted(set(segs))), "fused_loss" if (bwd and d.y) else "plain",
            "batch_slices" if (bwd and d.nsplit > 0) else "no_slices", "rows16" if (bwd and d.B >= 1024) else "rows1")


# ---- NASREC_OP_GEMM ----------------------------------------------------------------------------------------------------------------------
GEMM_FAMILY = {L.GEMM_ROUTE_GENERAL: "general", L.GEMM_ROUTE_KSLICE: "kslice", L.GEMM_ROUTE_SKINNY_N: "skinny_n", L.GEMM_ROUTE_TINYK: "tinyk",
               L.GEMM_ROUTE_TOKEN_LINEAR: "token_linear", L.GEMM_ROUTE_TOKEN_DW: "token_dw", L.GEMM_ROUTE_FAST: "fast"}
_AM = {L.AM_KC: "KC", L.AM_RC: "RC", L.AM_TOKR: "TOKR", L.AM_TOKK: "TOKK"}
_CM = {L.CM_PLAIN: "PLAIN", L.CM_TOKJ: "TOKJ"}
_ACT = {L.ACT_NONE: "act_none", L.ACT_RELU: "relu", L.ACT_SILU: "silu", L.ACT_SIGMOID: "sigmoid"}
_PRECISION = {L.PRECISION_HIGHEST: "highest", L.PRECISION_HIGH: "high", L.PRECISION_MEDIUM: "medium"}
# the configurations of the general template (csrc/gemm.hip launch_general_t) x the bodies launch_ring picks between
GENERAL_CONFIGS = ("big64x64", "mid64x64.deep", "mid64x64.shallow", "z32x32.deep", "64x16.deep", "64x16.shallow", "16x64.deep", "16x64.shallow")
GENERAL_BODIES = ("ring", "ring_aux", "plain_template")


def gemm_problems(d):
    """the segments that are problems of their own: every segment of a zmode launch, seg[0] otherwise"""
    return [d.seg[q] for q in range(d.nseg if d.zmode else 1)]


def gemm_uniform(d):
    """launch_ring's `uniform` (csrc/gemm.hip): the k-segments of one product agree on ones_col, Mvalid and on having mask operands"""
    if d.zmode:
        return True
    s0 = d.seg[0]
    for q in range(d.nseg):
        s = d.seg[q]
        if s.ones_col != s0.ones_col or s.Mvalid != s0.Mvalid:
            return False
        if s.A and (bool(s.Aaux) != bool(s0.Aaux) or bool(s.Baux) != bool(s0.Baux)):
            return False
    return True


def general_config(d):
    """-> (tile configuration, body) of the general template, as launch_general_t and launch_ring of csrc/gemm.hip decide: by the live
    workgroups of a 64 x 64 tiling x split-K (>= 1024: the 256-thread 64 x 64 template; >= GEMM_SKINNY_BELOW = 128: 64 x 64 on 1024
    threads, or 32 x 32 for a zmode batch of deep products; below: 64 x 16 strips when Nmax >= Mmax, else 16 x 64), by the deepest live
    k-segment (> 32: "deep"), and — except for the first — ring / ring with mask operands / the plain template when the k-segments
    disagree"""
    probs = gemm_problems(d)
    S = d.splitk if d.splitk > 1 else 1
    wgs = sum(((s.M + 63) // 64) * ((s.N + 63) // 64) * S for s in probs)
    deep = max([d.seg[q].K for q in range(d.nseg) if d.seg[q].A] + [0]) > 32
    Mmax, Nmax = max(s.M for s in probs), max(s.N for s in probs)
    if wgs >= 1024:
        return "big64x64", "plain_template"
    if wgs >= 128:
        cfg = "z32x32.deep" if (d.zmode and len(probs) > 1 and deep) else ("mid64x64.deep" if deep else "mid64x64.shallow")
    else:
        cfg = ("64x16" if Nmax >= Mmax else "16x64") + (".deep" if deep else ".shallow")
    if not gemm_uniform(d):
        return cfg, "plain_template"
    aux = any(d.seg[q].Aaux or d.seg[q].Baux for q in range(d.nseg))
    return cfg, "ring_aux" if aux else "ring"


def _fast_paths(d, probs, split):
    """the ways through ft_epilogue (csrc/gemm_fast_common.h) the problems of a launch take: a split launch leaves the epilogue to the
    common second pass; else acc_in_tile (ft_acc_init), the `plain` stores, the one-array path by what it reads, or the full path"""
    if split.startswith("split"):
        return ("second_pass",)
    out = set()
    for s in probs:
        acc = bool(s.accumulate if d.zmode else d.beta)
        mv = 0 < s.Mvalid < s.M
        bare = not (d.bias or d.pre_add or d.save_z or d.save_act or d.act != L.ACT_NONE or d.mul_nseg > 0 or d.dims_in_use >= 0 or s.ones_col)
        if bare and acc and not mv and split == "s1":
            out.add("acc_in_tile")
        elif bare and not acc:
            out.add("plain")
        elif s.ones_col:
            out.add("full_ones")
        else:
            nread = (1 if d.mul_nseg > 0 else 0) + (1 if d.pre_add else 0) + (1 if acc else 0)
            out.add("nread0" if nread == 0 else ("nread1" if nread == 1 else "full_nread2+"))
    return tuple(sorted(out))


def _gemm(d):
    """One property per branch of the seven GEMM families' launchers and epilogues (csrc/gemm.hip, gemm_tile.h, gemm_ring.h,
    gemm_fast_common.h, gemm_fast.hip, gemm_kslice.hip, gemm_skinny.hip, token_linear.hip, token_linear_common.h).  The family and the
    kernel's name are the library's own answers (plan.gemm_route = nasrec_gemm_route, plan.gemm_kernel_name); the general template's
    configuration restates launch_general_t / launch_ring (general_config above).  What no kernel branches on is left out: the value of
    dims_in_use (a comparison per element), the shapes beyond what picks a configuration, the strides.  The precision is part of the
    form; the harvest compiles at HIGHEST only — the bf16 bodies are held to their own error bound by tests/test_gemm_bf16_gpu.py and
    tests/test_token_linear_bf16_gpu.py and have no case in tests/gemm_cases.py."""
    route = P.gemm_route(d)[0]
    family = GEMM_FAMILY.get(route, "rejected%d" % route)
    kernel = P.gemm_kernel_name(d) if route >= 0 else "none"
    probs = gemm_problems(d)
    segs = [d.seg[q] for q in range(d.nseg)]
    split = "balanced" if d.splitk == L.SPLITK_BALANCED else ("s1" if d.splitk <= 1 else ("split_deferred" if d.defer_second_pass else "split"))
    Mmax, Nmax = max(s.M for s in probs), max(s.N for s in probs)
    if route == L.GEMM_ROUTE_GENERAL:
        cfg = ".".join(general_config(d))
    elif route == L.GEMM_ROUTE_FAST:
        cfg = ("ones_template" if any(s.ones_col for s in segs) else "no_ones_template") + "." + "+".join(_fast_paths(d, probs, split))
    elif route == L.GEMM_ROUTE_SKINNY_N:
        cfg = "4waves" if (probs[0].M + 15) // 16 >= 512 else "8waves"  # launch_gemm_skinny_n
    elif route == L.GEMM_ROUTE_TINYK:  # gemm_tinyk_kernel's `simple`
        simple = not (d.pre_add or d.mul_nseg > 0 or d.dims_in_use >= 0 or (d.bias and d.bias_on_rows) or any((s.accumulate if d.zmode else d.beta) for s in probs))
        cfg = "simple" if simple else "col4"
    elif route == L.GEMM_ROUTE_TOKEN_LINEAR:  # launch_token_linear: RB row blocks; the grid is shared out over the problems of a batch (z = blockIdx.x / wgs)
        cfg = "rb%d.%s" % ((probs[0].M + 15) // 16, "batch" if len(probs) > 1 else "one_problem")
    elif route == L.GEMM_ROUTE_TOKEN_DW:  # launch_token_dw: RB x CB blocks of 16
        cfg = "rb%d.cb%d" % ((Mmax + 15) // 16, (Nmax + 15) // 16)
    else:
        cfg = "-"
    accs = set(bool(s.accumulate if d.zmode else d.beta) for s in probs)
    acc = "acc_mixed" if len(accs) > 1 else ("accumulate" if accs.pop() else "overwrite")
    gate = "no_gate"
    if d.mul_nseg > 0:
        gap = not _covered(Nmax, [(d.mul_off[q], d.mul_width[q]) for q in range(d.mul_nseg)])
        null = any(not d.mul_ptr[q] for q in range(d.mul_nseg))
        gate = "gate_" + ("gap" if gap else "covering") + ("_null" if null else "")
    ones = "no_ones"
    if any(s.ones_col for s in segs):
        own = set(bool(s.rowsum) for s in probs if s.ones_col)
        ones = "ones_own_rowsum" if own == {True} else ("ones_rowsum_out" if own == {False} else "ones_both")
    aux = "aux_" + (("A" if any(s.Aaux for s in segs) else "") + ("B" if any(s.Baux for s in segs) else "") or "none")
    return (KIND_NAME[d.kind], family, kernel, cfg, "%s.%s.%s" % (_AM[d.amode], _AM[d.bmode], _CM[d.cmode]),
            ("z" if d.zmode else "k") + ("1" if d.nseg == 1 else "N"), "uniform" if gemm_uniform(d) else "disagree", split, _ACT[d.act],
            "no_bias" if not d.bias else ("bias_rows" if d.bias_on_rows else "bias_cols"),
            "no_mask" if d.dims_in_use < 0 else ("mask_rows" if d.mask_on_rows else "mask_cols"), acc, "pre_add" if d.pre_add else "no_pre",
            "save_z" if d.save_z else "no_z", "save_act" if d.save_act else "no_sact", gate, ones, aux,
            "mvalid<M" if any(0 <= s.Mvalid < s.M for s in segs) else "mvalid=M", "null_A" if any(not s.A for s in segs) else "live_A",
            _PRECISION.get(d.precision, "precision%d" % d.precision))


FORM_FN = {L.OP_GEMM: _gemm, L.OP_MHA_FWD: _mha, L.OP_MHA_BWD: _mha, L.OP_FM_FWD: _fm, L.OP_FM_BWD: _fm, L.OP_DOT_TRI_FWD: _dot_tri, L.OP_DOT_TRI_BWD: _dot_tri,
           L.OP_GATE_BWD: _gate, L.OP_COPY_SEGS: _copy, L.OP_REDUCE_ROWS: _reduce, L.OP_ACT_BWD: _act_bwd, L.OP_ROWSUM: _rowsum,
           L.OP_MEMSET: _memset, L.OP_CONST_I64: _const_i64, L.OP_SCALE: _scale, L.OP_FINAL_FWD: _final, L.OP_FINAL_FUSED: _final,
           L.OP_FINAL_BWD: _final}


def form_of(d):
    """-> the tuple of properties of descriptor `d` that select code or addressing in its kernel; KeyError for a kind without one"""
    return FORM_FN[d.kind](d)


# ---- the harvest ---------------------------------------------------------------------------------------------------------------------
FD, FS = 13, 26
BATCHES = (256, 2048)
SAMPLED_PATHS = 24
SEED = 20240521


class _Span:
    """an address range that stands in for a tensor: the plan compiler asks a buffer for its address and its size, nothing else"""
    __slots__ = ("shape", "_ptr", "_n")

    def __init__(self, ptr, shape):
        self.shape, self._ptr, self._n = tuple(shape), ptr, int(np.prod(shape, dtype=np.int64))

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n


class Addresses:
    """what engine.Arena is to a plan on the device, without memory behind it: 256-byte aligned addresses handed out in order (no
    descriptor of a host-side plan is ever launched)"""

    def __init__(self, base=1 << 40):
        self.next = base

    def alloc(self, numel, dtype=None, shape=None):
        ptr = self.next
        self.next += (4 * int(numel) + 255) & ~255
        return _Span(ptr, shape if shape is not None else (int(numel),))


def compile_host(cfg, choice, B, train):
    """-> (forward descriptors, backward descriptors) of one plan, before any scheduling (what ends up a worklist item is still a
    descriptor of its own here).  The settings the engine derives from (cfg, B) are derived the same way (engine.py compile)."""
    mem = Addresses()
    shapes = P.infer_param_shapes(cfg, choice if cfg.fixed else P.full_path_choice(cfg), FD, FS, [11] * FS)
    shapes = {n: s for n, s in shapes.items() if not n.startswith("_embedding.")}
    params = {n: mem.alloc(np.prod(s, dtype=np.int64), shape=s) for n, s in shapes.items()}
    grads = {n: mem.alloc(np.prod(s, dtype=np.int64), shape=s) for n, s in shapes.items()} if train else None
    ctx = P.Ctx(B, torch.device("cpu"), params, grads, shape_only=False, train=train)
    ctx.arena = mem
    scheduled = cfg.fixed and B <= 256
    ctx.defer_dw = not scheduled
    if scheduled:
        ctx.mha_bwd_form = 4
    sbuf = ctx.buf(B * FS * E)
    ctx.raw_sparse = sbuf
    d_last, s_last = P.network_walk(ctx, cfg, choice, P.DV(P.Buf(ctx, B * FD, False), 0, FD, FD), P.SV(sbuf, 0, FS, FS * E))
    if train:
        for v in d_last + s_last:  # (the final-logit backward writes these gradients: FINAL_* has tests of its own)
            v.buf.grad_tensor()
            v.buf.mark(*v.cols())
        ctx.build_backward()
    return list(ctx.fwd), list(ctx.bwd)


def _plain(o):
    return json.loads(json.dumps(o, default=lambda v: v.tolist() if hasattr(v, "tolist") else int(v)))


def plans():
    """-> [(label, cfg, choice)] of everything harvested"""
    from nasrec_amd.search_space import ops_config_lib
    from nasrec_amd.supernet.supernet import SuperNet
    out = []
    for f in sorted(glob.glob(os.path.join(ROOT, "nasrec_amd", "configs", "*", "*.json"))):
        ca = json.load(open(f))
        cfg = P.NetConfig(ca["num_blocks"], ops_config_lib[ca["config"]], False, "relu", fixed=True)
        out.append(("fixed:" + os.path.basename(f), cfg, {"macro": ca["macro"], "micro": ca["micro"]}))
    for space in ("xlarge", "autoctr"):
        cfg = P.NetConfig(7, ops_config_lib[space], True)
        out.append(("full:%s:layernorm" % space, cfg, P.full_path_choice(cfg)))
        cfg = P.NetConfig(7, ops_config_lib[space], False, "silu")
        out.append(("full:%s:silu" % space, cfg, P.full_path_choice(cfg)))
    state = np.random.get_state()
    try:
        np.random.seed(SEED)
        for space, ln, act in (("xlarge", True, "relu"), ("xlarge", False, "silu"), ("autoctr", True, "relu")):
            cfg = P.NetConfig(7, ops_config_lib[space], ln, act)
            net = SuperNet(num_blocks=7, ops_config=ops_config_lib[space], use_layernorm=ln, activation=act, num_embeddings=[11] * FS,
                           path_sampling_strategy="default")
            for i in range(SAMPLED_PATHS // 3):
                out.append(("sampled:%s:%s:%d" % (space, "layernorm" if ln else act, i), cfg, _plain(net._resolve_choice(None))))
    finally:
        np.random.set_state(state)
    return out


def harvest(batches=BATCHES, trains=(True, False), every=None):
    """-> ({form: example descriptor}, {kind: count} of the kinds form_of does not know); every: a list that receives every
    descriptor of a known kind"""
    forms, unknown = {}, {}
    for label, cfg, choice in plans():
        for B in batches:
            for train in trains:
                fwd, bwd = compile_host(cfg, choice, B, train)
                for d in fwd + bwd:
                    if d.kind in FORM_FN:
                        forms.setdefault(form_of(d), d)
                        if every is not None:
                            every.append(d)
                    else:
                        unknown[d.kind] = unknown.get(d.kind, 0) + 1
    return forms, unknown
