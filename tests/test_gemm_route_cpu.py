"""nasrec_gemm_route (include/nasrec_hip.h, csrc/gemm.hip): the one rule by which the launcher picks a GEMM kernel family and which the
planner queries.  Host only: no device, nothing is launched, and every pointer below is an arbitrary non-null integer that must never
be followed.  The expected family and eligibility bits of each case are written out by hand from the rules beside the kernels
(gemm_kslice.hip, gemm_skinny.hip, token_linear.hip, gemm_fast.hip), each boundary from both sides; they assume the shipped values of
the measurement knobs, which the library reads once per process."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nasrec_amd import _lib as L  # noqa: E402
from nasrec_amd import plan as P  # noqa: E402

pytestmark = pytest.mark.skipif(any(os.environ.get(k) is not None for k in ("NASREC_SKINNY_N", "NASREC_TINYK", "NASREC_FAST_MIN_K")),
                                reason="the table states the rule at the shipped values of its A/B knobs")

KC, RC, TOKR, TOKK, PLAIN, TOKJ = L.AM_KC, L.AM_RC, L.AM_TOKR, L.AM_TOKK, L.CM_PLAIN, L.CM_TOKJ
GENERAL, KSLICE, SKINNY_N, TINYK, TOKEN_LINEAR, TOKEN_DW, FAST = range(7)
G, KS, SN, TK, TL, TD, F = (1 << k for k in range(7))
PTR = 0x1000  # never dereferenced


def seg(M, N, K, **kw):
    s = dict(A=PTR, B=PTR + 8, C=PTR + 16, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, Mvalid=M)
    s.update(kw)
    return s


def desc(binding, segs, zmode=0, splitk=1, workspace=None, **kw):
    d = L.GemmDesc()
    d.kind = L.OP_GEMM
    d.amode, d.bmode, d.cmode = binding
    d.nseg, d.zmode, d.splitk, d.dims_in_use = len(segs), zmode, splitk, -1
    if workspace is None:
        workspace = PTR + 24 if splitk > 1 or splitk == L.SPLITK_BALANCED else 0
    d.workspace = workspace
    for k, v in kw.items():
        setattr(d, k, v)
    for q, s in enumerate(segs[:L.MAX_SEGS]):
        for k, v in s.items():
            setattr(d.seg[q], k, v)
    return d


FWD, DX, DW, TOK_FWD, TOK_DX, TOK_DW = (KC, KC, PLAIN), (KC, RC, PLAIN), (RC, RC, PLAIN), (KC, TOKR, TOKJ), (RC, TOKR, TOKJ), (TOKK, TOKK, PLAIN)
TOKENS = 1024 * 16   # N of a token-axis Linear over 1024 samples
TDW = [seg(80, 72, TOKENS), seg(16, 80, TOKENS)]  # two token-axis weight gradients over 1024 samples

# (name, descriptor, expected family, expected mask)
CASES = [
    # ---- gemm_kslice_eligible: KC/KC/PLAIN, one problem, splitk <= 1, <= 4 segments, M <= 512, 128 <= 32x32 tiles <= 512, K >= 512 ----
    ("kslice base 256x1024x512 (256 tiles)", desc(FWD, [seg(256, 1024, 512)]), KSLICE, G | KS),
    ("kslice M=512 (16x16 tiles)", desc(FWD, [seg(512, 512, 512)]), KSLICE, G | KS),
    ("kslice M=513", desc(FWD, [seg(513, 512, 512)]), GENERAL, G),
    ("kslice 127 tiles", desc(FWD, [seg(32, 127 * 32, 512)]), GENERAL, G),
    ("kslice 128 tiles", desc(FWD, [seg(32, 128 * 32, 512)]), KSLICE, G | KS),
    ("kslice 512 tiles", desc(FWD, [seg(32, 512 * 32, 512)]), KSLICE, G | KS),
    ("kslice 513 tiles", desc(FWD, [seg(32, 513 * 32, 512)]), GENERAL, G),
    ("kslice K=511", desc(FWD, [seg(256, 1024, 511)]), GENERAL, G),
    ("kslice 4 k-segments", desc(FWD, [seg(256, 1024, 128)] * 4), KSLICE, G | KS),
    ("kslice 5 k-segments", desc(FWD, [seg(256, 1024, 128)] * 5), GENERAL, G),
    ("kslice splitk=2", desc(FWD, [seg(256, 1024, 512)], splitk=2), GENERAL, G),
    ("kslice wrong binding (dx)", desc(DX, [seg(256, 1024, 512)]), GENERAL, G),
    # ---- gemm_skinny_n_eligible: KC/KC or KC/RC, PLAIN, splitk <= 1, 1 <= N <= 16, M >= 1024, K >= 256 ---------------------------
    ("skinny base 1024x16x256", desc(FWD, [seg(1024, 16, 256)]), SKINNY_N, G | SN),
    ("skinny KC/RC", desc(DX, [seg(1024, 16, 256, ldb=16)]), SKINNY_N, G | SN),
    ("skinny N=17", desc(FWD, [seg(1024, 17, 256)]), GENERAL, G),
    ("skinny M=1023", desc(FWD, [seg(1023, 16, 256)]), GENERAL, G),
    ("skinny K=255", desc(FWD, [seg(1024, 16, 255)]), GENERAL, G),
    ("skinny splitk=2", desc(FWD, [seg(1024, 16, 256)], splitk=2), GENERAL, G),
    # ---- gemm_tinyk_eligible: KC/KC, PLAIN, splitk <= 1, every problem M >= 1024, N >= 256, K <= 16 -------------------------------
    ("tinyk base 1024x256x16", desc(FWD, [seg(1024, 256, 16)]), TINYK, G | TK),
    ("tinyk K=17", desc(FWD, [seg(1024, 256, 17)]), GENERAL, G),
    ("tinyk N=255", desc(FWD, [seg(1024, 255, 16)]), GENERAL, G),
    ("tinyk KC/RC form is off", desc(DX, [seg(1024, 256, 16, ldb=256)]), GENERAL, G),
    # ---- token_linear_eligible: TOKR/TOKJ, A KC or RC, 1 <= M <= 80, N = 16 x (>= 1024 samples), weights + 80 bias floats <= 147456 B of LDS
    ("token_linear base 16 x 1024 samples", desc(TOK_FWD, [seg(16, TOKENS, 64)]), TOKEN_LINEAR, G | TL),
    ("token_linear dx binding", desc(TOK_DX, [seg(16, TOKENS, 64)]), TOKEN_LINEAR, G | TL),
    ("token_linear 1023 samples", desc(TOK_FWD, [seg(16, 1023 * 16, 64)]), GENERAL, G),
    ("token_linear M=80", desc(TOK_FWD, [seg(80, TOKENS, 64)]), TOKEN_LINEAR, G | TL),
    ("token_linear M=81", desc(TOK_FWD, [seg(81, TOKENS, 64)]), GENERAL, G),
    ("token_linear LDS: 456 x 80 x 4 + 320 = 146240 B", desc(TOK_FWD, [seg(80, TOKENS, 456)]), TOKEN_LINEAR, G | TL),
    ("token_linear LDS: 460 x 80 x 4 + 320 = 147520 B", desc(TOK_FWD, [seg(80, TOKENS, 457)]), GENERAL, G),
    ("token_linear N & 15", desc(TOK_FWD, [seg(16, TOKENS + 8, 64)]), GENERAL, G),
    ("token_linear two problems, 2 and 4 row blocks", desc(TOK_DX, [seg(23, TOKENS, 40), seg(56, TOKENS, 40)], zmode=1), GENERAL, G),
    # ---- token_dw_eligible: TOKK/TOKK/PLAIN zmode, splitk >= 2 with a workspace, M, N <= 80, K = 16 x (>= 1024 samples) -------------
    ("token_dw base, splitk=4", desc(TOK_DW, TDW, zmode=1, splitk=4), TOKEN_DW, G | TD),
    ("token_dw splitk=2", desc(TOK_DW, TDW, zmode=1, splitk=2), TOKEN_DW, G | TD),
    ("token_dw splitk=1", desc(TOK_DW, TDW, zmode=1, splitk=1), GENERAL, G),
    ("token_dw no workspace", desc(TOK_DW, TDW, zmode=1, splitk=4, workspace=0), GENERAL, G),
    ("token_dw 1023 samples", desc(TOK_DW, [seg(80, 72, 1023 * 16)] * 2, zmode=1, splitk=4), GENERAL, G),
    # ---- gemm_fast_eligible: PLAIN, KC/KC, KC/RC, RC/RC, no mask operands, 128x128 tiles x S >= 120, tiles at least half full, extents < 2^29
    ("fast 10 x 12 = 120 tiles", desc(FWD, [seg(1280, 1536, 64)]), FAST, G | F),
    ("fast 7 x 17 = 119 tiles", desc(FWD, [seg(896, 2176, 64)]), GENERAL, G),
    ("fast 30 tiles x splitk 4", desc(DW, [seg(640, 768, 4096, lda=640, ldb=768)], splitk=4), FAST, G | F),
    ("fast 30 tiles x splitk 3", desc(DW, [seg(640, 768, 4096, lda=640, ldb=768)], splitk=3), GENERAL, G),
    ("fast tiles exactly half full", desc(FWD, [seg(120 * 128, 64, 64)]), FAST, G | F),
    ("fast tiles less than half full", desc(FWD, [seg(120 * 128, 63, 64)]), GENERAL, G),
    ("fast Aaux operand", desc(FWD, [seg(1280, 1536, 64, Aaux=PTR + 32)]), GENERAL, G),
    ("fast extent 1536 x 349525 + 64 < 2^29", desc(FWD, [seg(1280, 1536, 64, lda=349525)]), FAST, G | F),
    ("fast extent 1536 x 349526 >= 2^29", desc(FWD, [seg(1280, 1536, 64, lda=349526)]), GENERAL, G),
    ("fast bias over rows", desc(FWD, [seg(1280, 1536, 64)], bias=PTR + 40, bias_on_rows=1), GENERAL, G),
    ("fast balanced schedule", desc(FWD, [seg(1280, 1536, 64)], splitk=L.SPLITK_BALANCED), FAST, F),
    # ---- precedence: the streaming kernel for K <= 16 wins over the throughput tile (64 x 8 = 512 tiles) ---------------------------
    ("tinyk before fast", desc(FWD, [seg(8192, 1024, 16)]), TINYK, G | TK | F),
    ("fast where tinyk's KC/RC form is off", desc(DX, [seg(8192, 1024, 16, ldb=1024)]), FAST, G | F),
    # ---- what the launcher rejects ---------------------------------------------------------------------------------------------------
    ("nseg=0", desc(FWD, []), L.GEMM_ROUTE_BAD_NSEG, 0),
    ("nseg=9", desc(FWD, [seg(64, 64, 64)] * 9), L.GEMM_ROUTE_BAD_NSEG, 0),
    ("binding RC/KC", desc((RC, KC, PLAIN), [seg(64, 64, 64)]), L.GEMM_ROUTE_BAD_BINDING, 0),
    ("balanced schedule on a small product", desc(FWD, [seg(64, 64, 64)], splitk=L.SPLITK_BALANCED), L.GEMM_ROUTE_BAD_BALANCED, 0),
]


@pytest.mark.parametrize("name,d,family,mask", CASES, ids=[c[0] for c in CASES])
def test_route_and_eligibility_bits(name, d, family, mask):
    assert P.gemm_route(d) == (family, mask)
    assert L.load().nasrec_gemm_route(P.C.addressof(d), None) == family  # the mask is optional


def test_families_and_kernel_names_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "nasrec_hip.h")).read()
    import re
    declared = {k: int(v) for k, v in re.findall(r"NASREC_GEMM_ROUTE_(\w+) = (-?\d+)", hdr)}
    assert declared == {k[len("GEMM_ROUTE_"):]: getattr(L, k) for k in dir(L) if k.startswith("GEMM_ROUTE_")}
    assert P.gemm_kernel_name(CASES[0][1]) == "gemm_kslice_kernel"
    assert P.gemm_kernel_name(desc(TOK_DW, TDW, zmode=1, splitk=4)) == "token_dw_kernel"
    assert P.gemm_kernel_name(desc(FWD, [seg(64, 64, 64)])) == "gemm_kernel"
    with pytest.raises(ValueError):
        P.gemm_kernel_name(desc((RC, KC, PLAIN), [seg(64, 64, 64)]))


DATASETS = {"criteo": (13, 26), "avazu": (1, 23), "kdd": (3, 10)}
CONFIGS = sorted(glob.glob(os.path.join(ROOT, "nasrec_amd", "configs", "*", "*.json")))


@pytest.mark.parametrize("B", [256, 4096])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[os.path.basename(c)[:-5] for c in CONFIGS])
def test_every_planned_gemm_routes_and_split_launches_have_a_split_form(cfg, B):
    import show_levels as SL
    assert len(CONFIGS) == 6
    Fd, Fs = DATASETS[os.path.basename(os.path.dirname(cfg))]
    ctx = SL.build_cpu_plan(cfg, B, Fd, Fs)
    gemms = [d for d in list(ctx.fwd) + list(ctx.bwd) if isinstance(d, L.GemmDesc)]
    assert gemms
    for d in gemms:
        family = P.gemm_route(d)[0]
        assert family >= 0, (family, d.amode, d.bmode, d.cmode, d.nseg, d.splitk)
        if d.splitk > 1:
            assert family in (GENERAL, FAST, TOKEN_DW), "a split launch on a single-pass kernel: %s" % P.gemm_kernel_name(d)
