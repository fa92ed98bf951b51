"""The descriptors of tests/test_opt_moments_refusals_cpu.py and of tools/record_opt_moments_refusals.py: NASREC_OP_OPT_MOMENTS
descriptors that can never launch (B = 0, dense_blocks = 0, nchunks = 0, nblocks = 0; lr / step point at one host float), so
launch_opt_moments (csrc/optim_moments.hip) answers each with a refusal and touches no device.

The core is the product of algo x sparse_rows x table_algo x phase x reg_mask x table_eps x momentum (2,800 descriptors, Fs = 1);
the variants change one more thing on the core's reg_mask = 0, table_eps = 1e-2, momentum = 0 slice: tm[1] set, the stamps and tv[0]
set, Fs = -1, Fs = MAX_TABLES + 1, lr missing."""
import ctypes as C
import itertools

from nasrec_amd import _lib as L

ALGOS, SPARSE, TABLE_ALGOS, PHASES = (0, 1, 2, 3, 4), (0, 1), tuple(range(7)), (-1, 0, 1, 2, 3)
REG_MASKS, TABLE_EPS, MOMENTA = (0, 1), (0.0, 1e-2), (0.0, 0.9)
VARIANTS = ("tm1", "stamps_tv0", "Fs-1", "Fs%d" % (L.MAX_TABLES + 1), "no_lr")

_HOST = (C.c_float * 4)()  # what lr / step / the variants' pointers point at: never read — nothing launches


def _desc(algo, sparse, table_algo, phase, reg_mask, table_eps, momentum, variant=None):
    d = L.OptMomentsDesc()
    d.kind, d.phase, d.algo, d.sparse_rows, d.table_algo = L.OP_OPT_MOMENTS, phase, algo, sparse, table_algo
    d.reg_mask, d.table_eps, d.momentum = reg_mask, table_eps, momentum
    d.Fs, d.beta1, d.beta2, d.eps, d.table_lr_scale = 1, 0.9, 0.999, 1e-8, 1.0
    d.lr = d.step = C.addressof(_HOST)
    if variant == "tm1":
        d.tm[1] = C.addressof(_HOST)
    elif variant == "stamps_tv0":
        d.tm[0] = d.tv[0] = C.addressof(_HOST)  # (the stamps travel in tm's storage)
    elif variant == "no_lr":
        d.lr = None
    elif variant is not None:
        d.Fs = int(variant[2:])
    return d


def cases():
    """[(key, descriptor)] in a fixed order; the key names every varied field"""
    out = []
    for a, s, t, p, r, e, m in itertools.product(ALGOS, SPARSE, TABLE_ALGOS, PHASES, REG_MASKS, range(2), range(2)):
        out.append(("a%d s%d t%d p%d r%d e%d m%d" % (a, s, t, p, r, e, m), _desc(a, s, t, p, r, TABLE_EPS[e], MOMENTA[m])))
    for v in VARIANTS:
        for a, s, t, p in itertools.product(ALGOS, SPARSE, TABLE_ALGOS, PHASES):
            out.append(("a%d s%d t%d p%d r0 e1 m0 %s" % (a, s, t, p, v), _desc(a, s, t, p, 0, TABLE_EPS[1], MOMENTA[0], v)))
    return out


def answer(lib, d):
    """(return code, nasrec_last_error) of one descriptor"""
    rc = lib.nasrec_opt_moments(None, C.addressof(d))
    return int(rc), lib.nasrec_last_error().decode(errors="replace")
