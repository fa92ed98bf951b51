"""The ROC AUC contract on the host: the NumPy restatement of sklearn's computation (tests/roc_auc_restated.py, what
NASREC_OP_ROC_AUC implements) against sklearn itself, the harness's routing of host tensors, and the op's C-ABI layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import sklearn.metrics
import torch

from nasrec_amd import _lib as L
from nasrec_amd import metrics
from nasrec_amd.utils import train_utils as TU
from roc_auc_restated import curve_points, inputs_with_kept_points, pairwise_sum, roc_auc_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.choice([2, 3, 5, 7, 8, 9, 16, 100, 127, 128, 129, 1000, 8191, 8193, 20000, 40000]))
    y = (rng.random(n) < rng.uniform(0.02, 0.98)).astype(np.float32)
    y[:2] = (0.0, 1.0)
    z = rng.normal(size=n) + y * rng.uniform(0.0, 2.0)
    kind = seed % 5
    if kind == 1:  # heavy ties
        z = np.round(z * rng.choice([1, 4, 30]))
    if kind == 2:  # raw logits with both zeros
        s = z.astype(np.float32)
        s[rng.random(n) < 0.2] = -0.0
        s[rng.random(n) < 0.2] = 0.0
        return y, s
    s = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    if kind == 3:  # saturated
        s[rng.random(n) < 0.3] = 1.0
        s[rng.random(n) < 0.3] = 0.0
    if kind == 4:  # denormals
        s = (s * np.float32(1e-38) * np.float32(1e-5)).astype(np.float32)
    return y, s


@pytest.mark.parametrize("block", range(6))
def test_restatement_is_bit_equal_to_sklearn(block):
    for seed in range(block * 50, block * 50 + 50):
        y, s = _case(seed)
        want = float(sklearn.metrics.roc_auc_score(y, s))
        assert roc_auc_restated(y, s).hex() == want.hex(), (seed, len(y))


@pytest.mark.parametrize("k", [7, 8, 127, 128, 129, 8191, 8192, 8193, 3 * 8192 + 5])
def test_restatement_at_chunk_and_leaf_edges(k):
    y, s = inputs_with_kept_points(k, seed=k)
    assert len(curve_points(y, s)[0]) == k
    assert roc_auc_restated(y, s).hex() == float(sklearn.metrics.roc_auc_score(y, s)).hex()


def test_restatement_needs_the_chunked_order():
    """summing every term in one pairwise tree, without numpy's 8192-element reduction buffer, is not the contract: at 100 000
    scores the two orders give different bits, and only the chunked one is sklearn's"""
    rng = np.random.default_rng(0)
    n = 100000
    y = (rng.random(n) < 0.3).astype(np.float32)
    s = (1.0 / (1.0 + np.exp(-(rng.normal(size=n) + y)))).astype(np.float32)
    fps, tps = curve_points(y, s)
    fps, tps = np.r_[0, fps].astype(np.float64), np.r_[0, tps].astype(np.float64)
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    one_tree = pairwise_sum(((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2.0).tolist())
    want = float(sklearn.metrics.roc_auc_score(y, s))
    assert roc_auc_restated(y, s).hex() == want.hex()
    assert one_tree.hex() != want.hex()


def test_auroc_sends_host_tensors_to_sklearn(monkeypatch):
    def device_path(*a, **k):
        raise AssertionError("host tensors took the device path")
    monkeypatch.setattr(metrics, "roc_auc_score", device_path)
    y, s = _case(3)
    got = TU._auroc(torch.from_numpy(y), torch.from_numpy(s))
    assert float(got).hex() == float(sklearn.metrics.roc_auc_score(y, s)).hex()
    assert not metrics.roc_auc_supported(torch.from_numpy(y), torch.from_numpy(s))


def test_roc_auc_rejects_host_tensors():
    y, s = _case(4)
    with pytest.raises(ValueError, match="CUDA"):
        metrics.roc_auc_score(torch.from_numpy(y), torch.from_numpy(s))


def test_roc_auc_desc_layout_and_kind():
    lib = L.load()
    sizes = (C.c_int32 * 43)()
    n = lib.nasrec_desc_sizes(sizes, 43)
    assert n == 43 and L.OP_ROC_AUC == 42
    assert sizes[L.OP_ROC_AUC] == C.sizeof(L.RocAucDesc) == 56
    assert [f[0] for f in L.RocAucDesc._fields_] == ["kind", "_pad", "n", "score", "label", "workspace", "workspace_bytes", "out"]
    hdr = open(os.path.join(ROOT, "include", "nasrec_hip.h")).read()
    assert re.search(r"NASREC_OP_ROC_AUC = 42\b", hdr)
    assert int(re.search(r"#define NASREC_ROC_AUC_MAX_N \(1ll << (\d+)\)", hdr).group(1)) == L.ROC_AUC_MAX_N.bit_length() - 1
    for name, bit in (("TOO_FEW", L.ROC_AUC_TOO_FEW), ("BAD_LABEL", L.ROC_AUC_BAD_LABEL), ("NOT_FINITE", L.ROC_AUC_NOT_FINITE),
                      ("ONE_CLASS", L.ROC_AUC_ONE_CLASS)):
        assert re.search(r"NASREC_ROC_AUC_%s = %d\b" % (name, bit), hdr)


def test_roc_auc_workspace_bytes():
    lib = L.load()
    assert lib.nasrec_roc_auc_workspace_bytes(0) == 0 and lib.nasrec_roc_auc_workspace_bytes(1) == 0
    assert lib.nasrec_roc_auc_workspace_bytes(L.ROC_AUC_MAX_N + 1) == 0
    sizes = [lib.nasrec_roc_auc_workspace_bytes(n) for n in (2, 4096, 4097, 1228800, 4600000)]
    assert all(b > 0 and b % 256 == 0 for b in sizes) and sizes == sorted(sizes)
    assert sizes[-1] < 19 * 4600000  # keys and labels twice, the group ends' int32 counts (the kept points reuse the keys): 18 B a sample
    d = L.RocAucDesc(kind=L.OP_ROC_AUC, n=L.ROC_AUC_MAX_N + 1, out=256)  # (never dereferenced: refused before any launch)
    assert lib.nasrec_roc_auc(None, C.byref(d)) != 0
    assert b"at most" in lib.nasrec_last_error()
    d.kind = L.OP_LAST_LAYER_STEP
    assert lib.nasrec_roc_auc(None, C.byref(d)) != 0 and b"does not match" in lib.nasrec_last_error()
