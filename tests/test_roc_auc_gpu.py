"""nasrec_amd.metrics.roc_auc_score (NASREC_OP_ROC_AUC on the GPU) against sklearn.metrics.roc_auc_score, bit for bit (float.hex), and
the harness's evaluation through it.  Every valid input must be answered by the device itself: the op's status word is read through
metrics._roc_auc_device and must be 0 (a non-zero status would hand the input to sklearn and hide the op's answer)."""
import warnings

import numpy as np
import pytest
import sklearn.metrics
import torch
import torch.nn as nn

from nasrec_amd import _lib as L
from nasrec_amd import metrics
from nasrec_amd.utils import train_utils as TU
from roc_auc_restated import curve_points, inputs_with_kept_points

pytestmark = pytest.mark.gpu


def _sigmoid_case(n, seed, tie_scale=None):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.25).astype(np.float32)
    y[0], y[-1] = 1.0, 0.0
    z = rng.normal(size=n) + 0.8 * y
    if tie_scale is not None:
        z = np.round(z * tie_scale) / tie_scale
    return y, (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def _special_cases():
    rng = np.random.default_rng(11)
    n = 5000
    y = (rng.random(n) < 0.4).astype(np.float32)
    y[:2] = (0.0, 1.0)
    out = {"all_equal": (y, np.full(n, 0.375, np.float32))}
    z = rng.normal(size=n)
    out["saturated"] = (y, np.where(z > 0.5, 1.0, np.where(z < -0.5, 0.0, 1.0 / (1.0 + np.exp(-z)))).astype(np.float32))
    out["denormals"] = (y, (rng.integers(1, 1 << 12, size=n) * np.float32(1.4e-45)).astype(np.float32))
    z = rng.normal(size=n).astype(np.float32)
    z[rng.random(n) < 0.3] = 0.0
    z[rng.random(n) < 0.3] = -0.0
    out["signed_zeros"] = (y, z)
    one_pos = np.zeros(n, np.float32)
    one_pos[1234] = 1.0
    out["single_positive"] = (one_pos, rng.random(n).astype(np.float32))
    out["single_negative"] = (1.0 - one_pos, rng.random(n).astype(np.float32))
    return out


def _check(y, s, device="cuda"):
    want = float(sklearn.metrics.roc_auc_score(y, s))
    yt, st = torch.from_numpy(y).to(device), torch.from_numpy(s).to(device)
    auc, status = metrics._roc_auc_device(yt, st)
    assert status == 0, "the device handed a valid input to sklearn (status %d)" % status
    assert auc.hex() == want.hex(), (auc, want)
    got = metrics.roc_auc_score(yt, st)
    assert isinstance(got, float) and got.hex() == want.hex()
    return got


@pytest.mark.parametrize("n", [2, 7, 8, 9, 1000, 1228800, 4600000])
def test_sigmoid_scores(n):
    _check(*_sigmoid_case(n, seed=n))


@pytest.mark.parametrize("n,scale", [(1000, 2), (1228800, 10), (1228800, 1000), (4600000, 100)])
def test_heavily_tied_scores(n, scale):
    _check(*_sigmoid_case(n, seed=n + scale, tie_scale=scale))


@pytest.mark.parametrize("k", [7, 8, 127, 128, 129, 8191, 8192, 8193, 3 * 8192 + 5])
def test_kept_points_at_leaf_and_chunk_edges(k):
    y, s = inputs_with_kept_points(k, seed=k)
    assert len(curve_points(y, s)[0]) == k
    _check(y, s)


@pytest.mark.parametrize("name", list(_special_cases()))
def test_special_scores(name):
    _check(*_special_cases()[name])


def test_repeated_calls_are_bit_identical():
    y, s = _sigmoid_case(1228800, seed=5, tie_scale=300)
    yt, st = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
    first, status = metrics._roc_auc_device(yt, st)
    assert status == 0 and first.hex() == float(sklearn.metrics.roc_auc_score(y, s)).hex()
    for _ in range(5):
        auc, status = metrics._roc_auc_device(yt, st)
        assert status == 0 and auc.hex() == first.hex()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_second_device_while_first_is_current():
    y, s = _sigmoid_case(100000, seed=3)
    with torch.cuda.device(0):
        _check(y, s, device="cuda:1")
        assert torch.cuda.current_device() == 0


def _outcome(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            r = fn()
            return ("value", float(r).hex(), sorted({(type(x.message).__name__, str(x.message)) for x in w}))
        except Exception as e:  # noqa: BLE001
            return ("raised", type(e).__name__, str(e))


@pytest.mark.parametrize("case,status", [("one_class", L.ROC_AUC_ONE_CLASS), ("nan", L.ROC_AUC_NOT_FINITE), ("inf", L.ROC_AUC_NOT_FINITE),
                                         ("label_2", L.ROC_AUC_BAD_LABEL), ("one_sample", L.ROC_AUC_TOO_FEW)])
def test_failures_match_sklearn(case, status):
    y, s = _sigmoid_case(1000, seed=9)
    if case == "one_class":
        y = np.ones_like(y)
    elif case == "nan":
        s[17] = np.nan
    elif case == "inf":
        s[17] = np.inf
    elif case == "label_2":
        y[17] = 2.0
    else:
        y, s = y[:1], s[:1]
    assert metrics._roc_auc_device(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())[1] == status
    want = _outcome(lambda: sklearn.metrics.roc_auc_score(y, s))
    got = _outcome(lambda: metrics.roc_auc_score(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()))
    assert got == want


def test_inputs_that_are_not_1d_go_to_sklearn():
    y, s = _sigmoid_case(1000, seed=4)
    yt, st = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda().view(500, 2)
    assert not metrics.roc_auc_supported(yt, st)
    with pytest.raises(ValueError, match="1-D"):
        metrics.roc_auc_score(yt, st)
    want = _outcome(lambda: sklearn.metrics.roc_auc_score(y, s.reshape(500, 2)))
    assert want[0] == "raised" and _outcome(lambda: TU._auroc(yt, st)) == want


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(13, 1)
        self.emb = nn.Embedding(1000, 1)

    def forward(self, int_x, cat_x):
        return self.lin(int_x).squeeze(-1) + self.emb(cat_x).sum(1).squeeze(-1)


def test_test_one_epoch_auroc_equals_sklearn(monkeypatch):
    torch.manual_seed(0)
    model = _Tiny().cuda()
    g = torch.Generator().manual_seed(1)
    loader = [(torch.randn(512, 13, generator=g), torch.randint(0, 1000, (512, 26), generator=g),
               (torch.rand(512, generator=g) < 0.3).float()) for _ in range(6)]
    calls = []
    device_auc = metrics._roc_auc_device

    def spy(y_true, y_score):
        r = device_auc(y_true, y_score)
        calls.append((y_true.device, y_score.dtype, r))
        return r
    monkeypatch.setattr(metrics, "_roc_auc_device", spy)
    acc, auroc, loss = TU.test_one_epoch(model, loader, nn.BCEWithLogitsLoss(), gpu=0)
    assert len(calls) == 1 and calls[0][0].type == "cuda" and calls[0][1] == torch.float32
    assert calls[0][2][1] == 0 and calls[0][2][0].hex() == auroc.hex()  # the device's own answer
    with torch.no_grad():
        prob = torch.sigmoid(torch.cat([model(i.cuda(), c.cuda()) for i, c, _ in loader]).flatten()).cpu().numpy()
    labels = torch.cat([y for _, _, y in loader]).numpy()
    assert auroc.hex() == float(sklearn.metrics.roc_auc_score(labels, prob)).hex()
