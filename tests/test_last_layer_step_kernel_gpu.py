"""NASREC_OP_LAST_LAYER_STEP (the optimizer tail of a last-layer fine-tune step, include/nasrec_hip.h) through the C-ABI against an
fp64 NumPy restatement of torch's formulas (clip_grad_norm_, torch.optim.Adagrad / Adam / SGD(momentum, nesterov)): widths K that are
not multiples of 4 or 64, the split backward's partial buffer, the clip binding and not, no clip, weight decay on the weight (and
skipped by no_reg), Adam's counter at 0 and above.  Two runs of the same step give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from nasrec_amd import _lib as L

pytestmark = pytest.mark.gpu

LR, EPS_ADAGRAD, EPS_ADAM, MOM, B1, B2 = 0.05, 1e-2, 1e-8, 0.9, 0.9, 0.999


def _case(K, nsplit, seed):
    g = torch.Generator().manual_seed(seed)
    c = {"w": torch.randn(K, generator=g) * 0.1, "b": torch.randn(1, generator=g) * 0.1,
         "s_w": torch.rand(K, generator=g) * 0.1, "s_b": torch.rand(1, generator=g) * 0.1,
         "v_w": torch.rand(K, generator=g) * 0.01, "v_b": torch.rand(1, generator=g) * 0.01}
    if nsplit > 1:
        c["partial"] = torch.randn(nsplit, K + 1, generator=g) * 0.3
    else:
        c["dw"], c["dbias"] = torch.randn(K, generator=g) * 0.3, torch.randn(1, generator=g) * 0.3
    return c


def _run(algo, c, K, nsplit, max_norm, wd, decay_w, steps):
    dev = torch.device("cuda", 0)
    t = {k: v.clone().to(dev) for k, v in c.items()}
    if nsplit > 1:
        t["dw"], t["dbias"] = torch.zeros(K, device=dev), torch.zeros(1, device=dev)
    step = torch.tensor(steps, dtype=torch.float32, device=dev)
    lr = torch.tensor([LR], dtype=torch.float32, device=dev)
    g_out, norm_out = torch.zeros(K + 1, device=dev), torch.zeros(2, device=dev)
    d = L.LastLayerStepDesc()
    d.kind, d.algo, d.K, d.nsplit, d.decay_w, d.nesterov = L.OP_LAST_LAYER_STEP, algo, K, nsplit, int(decay_w), 1
    d.max_norm, d.wd, d.momentum, d.beta1, d.beta2 = max_norm, wd, MOM, B1, B2
    d.eps = EPS_ADAGRAD if algo == L.OPTIM_ADAGRAD else EPS_ADAM
    d.partial = t["partial"].data_ptr() if nsplit > 1 else None
    d.dw, d.dbias, d.w, d.bias = t["dw"].data_ptr(), t["dbias"].data_ptr(), t["w"].data_ptr(), t["b"].data_ptr()
    d.s_w, d.s_b, d.v_w, d.v_b = t["s_w"].data_ptr(), t["s_b"].data_ptr(), t["v_w"].data_ptr(), t["v_b"].data_ptr()
    d.step, d.lr, d.g_out, d.norm_out = step.data_ptr(), lr.data_ptr(), g_out.data_ptr(), norm_out.data_ptr()
    s = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.load().nasrec_last_layer_step(s, C.addressof(d)))
    torch.cuda.synchronize(dev)
    out = {k: v.cpu() for k, v in t.items()}
    out.update(step=step.cpu(), g_out=g_out.cpu(), norm=norm_out.cpu())
    return out


def _ref(algo, c, K, nsplit, max_norm, wd, decay_w, steps):
    f = {k: v.double().numpy().copy() for k, v in c.items()}
    if nsplit > 1:
        g = f["partial"].sum(0)
    else:
        g = np.concatenate([f["dw"], f["dbias"]])
    raw = g.copy()
    if decay_w:
        g[:K] += 2.0 * wd * f["w"]
    total = np.sqrt((g * g).sum())
    coef = min(1.0, max_norm / (total + 1e-6)) if max_norm > 0 else 1.0
    g = g * coef
    p = np.concatenate([f["w"], f["b"]])
    s = np.concatenate([f["s_w"], f["s_b"]])
    v = np.concatenate([f["v_w"], f["v_b"]])
    if algo == L.OPTIM_ADAGRAD:
        s = s + g * g
        p = p - LR * g / (np.sqrt(s) + EPS_ADAGRAD)
    elif algo == L.OPTIM_ADAM:
        t = np.array([steps[0]] * K + [steps[1]]) + 1.0
        s = B1 * s + (1 - B1) * g
        v = B2 * v + (1 - B2) * g * g
        p = p - (LR / (1 - B1 ** t)) * s / (np.sqrt(v) / np.sqrt(1 - B2 ** t) + EPS_ADAM)
    else:
        s = MOM * s + g
        p = p - LR * (g + MOM * s)
    return {"p": p, "s": s, "v": v, "g": g, "raw": raw, "coef": coef, "total": total}


CASES = [(1, 1), (37, 3), (1000, 8), (3075, 1), (3075, 8), (37, 1), (1000, 1)]


@pytest.mark.parametrize("K,nsplit", CASES)
@pytest.mark.parametrize("algo", [L.OPTIM_ADAGRAD, L.OPTIM_ADAM, L.OPTIM_SGD])
@pytest.mark.parametrize("max_norm,wd,decay_w", [(5.0, 0.0, False), (0.05, 0.0, False), (0.0, 0.0, False), (0.05, 1e-2, True),
                                                 (5.0, 1e-2, False)])
def test_last_layer_step_matches_fp64(K, nsplit, algo, max_norm, wd, decay_w):
    c = _case(K, nsplit, seed=K * 10 + nsplit)
    steps = [0.0, 0.0] if (K + nsplit) % 2 == 0 else [4.0, 7.0]  # Adam: the counter at zero and above
    got = _run(algo, c, K, nsplit, max_norm, wd, decay_w, steps)
    ref = _ref(algo, c, K, nsplit, max_norm, wd, decay_w, steps)
    if max_norm == 0.05:
        assert ref["coef"] < 1.0  # the clip binds
    np.testing.assert_allclose(got["norm"][0].item(), ref["coef"], rtol=1e-5)
    np.testing.assert_allclose(got["norm"][1].item(), ref["total"], rtol=1e-5)
    np.testing.assert_allclose(got["g_out"].double().numpy(), ref["g"], rtol=1e-5, atol=1e-7)
    p = torch.cat([got["w"], got["b"]]).double().numpy()
    s = torch.cat([got["s_w"], got["s_b"]]).double().numpy()
    np.testing.assert_allclose(p, ref["p"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(s, ref["s"], rtol=1e-5, atol=1e-7)
    if algo == L.OPTIM_ADAM:
        np.testing.assert_allclose(torch.cat([got["v_w"], got["v_b"]]).double().numpy(), ref["v"], rtol=1e-5, atol=1e-9)
    if nsplit > 1:  # the summed partials land where the reduce launch would have put them
        np.testing.assert_allclose(torch.cat([got["dw"], got["dbias"]]).double().numpy(), ref["raw"], rtol=1e-5, atol=1e-6)
    if algo == L.OPTIM_ADAGRAD:
        assert got["step"].tolist() == steps
    else:
        assert got["step"].tolist() == [steps[0] + 1, steps[1] + 1]
    again = _run(algo, c, K, nsplit, max_norm, wd, decay_w, steps)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_last_layer_step_refuses_bad_descriptors():
    c = _case(8, 1, 0)
    with pytest.raises(L.EngineError):
        _run(L.OPTIM_ADAGRAD, c, L.LAST_LAYER_MAX, 1, 5.0, 0.0, False, [0.0, 0.0])
    with pytest.raises(L.EngineError):
        _run(7, c, 8, 1, 5.0, 0.0, False, [0.0, 0.0])
