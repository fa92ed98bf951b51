"""Evaluation metrics on the device.

`roc_auc_score(y_true, y_score)` is `sklearn.metrics.roc_auc_score` for binary labels and float32 scores, computed by the engine's
NASREC_OP_ROC_AUC (csrc/roc_auc.hip) on the scores' GPU and equal to sklearn's float64 bit for bit (DESIGN.md "ROC AUC on the device").  The
launch chain runs on the current stream; reading back the 12-byte result is the one synchronisation.  Whatever sklearn does not
score as a plain binary AUC (fewer than two samples, a label other than 0 / 1, one class only, a score that is not finite) comes
back as a non-zero status, and then sklearn itself runs on host copies, so it raises or warns exactly as it always did."""
import ctypes as C
import struct

import sklearn.metrics
import torch

from . import _lib as L

ROC_AUC_MAX_N = L.ROC_AUC_MAX_N


def roc_auc_supported(y_true: torch.Tensor, y_score: torch.Tensor) -> bool:
    """True when roc_auc_score below takes these tensors: 1-D contiguous float32 of one CUDA device, equal length <= ROC_AUC_MAX_N"""
    return (y_score.is_cuda and y_true.device == y_score.device and y_true.dtype == torch.float32 and y_score.dtype == torch.float32
            and y_true.dim() == 1 and y_score.dim() == 1 and y_true.is_contiguous() and y_score.is_contiguous()
            and y_true.numel() == y_score.numel() and y_score.numel() <= ROC_AUC_MAX_N)


def _roc_auc_device(y_true: torch.Tensor, y_score: torch.Tensor):
    """-> (auc, status) of NASREC_OP_ROC_AUC: auc is sklearn's value when status == 0; otherwise status holds NASREC_ROC_AUC_* bits
    (L.ROC_AUC_TOO_FEW / _BAD_LABEL / _NOT_FINITE / _ONE_CLASS) and auc means nothing"""
    if not roc_auc_supported(y_true, y_score):
        raise ValueError("roc_auc_score takes 1-D contiguous float32 CUDA tensors of one device and equal length <= %d; got %s %s %s and "
                         "%s %s %s" % (ROC_AUC_MAX_N, tuple(y_true.shape), y_true.dtype, y_true.device, tuple(y_score.shape),
                                       y_score.dtype, y_score.device))
    lib = L.load()
    n = y_score.numel()
    with torch.cuda.device(y_score.device):
        ws_bytes = int(lib.nasrec_roc_auc_workspace_bytes(n))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=y_score.device)
        out = torch.empty(16, dtype=torch.uint8, device=y_score.device)
        d = L.RocAucDesc()
        d.kind, d.n = L.OP_ROC_AUC, n
        d.score, d.label, d.out = y_score.data_ptr(), y_true.data_ptr(), out.data_ptr()
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws_bytes
        L.check(lib.nasrec_roc_auc(torch.cuda.current_stream().cuda_stream, C.byref(d)))
        auc, status = struct.unpack("<di", out[:12].cpu().numpy().tobytes())
    return auc, status


def roc_auc_score(y_true: torch.Tensor, y_score: torch.Tensor) -> float:
    """sklearn.metrics.roc_auc_score(y_true, y_score) of 1-D CUDA tensors (float32, contiguous, one device), on that device"""
    auc, status = _roc_auc_device(y_true, y_score)
    if status != 0:
        return float(sklearn.metrics.roc_auc_score(y_true.detach().cpu().numpy(), y_score.detach().cpu().numpy()))
    return auc


__all__ = ["roc_auc_score", "roc_auc_supported", "ROC_AUC_MAX_N"]
