"""What the fused engine step needs to know about the torch optimizer it stands in for (main_train.py:150-160).

`OptimSpec.from_optimizer` answers which torch optimizers the fused step reproduces: torch.optim.Adam and torch.optim.SGD with
momentum, under the conditions listed there, in one process or in every rank of a data-parallel run with whole tables
(nasrec_amd/parallel.py).  Adagrad keeps its own checks (utils/train_utils.py: _fused_step_applies)."""
from typing import NamedTuple, Optional

import torch


class OptimSpec(NamedTuple):
    kind: str               # "adam" | "sgd"
    beta1: float = 0.9      # Adam
    beta2: float = 0.999
    eps: float = 1e-8
    momentum: float = 0.0   # SGD
    nesterov: bool = False

    @property
    def state_keys(self):
        """the per-parameter moment tensors torch keeps in optimizer.state[p] (besides Adam's "step")"""
        return ("exp_avg", "exp_avg_sq") if self.kind == "adam" else ("momentum_buffer",)

    @staticmethod
    def from_optimizer(optimizer) -> Optional["OptimSpec"]:
        """the spec of a torch.optim.Adam / torch.optim.SGD the fused step reproduces, else None.
        Adam: one group, amsgrad, weight_decay, maximize, capturable, differentiable and fused all off.
        SGD: one group, momentum != 0 (plain SGD keeps the torch route), dampening 0, weight_decay 0, not maximize / differentiable / fused."""
        if len(optimizer.param_groups) != 1:
            return None
        g = optimizer.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("maximize", False) or g.get("differentiable", False) or g.get("fused"):
            return None
        if type(optimizer) is torch.optim.Adam:
            if g.get("amsgrad", False) or g.get("capturable", False):
                return None
            b1, b2 = g["betas"]
            if torch.is_tensor(b1) or torch.is_tensor(b2):
                return None
            return OptimSpec("adam", beta1=float(b1), beta2=float(b2), eps=float(g["eps"]))
        if type(optimizer) is torch.optim.SGD:
            if g.get("dampening", 0) != 0 or not g.get("momentum", 0):
                return None
            return OptimSpec("sgd", momentum=float(g["momentum"]), nesterov=bool(g.get("nesterov", False)))
        return None
