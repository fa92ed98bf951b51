"""Row-sparse ("lazy") Adam over a whole model: torch.optim.Adam on the dense parameters, torch.optim.SparseAdam on the embedding tables.

A table moves only in the rows whose ids are in the batch — weights and both moments — and every other row keeps its bits: what
recommendation models with tables of 10^7 rows train with.  The tables' gradients stay dense tensors (nn.Embedding(sparse=False), as the
reference builds them), so the optimizer cannot see which rows the batch touched: the training loop tells it (`touch`).  A touched row
whose summed gradient is exactly zero still decays its moments and moves, as a row of a coalesced sparse gradient does.

`step()` is the torch route; the fused engine step reproduces it (OptimSpec.sparse_rows, csrc/optim_moments.hip) and shares its state
through SuperNet.engine_bind_optimizer, as with torch.optim.Adam.

RowwiseSparseAdam is the same optimizer with one second-moment float per table row (`--optimizer rowwise-adam`)."""
import contextlib
import math
from typing import Iterable

import numpy as np
import torch
from torch.optim.adam import adam as _adam


class RowSparseAdam(torch.optim.Optimizer):
    """params: every parameter of the model, the tables included; table_params: the tables, table f first ... (model._embedding's
    parameters in order): column f of the ids given to `touch` belongs to table_params[f].  One param group with torch.optim.Adam's
    keys; state per parameter: step, exp_avg, exp_avg_sq (Adam's key set: a checkpoint has Adam's shape)."""

    def __init__(self, params, table_params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("RowSparseAdam: lr %r, betas %r, eps %r" % (lr, betas, eps))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, capturable=False,
                        differentiable=False, fused=None)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("RowSparseAdam keeps one param group")
        self._tables = list(table_params)
        own = {id(p) for p in self.param_groups[0]["params"]}
        if not all(id(t) in own for t in self._tables):
            raise ValueError("RowSparseAdam: every table must be one of params")
        self._table_index = {id(t): f for f, t in enumerate(self._tables)}
        self._ids = None

    def touch(self, cat_feats: torch.Tensor):
        """the ids [B, Fs] of the batch whose gradients the next step() applies: column f = the rows of table f it touches.  In a
        process group of several ranks the torch route averages the tables' dense gradients over the ranks, so the touched rows are
        those of every rank's batch: the ids are gathered (a collective: every rank calls touch)."""
        if cat_feats.dim() != 2 or cat_feats.shape[1] != len(self._tables):
            raise ValueError("touch: ids of shape [B, %d] expected, got %s" % (len(self._tables), tuple(cat_feats.shape)))
        ids = cat_feats.detach().long()
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            parts = [torch.empty_like(ids) for _ in range(dist.get_world_size())]
            dist.all_gather(parts, ids.contiguous())
            ids = torch.cat(parts)
        # an id must name a row of its table: a row-sharded table (SuperNet(table_sharding="row")) holds one rank's rows under local
        # ids, which the batch's global ids do not address (one comparison on the device, one flag read back per step)
        sizes = torch.tensor([t.shape[0] for t in self._tables], device=ids.device)
        if ids.numel() and bool(((ids < 0) | (ids >= sizes)).any()):
            raise ValueError("touch: an id lies outside its table (%s rows): RowSparseAdam needs whole tables under the batch's ids, "
                             "not row-sharded ones" % [int(t.shape[0]) for t in self._tables])
        self._ids = ids

    RULE = "element-wise"  # the second moment's form on a table: one per element here, one per row in RowwiseSparseAdam

    def _second_moment_shape(self, p):
        """shape of exp_avg_sq of parameter p under this optimizer's rule"""
        return tuple(p.shape)

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if self._second_moment_shape(p) == tuple(p.shape):
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            else:
                st["exp_avg_sq"] = torch.zeros(self._second_moment_shape(p), dtype=p.dtype, device=p.device)
        return st

    def load_state_dict(self, state_dict):
        """torch's, after a check that changes nothing: every table's exp_avg_sq in the checkpoint must have this rule's shape — a
        RowwiseSparseAdam checkpoint ([rows]) under RowSparseAdam ([rows, width]), or the reverse, is refused (ValueError), never
        reshaped or broadcast"""
        groups = state_dict.get("param_groups") or [{}]
        ids = groups[0].get("params", []) if len(groups) == 1 else []
        for k, p in zip(ids, self.param_groups[0]["params"]):
            st = state_dict.get("state", {}).get(k)
            if id(p) in self._table_index and st and "exp_avg_sq" in st and tuple(st["exp_avg_sq"].shape) != self._second_moment_shape(p):
                raise ValueError("%s.load_state_dict: exp_avg_sq of a table of shape %s has shape %s; this optimizer keeps the %s second "
                                 "moment %s (a checkpoint of %s?)"
                                 % (type(self).__name__, tuple(p.shape), tuple(st["exp_avg_sq"].shape), self.RULE,
                                    self._second_moment_shape(p), "RowSparseAdam" if self.RULE == "row-wise" else "RowwiseSparseAdam"))
        super().load_state_dict(state_dict)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        beta1, beta2 = group["betas"]
        lr, eps = group["lr"], group["eps"]
        dense = ([], [], [], [], [])
        tables = []
        for p in group["params"]:
            if p.grad is None:
                continue  # (a parameter the sampled path does not reach; a table when the backward stops short of the stem)
            if p.grad.is_sparse:
                raise RuntimeError("RowSparseAdam reads dense gradients (nn.Embedding(sparse=False)) and the ids of touch()")
            st = self._init_state(p)
            if id(p) in self._table_index:
                tables.append((p, st))
                continue
            for lst, v in zip(dense, (p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"])):
                lst.append(v)
        if tables and self._ids is None:
            raise RuntimeError("RowSparseAdam.step: a table has a gradient and no ids were given since the last step: call "
                               "optimizer.touch(cat_feats) before step() (touched rows are never guessed from non-zero gradients)")
        if dense[0]:
            # torch.optim.Adam itself, per-parameter step counters included
            _adam(dense[0], dense[1], dense[2], dense[3], [], dense[4], amsgrad=False, beta1=beta1, beta2=beta2, lr=lr, weight_decay=0,
                  eps=eps, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None, has_complex=False)
        for p, st in tables:
            st["step"] += 1
            rows = torch.unique(self._ids[:, self._table_index[id(p)]]).to(p.device)
            self._update_rows(p, st, rows, float(st["step"]), lr, beta1, beta2, eps)
        self._ids = None  # consumed: the next gradients need their own ids
        return loss

    def _update_rows(self, p, st, rows, t, lr, beta1, beta2, eps):
        """torch.optim.SparseAdam on the rows of the batch (torch/optim/_functional.py sparse_adam, statement by statement)"""
        g = p.grad.index_select(0, rows)
        m_old, v_old = st["exp_avg"].index_select(0, rows), st["exp_avg_sq"].index_select(0, rows)
        m_upd = g.sub(m_old).mul_(1 - beta1)
        v_upd = g.pow(2).sub_(v_old).mul_(1 - beta2)
        numer = m_upd.add(m_old)
        v_new = v_upd.add(v_old)
        st["exp_avg"].index_copy_(0, rows, numer)
        st["exp_avg_sq"].index_copy_(0, rows, v_new)
        denom = v_new.sqrt().add_(eps)
        step_size = lr * math.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
        p.index_add_(0, rows, numer.div(denom).mul_(-step_size))


class RowwiseSparseAdam(RowSparseAdam):
    """`--optimizer rowwise-adam`: RowSparseAdam with ONE second moment per embedding row ("partial row-wise Adam") — torch.optim.Adam
    on the dense parameters; on a table the first moment stays per element and `exp_avg_sq` has shape [rows], fed the mean of the
    row's squared gradient, and divides the whole row.  A row r whose id is in the batch, g = its summed, clipped gradient, zero or not:

        m[r] += (g - m[r]) * (1 - beta1)
        v[r] += ((g * g).mean() - v[r]) * (1 - beta2)
        p[r] -= lr * sqrt(1 - beta2^t) / (1 - beta1^t) * m[r] / (sqrt(v[r]) + eps)         t = the table's step count after this step

    — the order of statements and the step size of RowSparseAdam.  A row outside the batch keeps its bits in p, m and v.  At embedding
    width 16 the tables' optimizer state is 17/32 of RowSparseAdam's.  Same constructor, `touch()` protocol and param-group keys; a
    table must be 2-D, and a checkpoint of the other form is refused by either class (load_state_dict): nothing broadcasts silently.

    `step()` is the torch route, on any device; the fused engine step reproduces it (OptimSpec.table_kind "rowwise_adam",
    csrc/optim_moments.hip RowwiseSparseAdamRows) and shares its state through SuperNet.engine_bind_optimizer."""

    RULE = "row-wise"

    def __init__(self, params, table_params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        table_params = list(table_params)
        for t in table_params:
            if t.dim() != 2:
                raise ValueError("RowwiseSparseAdam: the row-wise second moment needs 2-D tables [rows, width], got shape %s" % (tuple(t.shape),))
        super().__init__(params, table_params, lr=lr, betas=betas, eps=eps)

    def _second_moment_shape(self, p):
        return (p.shape[0],) if id(p) in self._table_index else tuple(p.shape)

    def _update_rows(self, p, st, rows, t, lr, beta1, beta2, eps):
        """RowSparseAdam's statements with the row's mean squared gradient in place of g^2 and one denominator per row"""
        if tuple(st["exp_avg_sq"].shape) != (p.shape[0],):
            raise ValueError("RowwiseSparseAdam: exp_avg_sq of a table of shape %s has shape %s, the row-wise rule keeps %s (a checkpoint "
                             "of RowSparseAdam?)" % (tuple(p.shape), tuple(st["exp_avg_sq"].shape), (p.shape[0],)))
        g = p.grad.index_select(0, rows)
        m_old, v_old = st["exp_avg"].index_select(0, rows), st["exp_avg_sq"].index_select(0, rows)
        m_upd = g.sub(m_old).mul_(1 - beta1)
        v_upd = (g * g).mean(dim=1).sub_(v_old).mul_(1 - beta2)
        numer = m_upd.add(m_old)
        v_new = v_upd.add(v_old)
        st["exp_avg"].index_copy_(0, rows, numer)
        st["exp_avg_sq"].index_copy_(0, rows, v_new)
        denom = v_new.sqrt().add_(eps)
        step_size = lr * math.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
        p.index_add_(0, rows, numer.div(denom.unsqueeze(1)).mul_(-step_size))


_SR_T, _SR_F = 0x9E3779B9, 0x85EBCA6B  # the odd constants that spread the step count and the table index over 32 bits
_M32 = 0xFFFFFFFF


def _sr_mix(h: torch.Tensor) -> torch.Tensor:
    """one 32-bit avalanche round (xorshift-multiply, 0x7feb352d / 0x846ca68b) on int64 tensors holding values below 2^32; a product
    wraps modulo 2^64, which leaves its low 32 bits right, and is masked before the next shift"""
    h = h ^ (h >> 16)
    h = (h * 0x7feb352d) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x846ca68b) & _M32
    return h ^ (h >> 16)


def stochastic_round_bits(seed: int, step: int, table: int, row_ids: torch.Tensor, width: int = 16) -> torch.Tensor:
    """r [n, width] (int64, 0 .. 65535): the 16 uniform bits of stochastic_round_bf16 for element e of row row_ids[i] of table `table`
    at step `step` — the top half of mix(mix(mix(seed32 ^ step * 0x9E3779B9) ^ table * 0x85EBCA6B) ^ (row * 16 + e)), all in 32-bit
    arithmetic (row * 16 + e wraps), seed32 = the seed's two halves xor-ed.  A counter hash: nothing is carried from call to call."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seed32 = (seed ^ (seed >> 32)) & _M32
    head = torch.tensor(seed32 ^ ((int(step) * _SR_T) & _M32), dtype=torch.int64)
    head = _sr_mix(_sr_mix(head) ^ ((int(table) * _SR_F) & _M32))
    rows = torch.as_tensor(row_ids).to(torch.int64).cpu().reshape(-1, 1)
    pos = (rows * 16 + torch.arange(width, dtype=torch.int64)) & _M32
    return _sr_mix(head ^ pos) >> 16


def stochastic_round_bf16(x_fp32: torch.Tensor, seed: int, step: int, table: int, row_ids: torch.Tensor) -> torch.Tensor:
    """THE definition of how a bf16 embedding table stores an fp32 weight (csrc/optim_moments.hip RowwiseAdagradBf16TableRows matches
    it bit for bit): x_fp32 [n, 16] = the new weights of rows row_ids [n] of table `table`, step = that table's step count AFTER the
    step that produced them -> bfloat16 [n, 16],
        out16 = (bits(x) + r) >> 16,   r = stochastic_round_bits(seed, step, table, row_ids)
    so x moves up to the next bf16 with probability (low 16 bits of x) / 65536 and down otherwise: unbiased.  A value that already is
    a bf16 (low bits 0) never moves; a non-finite x is stored truncated (r = 0); the largest finite values may carry into inf, which
    is the overflow rounding up means.  Pure integer torch ops, on the CPU."""
    x = x_fp32.detach().to(torch.float32).cpu().contiguous()
    if x.dim() != 2 or x.shape[1] != 16:
        raise ValueError("stochastic_round_bf16: rows of 16 floats expected, got shape %s" % (tuple(x.shape),))
    bits = x.view(torch.int32).to(torch.int64) & _M32
    r = stochastic_round_bits(seed, step, table, row_ids, 16)
    if tuple(r.shape) != tuple(bits.shape):
        raise ValueError("stochastic_round_bf16: %d row ids for %d rows" % (r.shape[0], bits.shape[0]))
    finite = (bits & 0x7F800000) != 0x7F800000
    out = ((bits + torch.where(finite, r, torch.zeros_like(r))) >> 16) & 0xFFFF
    return ((out ^ 0x8000) - 0x8000).to(torch.int16).view(torch.bfloat16)  # (the 16 bits as a signed word, then reinterpreted)


class AdamAdagradTables(torch.optim.Optimizer):
    """`--optimizer adam-adagrad-tables`: torch.optim.Adam on the dense parameters, torch.optim.Adagrad on the embedding tables with
    their own learning rate `lr * table_lr_scale` and `table_eps` — how recommendation models are usually trained.  Adagrad with a
    zero gradient changes neither the accumulator nor the weight (`0 / (sqrt(sum) + table_eps)` is an exact zero: table_eps > 0), so
    the dense statements are already exactly row-sparse: no ids, no `touch`, no catch-up.

    params: every parameter of the model, the tables included; table_params: the tables.  ONE param group — Adam's keys plus
    table_lr_scale and table_eps — so a scheduler that publishes one lr moves both halves together.  State: step, exp_avg, exp_avg_sq
    on a dense parameter (Adam's), step, sum on a table (Adagrad's).

    table_rowwise: row-wise Adagrad on the tables (the "exact row-wise Adagrad" of DLRM-style trainers) — `sum` has shape [rows], one
    accumulator per embedding row, fed the mean of the row's squared gradient, and divides the whole row:
        sum += (g * g).mean(dim=1);  W -= table_lr * g / (sqrt(sum) + table_eps)[:, None]
    As exactly row-sparse as the element-wise form, with 1/16 of its state at embedding width 16.  A table must be 2-D, and a `sum`
    of the other form's shape (a checkpoint of the other rule) is refused: nothing broadcasts silently.

    Tables of dtype bfloat16 (SuperNet(table_dtype=torch.bfloat16)) are accepted with table_rowwise only; their `sum` is fp32 [rows],
    created here, and `table_seed` — the seed of the stochastic rounding their new weights are stored with (stochastic_round_bf16) —
    sits in the param group, so a checkpoint carries it.  They train on the fused step alone: `step()` raises, because autograd would
    hand it a dense bf16 gradient the size of the table, which is neither that rule nor affordable.

    `step()` is the torch route, on any device; the fused engine step reproduces it (OptimSpec.table_kind, csrc/optim_moments.hip)
    and shares its state through SuperNet.engine_bind_optimizer."""

    def __init__(self, params, table_params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 table_lr_scale: float = 1.0, table_eps: float = 1e-2, table_rowwise: bool = False, table_seed: int = 0):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("AdamAdagradTables: lr %r, betas %r, eps %r" % (lr, betas, eps))
        if not table_eps > 0.0:
            raise ValueError("AdamAdagradTables: table_eps %r is not positive (a row with a zero gradient must stay where it is)" % (table_eps,))
        if not table_lr_scale > 0.0:
            raise ValueError("AdamAdagradTables: table_lr_scale %r is not positive" % (table_lr_scale,))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, capturable=False,
                        differentiable=False, fused=None, table_lr_scale=table_lr_scale, table_eps=table_eps,
                        table_rowwise=bool(table_rowwise), table_seed=int(table_seed))
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("AdamAdagradTables keeps one param group")
        tables = list(table_params)
        own = {id(p) for p in self.param_groups[0]["params"]}
        if not all(id(t) in own for t in tables):
            raise ValueError("AdamAdagradTables: every table must be one of params")
        self._table_ids = {id(t) for t in tables}
        if table_rowwise:
            for t in tables:
                if t.dim() != 2:
                    raise ValueError("AdamAdagradTables: table_rowwise needs 2-D tables [rows, width], got shape %s" % (tuple(t.shape),))
        self._bf16_tables = [t for t in tables if t.dtype == torch.bfloat16]
        if self._bf16_tables and not table_rowwise:
            raise ValueError("AdamAdagradTables: bf16 tables take the row-wise rule only (table_rowwise=True): element-wise Adagrad on "
                             "bf16 tables is not built")
        if self._bf16_tables and len(self._bf16_tables) != len(tables):
            raise ValueError("AdamAdagradTables: the tables are bf16 or fp32, not a mixture")
        for t in self._bf16_tables:  # (no step() will: the fused step's binding finds the state and shares it)
            self.state[t] = {"step": torch.tensor(0.0, dtype=torch.float32), "sum": self._new_sum(t, True)}

    @property
    def bf16_tables(self) -> bool:
        """the tables are stored as bfloat16: the fused step is the only route (OptimSpec.table_kind "rowwise_adagrad_bf16")"""
        return bool(self._bf16_tables)

    @staticmethod
    def _new_sum(p, rowwise):
        """a table's zero accumulator: [rows] under the row-wise rule, else the table's shape; fp32 where the table is bf16"""
        dt = torch.float32 if p.dtype == torch.bfloat16 else p.dtype
        if rowwise and p.dim() == 2:
            return torch.zeros(p.shape[0], dtype=dt, device=p.device)
        return torch.zeros_like(p, dtype=dt, memory_format=torch.preserve_format)

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:
            g.setdefault("table_rowwise", False)  # (a pickle from before the flag)
            g.setdefault("table_seed", 0)

    def load_state_dict(self, state_dict):
        """torch's, after a check that changes nothing: the checkpoint's rule (its group's table_rowwise; absent = element-wise) and
        the shape of every table's `sum` must be this optimizer's — an element-wise state under table_rowwise, or the reverse, is
        refused (ValueError), never reshaped or broadcast"""
        rowwise = bool(self.param_groups[0].get("table_rowwise", False))
        groups = state_dict.get("param_groups") or [{}]
        if len(groups) == 1 and bool(groups[0].get("table_rowwise", False)) != rowwise:
            raise ValueError("AdamAdagradTables.load_state_dict: the checkpoint was written with table_rowwise=%r, this optimizer was built "
                             "with table_rowwise=%r" % (bool(groups[0].get("table_rowwise", False)), rowwise))
        ids = groups[0].get("params", []) if len(groups) == 1 else []
        for k, p in zip(ids, self.param_groups[0]["params"]):
            st = state_dict.get("state", {}).get(k)
            if id(p) in self._table_ids and st and "sum" in st and tuple(st["sum"].shape) != self._sum_shape(p, rowwise):
                raise ValueError("AdamAdagradTables.load_state_dict: `sum` of a table of shape %s has shape %s, table_rowwise=%r keeps %s"
                                 % (tuple(p.shape), tuple(st["sum"].shape), rowwise, self._sum_shape(p, rowwise)))
        super().load_state_dict(state_dict)
        # (torch casts a floating-point parameter's state to the parameter's dtype: a bf16 table's `sum` is fp32 and stays so)
        for k, p in zip(ids, self.param_groups[0]["params"]):
            st = state_dict.get("state", {}).get(k)
            if p.dtype == torch.bfloat16 and id(p) in self._table_ids and st and "sum" in st:
                self.state[p]["sum"] = st["sum"].detach().to(device=p.device, dtype=torch.float32).clone()

    @staticmethod
    def _sum_shape(p, rowwise):
        if rowwise and p.dim() != 2:
            raise ValueError("AdamAdagradTables: table_rowwise needs 2-D tables [rows, width], got shape %s" % (tuple(p.shape),))
        return (p.shape[0],) if rowwise else tuple(p.shape)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._bf16_tables:
            raise RuntimeError("AdamAdagradTables.step: bf16 tables train on the fused step only (SuperNet.engine_train_step): autograd "
                               "would hand this step a dense bf16 gradient the size of a table, which is neither the rule "
                               "(fp32 row-wise Adagrad, stored with stochastic rounding) nor affordable")
        group = self.param_groups[0]
        beta1, beta2 = group["betas"]
        lr, eps = group["lr"], group["eps"]
        table_lr, table_eps = lr * group["table_lr_scale"], group["table_eps"]
        rowwise = bool(group.get("table_rowwise", False))
        dense = ([], [], [], [], [])
        for p in group["params"]:
            if p.grad is None:
                continue  # (a parameter the sampled path does not reach; a table when the backward stops short of the stem)
            if p.grad.is_sparse:
                raise RuntimeError("AdamAdagradTables reads dense gradients (nn.Embedding(sparse=False))")
            st = self.state[p]
            if id(p) in self._table_ids:
                # torch.optim.Adagrad's dense single-tensor statements (torch/optim/adagrad.py), lr_decay 0 and weight_decay 0
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["sum"] = self._new_sum(p, rowwise)
                if tuple(st["sum"].shape) != self._sum_shape(p, rowwise):
                    raise ValueError("AdamAdagradTables: `sum` of a table of shape %s has shape %s, table_rowwise=%r keeps %s (a checkpoint "
                                     "of the other rule?)" % (tuple(p.shape), tuple(st["sum"].shape), rowwise, self._sum_shape(p, rowwise)))
                st["step"] += 1
                if rowwise:
                    g = p.grad
                    msq = (g * g).mean(dim=1)
                    st["sum"].add_(msq)
                    std = st["sum"].sqrt().add_(table_eps)
                    p.addcdiv_(g, std.unsqueeze(1), value=-table_lr)
                    continue
                st["sum"].addcmul_(p.grad, p.grad, value=1)
                std = st["sum"].sqrt().add_(table_eps)
                p.addcdiv_(p.grad, std, value=-table_lr)
                continue
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            for lst, v in zip(dense, (p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"])):
                lst.append(v)
        if dense[0]:
            # torch.optim.Adam itself, per-parameter step counters included
            _adam(dense[0], dense[1], dense[2], dense[3], [], dense[4], amsgrad=False, beta1=beta1, beta2=beta2, lr=lr, weight_decay=0,
                  eps=eps, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None, has_complex=False)
        return loss


class LazyRMSprop(torch.optim.RMSprop):
    """`--optimizer rmsprop`: torch.optim.RMSprop, and on the torch route exactly that.  The type is what the fused engine step looks for
    (OptimSpec.from_optimizer: momentum 0, not centered): there a table row outside the batch owes `square_avg` only a factor
    alpha^n, which the engine pays when the row is next touched, or when somebody reads the state ("Lazy RMSprop").  Bound
    to an engine (SuperNet.engine_bind_optimizer) the optimizer carries a flush hook that brings every row current; `step()` and
    `state_dict()` call it first, so whoever reads or advances the aliased `square_avg` sees torch.optim.RMSprop's state."""

    _lazy_flush = None  # (set by SuperNet.engine_bind_optimizer; never part of a checkpoint)

    def flush_lazy_rows(self):
        if self._lazy_flush is not None:
            self._lazy_flush()

    def step(self, closure=None):
        self.flush_lazy_rows()
        return super().step(closure)

    def state_dict(self):
        self.flush_lazy_rows()
        return super().state_dict()


class WeightEMA:
    """`--ema DECAY`: an exponential moving average of every parameter of `model` (parameters only: no buffer of the model trains),
    0 < decay < 1.  `shadow[name]` starts as a copy of the parameter; `update()`, called after every optimizer step that was taken,
    averages every parameter whether or not it had a gradient, in fp32 with w = (float)(1 - decay):

        s = s + w (p - s)        torch: `s.add_(p - s, alpha=w)`, one statement per tensor

    No warm-up, no bias correction, no decay that depends on `num_updates`.  The fused engine step (SuperNet.engine_train_step(...,
    ema_decay=)) computes `fmaf(w, p - s, s)` and pays the resting table rows in closed form (csrc/weight_ema.hip); it is checked
    against this rule in fp64, not against torch's bits.  Bound to an engine (SuperNet.engine_bind_ema) the shadows alias the engine's
    arrays and `state_dict()` / `averaged()` bring every row current first."""

    def __init__(self, model, decay: float):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("WeightEMA: decay %r is not inside (0, 1)" % (decay,))
        self.model, self.decay = model, decay
        self.shadow = {n: p.detach().clone() for n, p in model.named_parameters()}
        self.num_updates = 0
        self._swapped = False
        self._hooks = None  # (set by SuperNet.engine_bind_ema; never part of a checkpoint)

    @property
    def weight(self) -> float:
        """w = (float)(1 - decay) as a Python float"""
        return float(np.float32(1.0 - self.decay))

    @torch.no_grad()
    def update(self):
        if self._swapped:
            raise RuntimeError("WeightEMA.update() inside averaged(): the parameters hold the average")
        if self._hooks is not None:
            self._hooks["flush"]()
        w = self.weight
        for n, p in self.model.named_parameters():
            s = self.shadow[n]
            s.add_(p.detach().to(s.device) - s, alpha=w)
        if self._hooks is not None:
            self._hooks["advance"]()
        self.num_updates += 1

    @torch.no_grad()
    def _exchange(self):
        if self._hooks is not None:
            self._hooks["swap"]()  # (flush + exchange, one launch)
            return
        for n, p in self.model.named_parameters():
            s = self.shadow[n]
            tmp = p.detach().clone()
            p.copy_(s.to(p.device))
            s.copy_(tmp.to(s.device))

    @contextlib.contextmanager
    def averaged(self):
        """inside, the model's parameters hold the averaged values and the shadow holds the parameters; on exit both are back, bit for
        bit.  update() and a fused training step raise inside."""
        if self._swapped:
            raise RuntimeError("WeightEMA.averaged() is not re-entrant")
        self._exchange()
        self._swapped = True
        try:
            yield self.model
        finally:
            self._exchange()
            self._swapped = False

    def state_dict(self):
        if self._swapped:
            raise RuntimeError("WeightEMA.state_dict() inside averaged()")
        if self._hooks is not None:
            self._hooks["flush"]()
        return {"decay": self.decay, "num_updates": int(self.num_updates), "shadow": {n: s.detach().clone() for n, s in self.shadow.items()}}

    @torch.no_grad()
    def load_state_dict(self, state):
        if set(state["shadow"]) != set(self.shadow):
            raise KeyError("WeightEMA.load_state_dict: parameter names differ")
        if self._hooks is not None:
            raise RuntimeError("WeightEMA.load_state_dict on a bound average: load first, then SuperNet.engine_bind_ema")
        self.decay, self.num_updates = float(state["decay"]), int(state["num_updates"])
        for n, s in self.shadow.items():
            s.copy_(state["shadow"][n].to(s.device))


class DecoupledWeightDecay:
    """`--decoupled-wd LAMBDA`: decoupled weight decay beside any optimizer, the "W" of torch.optim.AdamW.  `apply(lr)`, called
    immediately before `optimizer.step()` (after clipping and `optimizer.touch`), runs torch.optim.AdamW's statement

        p.mul_(1 - lr * weight_decay)

    on every SELECTED parameter that has a gradient this step; a parameter whose grad is None is skipped exactly as AdamW skips it (a
    supernet parameter off the sampled path; a table in a step whose backward stops short of the stem).  Selected is get_l2_loss's
    rule: at least 2 dimensions and a name that does not start with `no_reg_param_name`.  No state: nothing goes into a checkpoint.

    The fused engine step (SuperNet.engine_train_step(..., decoupled_wd=)) multiplies the dense parameters and the batch's table rows
    and lets every other row rest; a resting row owes the product of the factors it missed, paid when it is next touched or read
    (csrc/decoupled_decay.hip).  Between fused steps the table tensors therefore hold rows that still owe their decay: a RAW read of
    `_embedding.<f>.weight` needs `SuperNet.engine_flush_decay()` first.  `SuperNet.forward`, `SuperNet.state_dict`,
    `engine_sync_optimizer_steps`, the end of train_and_test_one_epoch and `apply` of a bound helper (SuperNet.engine_bind_decay) flush
    by themselves."""

    def __init__(self, model, weight_decay: float, no_reg_param_name=None):
        weight_decay = float(weight_decay)
        if not weight_decay >= 0.0:
            raise ValueError("DecoupledWeightDecay: weight_decay %r is negative" % (weight_decay,))
        self.model, self.weight_decay, self.no_reg_param_name = model, weight_decay, no_reg_param_name
        self._flush = None  # (set by SuperNet.engine_bind_decay: pays what the fused steps left owing; never part of a checkpoint)

    def selected(self):
        """[(name, parameter)] the decay covers: get_l2_loss's rule"""
        skip = self.no_reg_param_name
        return [(n, p) for n, p in self.model.named_parameters() if p.dim() >= 2 and not (skip is not None and n.startswith(skip))]

    @torch.no_grad()
    def apply(self, lr: float):
        if not self.weight_decay:
            return
        lr = float(lr)
        if not lr * self.weight_decay < 1.0:
            raise ValueError("DecoupledWeightDecay: lr %r x weight_decay %r is not below 1" % (lr, self.weight_decay))
        if self._flush is not None:
            self._flush()
        for _, p in self.selected():
            if p.grad is not None:
                p.mul_(1 - lr * self.weight_decay)


def parse_cowclip(text):
    """`--cowclip R[,ZETA]` -> (r, zeta), or None for an absent flag (None / ""); ZETA defaults to 1e-5.  r >= 0 and zeta > 0, both
    finite: anything else is a ValueError that names the flag."""
    if text is None or text == "":
        return None
    if isinstance(text, (tuple, list)):
        parts = [str(v) for v in text]
    else:
        parts = str(text).split(",")
    try:
        if not 1 <= len(parts) <= 2:
            raise ValueError
        r = float(parts[0])
        zeta = float(parts[1]) if len(parts) == 2 else 1e-5
    except ValueError:
        raise ValueError("--cowclip takes R or R,ZETA (two numbers), got %r" % (text,)) from None
    if not (math.isfinite(r) and r >= 0.0):
        raise ValueError("--cowclip: R = %r must be a finite number >= 0" % (r,))
    if not (math.isfinite(zeta) and zeta > 0.0):
        raise ValueError("--cowclip: ZETA = %r must be a finite number > 0" % (zeta,))
    return r, zeta


class CowClip:
    """`--cowclip R[,ZETA]`: CowClip (Zheng et al., "CowClip: Reducing CTR Prediction Model Training Time from 12 hours to 10 minutes on
    1 GPU", AAAI 2023), per-row adaptive gradient clipping of the embedding tables — what lets the batch grow: a frequent id receives
    the sum of many per-sample gradients, a rare id one, and a single global clip cannot serve both.

    `apply(cat_x)`, called after `clip_grad_norm_` and `DecoupledWeightDecay.apply`, before `optimizer.step()` (beside
    `optimizer.touch(cat_x)`), rescales rows of the tables' dense `.grad` (which already carries the global clip coefficient).  For
    table f and every in-range id k of column f of the batch, with cnt = how often k occurs there, in fp32:

        G = sqrt(sum(grad[k]^2));  T = cnt * max(r * sqrt(sum(w[k]^2)), zeta);  if G > T: grad[k] *= T / G

    A zero or NaN gradient row is never clipped (the comparison is false), ids outside the table are skipped, no other row is read or
    written.  No state beyond two counters (rows touched, rows clipped): nothing goes into a checkpoint.

    This is the definition the fused engine step is held to (SuperNet.engine_train_step(..., cowclip=(r, zeta)); csrc/cowclip.hip),
    which scales the summed gradient rows in front of the optimizer's launch, whatever rule the tables take."""

    def __init__(self, tables: Iterable[torch.Tensor], r: float = 1.0, zeta: float = 1e-5):
        self.r, self.zeta = parse_cowclip((r, zeta))
        self.tables = list(tables)
        self.touched = self.clipped = 0

    def rows(self, cat_x: torch.Tensor, f: int):
        """(unique in-range ids of column f, their counts)"""
        ids = cat_x[:, f].detach().long()
        ids = ids[(ids >= 0) & (ids < self.tables[f].shape[0])]
        return torch.unique(ids, return_counts=True)

    @torch.no_grad()
    def apply(self, cat_x: torch.Tensor):
        """-> (rows touched, rows clipped) of this batch; a table whose grad is None (a backward that stops short of the stem) is skipped"""
        if cat_x.dim() != 2 or cat_x.shape[1] != len(self.tables):
            raise ValueError("CowClip.apply: ids of shape [B, %d] expected, got %s" % (len(self.tables), tuple(cat_x.shape)))
        touched = clipped = 0
        for f, w in enumerate(self.tables):
            if w.grad is None:
                continue
            ids, cnt = self.rows(cat_x.to(w.device), f)
            if not ids.numel():
                continue
            g = w.grad[ids].float()
            G = g.square().sum(1).sqrt()
            T = cnt.float() * torch.fmax(self.r * w[ids].float().square().sum(1).sqrt(), torch.tensor(self.zeta, dtype=torch.float32, device=w.device))
            clip = G > T
            scale = torch.where(clip, T / G, torch.ones_like(G))
            sel = ids[clip]
            if sel.numel():
                w.grad[sel] = (g[clip] * scale[clip, None]).to(w.grad.dtype)
            touched += int(ids.numel())
            clipped += int(clip.sum())
        self.touched += touched
        self.clipped += clipped
        return touched, clipped
