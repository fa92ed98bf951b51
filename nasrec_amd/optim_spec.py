"""The optimizer of the fused engine step as one value: which torch optimizer it stands in for (main_train.py:150-160), that optimizer's
hyperparameters, and the weight decay of get_l2_loss, whose gradient the step folds in.

`OptimSpec.for_step` decides which torch optimizers the fused step reproduces: torch.optim.Adagrad, and torch.optim.Adam / torch.optim.SGD
with momentum / RowSparseAdam / RowwiseSparseAdam / LazyRMSprop / AdamAdagradTables (nasrec_amd/utils/optim.py) under the conditions of `from_optimizer`, in one process or in every rank of a data-parallel run with whole tables
(nasrec_amd/parallel.py).  The public entry points (SuperNet.engine_*, SupernetEngine.train_step / last_layer_step, DataParallelStep)
normalise their arguments into one spec (`of`); everything below them passes that."""
from typing import NamedTuple, Optional

import torch


class TableRule(NamedTuple):
    """One rule for an embedding-table row of the fused step, stated once: OptimSpec.table_rule finds it, and the engine, the
    data-parallel agreement check, the optimizer binding and the harness read it (its kernel-side twin: ROW_FORMS, csrc/optim_moments.hip)."""
    phrase: str                    # the rule in messages
    table_algo: Optional[int]      # NASREC_TABLE_ALGO_* of the NASREC_OP_OPT_MOMENTS descriptor; None = no such launch (Adagrad's apply launch)
    kinds: tuple = ("adam",)       # the OptimSpec.kind values (the dense parameters' rule) it goes with
    rows_only: bool = True         # the tables move in the batch's rows only
    state: str = "moments"         # the engine attribute that keeps the tables' state: moments, table_state ([rows, 16]) or table_row_state ([rows])
    rowwise: bool = False          # the second moment / the sum is ONE float per row, fed the mean of the row's squared gradient
    first_moment: bool = False     # the tables keep a first moment (exp_avg / momentum_buffer)
    bf16: bool = False             # the tables are STORED as bf16 (stochastic rounding under the seed that table_kind carries)
    dp_code: int = 0               # what data-parallel ranks compare (utils/dist.table_rule_code): ranks that differ would drift


TABLE_RULES = {  # (the four keys with a table_algo of their own are the values of OptimSpec.table_kind; bf16: in front of its ":<seed>")
    "dense": TableRule("dense Adam / momentum SGD", 0, kinds=("adam", "sgd"), rows_only=False, first_moment=True),
    "plain_adagrad": TableRule("Adagrad", None, kinds=("adagrad",), state="table_state"),
    "row_sparse_adam": TableRule("row-sparse Adam", 0, first_moment=True, dp_code=1),  # (descriptor: sparse_rows = 1)
    "lazy_rmsprop": TableRule("lazy RMSprop", 0, kinds=("rmsprop",)),
    "adagrad": TableRule("Adagrad on the tables", 1, state="table_state", dp_code=2),
    "rowwise_adagrad": TableRule("Adagrad on the tables", 3, state="table_row_state", rowwise=True, dp_code=3),
    "rowwise_adagrad_bf16": TableRule("Adagrad on the tables", 4, state="table_row_state", rowwise=True, bf16=True, dp_code=4),
    "rowwise_adam": TableRule("row-wise Adam", 5, rowwise=True, first_moment=True, dp_code=5),
}
_UNKNOWN_RULE = TableRule("an unknown table_kind", -1, kinds=(), rows_only=False, state="table_state", dp_code=-1)


class OptimSpec(NamedTuple):
    kind: str               # "adagrad" | "adam" | "sgd" | "rmsprop" (with table_kind: the dense parameters' rule)
    beta1: float = 0.9      # Adam
    beta2: float = 0.999
    eps: float = 1e-8       # Adam's / RMSprop's, or Adagrad's
    momentum: float = 0.0   # SGD
    nesterov: bool = False
    wd: float = 0.0         # get_l2_loss(model, wd, no_reg): the step minimises BCE + that term
    no_reg: Optional[str] = None
    sparse_rows: bool = False  # Adam: row-sparse on the tables (utils/optim.RowSparseAdam: torch.optim.SparseAdam on the batch's rows)
    alpha: float = 0.99     # RMSprop's smoothing constant (utils/optim.LazyRMSprop: momentum 0, not centered)
    table_kind: str = ""    # "" = the tables take `kind`; else (kind "adam") a key of TABLE_RULES: "adagrad" / "rowwise_adagrad"
                            # (utils/optim.AdamAdagradTables: torch.optim.Adagrad on the tables, exactly row-sparse, with table_eps and
                            # the learning rate lr * table_lr_scale; row-wise: ONE accumulator per row), "rowwise_adagrad_bf16[:<seed>]"
                            # (bf16_table_kind: that rule on tables STORED as bf16, rounded stochastically under the seed the value
                            # carries — no field of its own: tests pin the tuple's fields), "rowwise_adam" (utils/optim.RowwiseSparseAdam:
                            # row-sparse Adam with ONE second moment per row; table_eps and table_lr_scale unused)
    table_eps: float = 1e-2
    table_lr_scale: float = 1.0
    dwd: float = 0.0        # decoupled weight decay p <- p (1 - lr dwd) before the update (utils/optim.DecoupledWeightDecay,
                            # csrc/decoupled_decay.hip) over the parameters no_reg leaves in; 0 = none.  (In front of `ema`, which tests pin as the last field:
                            # every positional use stops at `alpha`.)
    ema: float = 0.0        # decay of a weight average kept beside the step (utils/optim.WeightEMA, csrc/weight_ema.hip); 0 = none

    @property
    def table_rule(self) -> TableRule:
        """what the fused step does to a table row under this spec.  A table_kind that is no rule of the tables' own (only the bf16
        rule takes a ":<seed>") gives _UNKNOWN_RULE, which goes with no dense rule: SupernetEngine._optim_scalars refuses it"""
        if self.table_kind:
            head = self.table_kind.partition(":")[0]
            rule = TABLE_RULES.get(head if head == "rowwise_adagrad_bf16" else self.table_kind)
            return rule if rule is not None and rule.table_algo else _UNKNOWN_RULE
        if self.kind in ("adagrad", "rmsprop"):
            return TABLE_RULES["plain_adagrad" if self.kind == "adagrad" else "lazy_rmsprop"]
        return TABLE_RULES["row_sparse_adam" if self.sparse_rows else "dense"]

    @property
    def moments(self) -> bool:
        """Adam / SGD / RMSprop: state in the engine's moment arrays and step counters (Adagrad: its accumulators)"""
        return self.kind != "adagrad"  # (the dense parameters' rule: no fact about the tables)

    rows_only = property(lambda self: self.table_rule.rows_only, doc="the tables move in the batch's rows only (a row outside it keeps its bits, or owes only a closed-form factor)")
    table_rowwise = property(lambda self: self.table_rule.rowwise, doc="the tables' accumulator / second moment is one float per row")
    rowwise_adam = property(lambda self: self.table_rule is TABLE_RULES["rowwise_adam"], doc="row-sparse Adam on the tables with one second moment per row (utils/optim.RowwiseSparseAdam)")
    adagrad_tables = property(lambda self: bool(self.table_kind) and self.table_rule.state != "moments", doc="the split optimizer: the tables' state is Adagrad's `sum`, not a moment array")
    bf16_tables = property(lambda self: self.table_rule.bf16, doc="the rule of tables stored as bf16: the only one the fused step has for them")

    @property
    def table_seed(self) -> int:
        """the seed of the stochastic rounding of bf16 tables (0 for every other rule)"""
        head, _, seed = self.table_kind.partition(":")
        return int(seed) if (head == "rowwise_adagrad_bf16" and seed) else 0

    @staticmethod
    def bf16_table_kind(seed: int = 0) -> str:
        """the table_kind of row-wise Adagrad on bf16 tables with this seed"""
        return "rowwise_adagrad_bf16:%d" % int(seed) if int(seed) else "rowwise_adagrad_bf16"

    @property
    def state_keys(self):
        """the per-parameter tensors torch keeps in optimizer.state[p] (besides "step")"""
        return {"adagrad": ("sum",), "adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",)}.get(self.kind, ("momentum_buffer",))

    @staticmethod
    def of(eps: float = 1e-2, weight_decay: float = 0.0, no_reg_param_name: Optional[str] = None, optim=None, ema: float = 0.0,
           decoupled_wd: float = 0.0) -> "OptimSpec":
        """the public entry points' optimizer arguments as one spec: optim None = Adagrad with `eps` (its only source: the default eps
        of a spec is Adam's), else an Adam / SGD spec; no_reg_param_name only counts with weight decay (the L2 term's or the decoupled one);
        ema: the decay of the weight average the step keeps (0 = none, or what `optim` already carries); decoupled_wd: the lambda of
        the decoupled weight decay in front of the update (0 = none, or what `optim` already carries)"""
        if optim is not None and not optim.moments:
            raise ValueError("optim is an Adam / SGD spec; Adagrad is optim=None with its eps")
        wd = float(weight_decay or 0.0)
        base = optim if optim is not None else OptimSpec("adagrad", eps=float(eps))
        ema = float(ema or 0.0)
        if ema and not 0.0 < ema < 1.0:
            raise ValueError("ema decay %r is not inside (0, 1)" % (ema,))
        dwd = float(decoupled_wd or 0.0)
        if dwd < 0.0:
            raise ValueError("decoupled weight decay %r is negative" % (dwd,))
        dwd = dwd if dwd else base.dwd
        return base._replace(wd=wd, no_reg=no_reg_param_name if (wd or dwd) else None, ema=ema if ema else base.ema, dwd=dwd)

    @staticmethod
    def from_optimizer(optimizer) -> Optional["OptimSpec"]:
        """the spec of a torch.optim.Adam / torch.optim.SGD the fused step reproduces, else None.
        Adam: one group, amsgrad, weight_decay, maximize, capturable, differentiable and fused all off.
        SGD: one group, momentum != 0 (plain SGD keeps the torch route), dampening 0, weight_decay 0, not maximize / differentiable / fused.
        RowSparseAdam: Adam's conditions (its one group carries Adam's keys) -> sparse_rows.
        RowwiseSparseAdam: the same conditions -> table_kind "rowwise_adam" (sparse_rows stays False: the tables take one rule).
        AdamAdagradTables: Adam's conditions -> table_kind "adagrad", or "rowwise_adagrad" where the group's table_rowwise is set, with
        the group's table_eps / table_lr_scale (plain numbers); tables of dtype bfloat16 (accepted by that optimizer only with
        table_rowwise) -> bf16_table_kind(the group's table_seed).
        LazyRMSprop (that type exactly: a hand-built torch.optim.RMSprop keeps the torch route): one group, momentum 0, not centered,
        weight_decay 0, not maximize / capturable / differentiable."""
        from .utils.optim import AdamAdagradTables, LazyRMSprop, RowSparseAdam, RowwiseSparseAdam
        if len(optimizer.param_groups) != 1:
            return None
        g = optimizer.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("maximize", False) or g.get("differentiable", False) or g.get("fused"):
            return None
        if type(optimizer) in (torch.optim.Adam, RowSparseAdam, RowwiseSparseAdam, AdamAdagradTables):
            if g.get("amsgrad", False) or g.get("capturable", False):
                return None
            b1, b2 = g["betas"]
            if torch.is_tensor(b1) or torch.is_tensor(b2):
                return None
            if type(optimizer) is AdamAdagradTables:
                if torch.is_tensor(g["table_eps"]) or torch.is_tensor(g["table_lr_scale"]) or torch.is_tensor(g["eps"]):
                    return None
                kind = "rowwise_adagrad" if g.get("table_rowwise", False) else "adagrad"
                if optimizer.bf16_tables:
                    if kind != "rowwise_adagrad":
                        return None
                    kind = OptimSpec.bf16_table_kind(g.get("table_seed", 0))
                return OptimSpec("adam", beta1=float(b1), beta2=float(b2), eps=float(g["eps"]), table_kind=kind,
                                 table_eps=float(g["table_eps"]), table_lr_scale=float(g["table_lr_scale"]))
            if type(optimizer) is RowwiseSparseAdam:
                if torch.is_tensor(g["eps"]):
                    return None
                return OptimSpec("adam", beta1=float(b1), beta2=float(b2), eps=float(g["eps"]), table_kind="rowwise_adam")
            return OptimSpec("adam", beta1=float(b1), beta2=float(b2), eps=float(g["eps"]), sparse_rows=type(optimizer) is RowSparseAdam)
        if type(optimizer) is LazyRMSprop:
            if g.get("momentum", 0) != 0 or g.get("centered", False) or g.get("capturable", False):
                return None
            if torch.is_tensor(g["alpha"]) or torch.is_tensor(g["eps"]):
                return None
            return OptimSpec("rmsprop", alpha=float(g["alpha"]), eps=float(g["eps"]))
        if type(optimizer) is torch.optim.SGD:
            if g.get("dampening", 0) != 0 or not g.get("momentum", 0):
                return None
            return OptimSpec("sgd", momentum=float(g["momentum"]), nesterov=bool(g.get("nesterov", False)))
        return None

    @staticmethod
    def for_step(optimizer, weight_decay: float = 0.0, no_reg_param_name: Optional[str] = None) -> Optional["OptimSpec"]:
        """the spec of the fused step that stands in for `optimizer.step()` on the loss + get_l2_loss(model, weight_decay,
        no_reg_param_name), or None when the fused step does not reproduce the optimizer.  torch.optim.Adagrad: one group,
        weight_decay, lr_decay and initial_accumulator_value 0, not maximize; Adam / SGD / RowSparseAdam: from_optimizer.  Row-sparse
        Adam (either form), RMSprop and AdamAdagradTables with a regularised table are None too (`regularises_tables`): the L2 term puts a gradient
        on every row, and RMSprop's rows rest only while their gradient is zero."""
        if type(optimizer) is not torch.optim.Adagrad:
            optim = OptimSpec.from_optimizer(optimizer)
            if optim is not None and (optim.sparse_rows or optim.kind == "rmsprop" or optim.table_kind) and regularises_tables(weight_decay, no_reg_param_name):
                return None
            return OptimSpec.of(weight_decay=weight_decay, no_reg_param_name=no_reg_param_name, optim=optim) if optim is not None else None
        if len(optimizer.param_groups) != 1:
            return None
        g = optimizer.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("lr_decay", 0) != 0 or g.get("initial_accumulator_value", 0) != 0 or g.get("maximize", False):
            return None
        return OptimSpec.of(float(g["eps"]), weight_decay, no_reg_param_name)


def regularises_tables(weight_decay, no_reg_param_name: Optional[str]) -> bool:
    """get_l2_loss(model, weight_decay, no_reg_param_name) reaches an embedding table: it leaves out the names that START with
    no_reg_param_name (utils/train_utils.py), so every table "_embedding.<f>.weight" is left out exactly by a prefix of "_embedding." """
    return bool(weight_decay) and not (no_reg_param_name is not None and "_embedding.".startswith(no_reg_param_name))
