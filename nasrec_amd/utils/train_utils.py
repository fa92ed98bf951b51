"""Training / evaluation loops of the harness with the reference's signatures, logs and printouts
(nasrec/utils/train_utils.py:70-499), driving the HIP engine.

`train_and_test_one_epoch` keeps the reference's step order (H2D, zero_grad, forward, BCE + L2, backward,
clip_grad_norm_, optimizer.step, LR step after the optimizer, train_utils.py:255-287,386).  When the run is one the fused
engine step covers — the model exposes `engine_train_step`, the optimizer is torch.optim.Adagrad without weight/lr decay
(or torch.optim.Adam / SGD with momentum as main_train.py builds them, one process with whole tables: optim_spec.py),
the L2 term is identically zero (`--wd 0`, the published recipes) or an `L2Loss` spec (any `--wd`, one process with whole
tables) and AMP is off — the whole step is ONE engine call
(captured in a hipGraph for fixed sub-networks); anything else takes the reference's operator-by-operator route through
`model(int_x, cat_x)` + autograd + the torch optimizer, which the module also supports.

Not available in this environment: fvcore and tensorboard.  FLOPs are counted analytically from the engine's launch plan
(multiply-accumulates of every Linear / attention product, what fvcore's FlopCountAnalysis reports for the supported
operators), the TensorBoard writer is optional (None disables it)."""
import contextlib
import copy
import os
import time
from typing import Any, Optional, Union

import numpy as np
import sklearn.metrics
import torch
import torch.nn as nn

from .. import metrics
from ..supernet.supernet import SuperNet


def init_weights(m):
    """train_utils.py:70-89: type-exact dispatch (sub-classes keep their own init)"""
    if type(m) == nn.Embedding:
        torch.nn.init.xavier_normal_(m.weight)
    elif type(m) == nn.Linear:
        torch.nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            torch.nn.init.zeros_(m.bias)
    elif type(m) == nn.MultiheadAttention:
        for p in m.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
            else:
                torch.nn.init.zeros_(p)


def get_l2_loss(model: nn.Module, reg: float, no_reg_param_name: Union[str, None] = None, gpu: Optional[int] = None):
    """reg * sum ||W||_2^2 over every parameter with >= 2 dimensions (tables included) whose name does not start with
    `no_reg_param_name`; exactly 0 for reg == 0 (train_utils.py:91-115)"""
    if reg == 0:
        return torch.tensor(0.0).to(gpu)
    total = None
    for name, p in model.named_parameters():
        if p.dim() == 1 or (no_reg_param_name is not None and name.startswith(no_reg_param_name)):
            continue
        term = torch.square(torch.norm(p, p=2)) * reg
        total = term if total is None else total + term
    return total


class L2Loss:
    """get_l2_loss(model, wd, no_reg_param_name, gpu) as a callable the fused engine step can read: calling it returns exactly what
    get_l2_loss returns, and `wd` / `no_reg_param_name` tell the engine which term to fold into its step (an opaque callable with a
    non-zero value sends the step to the torch route)."""

    def __init__(self, wd: float, no_reg_param_name: Union[str, None] = None, gpu: Optional[int] = None):
        self.wd, self.no_reg_param_name, self.gpu = float(wd), no_reg_param_name, gpu

    def __call__(self, model: nn.Module):
        return get_l2_loss(model, self.wd, self.no_reg_param_name, gpu=self.gpu)

    def __repr__(self):
        return "L2Loss(wd=%r, no_reg_param_name=%r, gpu=%r)" % (self.wd, self.no_reg_param_name, self.gpu)


def accuracy(gt, pred):
    """fraction of predictions > 0.5 that equal the label (train_utils.py:118-126; callers pass probabilities)"""
    hit = (torch.gt(pred, 0.5).float() == gt).sum()
    return hit / pred.size(0)


def _auroc(y_true, y_prob):
    """sklearn.metrics.roc_auc_score of the two tensors: on their GPU (metrics.roc_auc_score, the same float64 bits) when both are
    contiguous float32 CUDA tensors of one device and equal length; anything else (CPU tensors, half scores under autocast, other
    dtypes) on the host as before"""
    if metrics.roc_auc_supported(y_true, y_prob):
        return metrics.roc_auc_score(y_true.detach(), y_prob.detach())
    return sklearn.metrics.roc_auc_score(y_true.detach().cpu().numpy(), y_prob.detach().cpu().numpy())


def test_one_epoch(model, test_loader, loss_fn, gpu: Optional[int] = None, max_steps=-1, use_amp: bool = False):
    """-> (accuracy, AUROC, loss) over the concatenated predictions of the loader (train_utils.py:129-178)"""
    model.eval()
    preds, labels, n = [], [], 0
    with torch.no_grad():
        for int_x, cat_x, y in test_loader:
            int_x, cat_x, y = int_x.to(gpu), cat_x.to(gpu), y.to(gpu)
            with torch.autocast("cuda", enabled=use_amp):
                preds.append(model(int_x, cat_x).clone())
            labels.append(y)
            n += 1
            if n % 50 == 0:
                print("done {} batches!".format(n))
            if max_steps != -1 and n >= max_steps:
                break
        print("Done {} batches!".format(n))
        y_true, y_pred = torch.cat(labels).flatten(), torch.cat(preds).flatten()
        prob = torch.sigmoid(y_pred)
        auroc = _auroc(y_true, prob)
        acc = accuracy(y_true, prob)
        loss = loss_fn(y_pred, y_true)
    return acc.item(), float(auroc), loss.item()


test_one_epoch.__test__ = False  # not a pytest test


def _optim_spec(optimizer, l2_loss_fn):
    """OptimSpec.for_step with the weight decay of an L2Loss (any other l2_loss_fn adds none: the callers check that it is zero)"""
    from ..optim_spec import OptimSpec
    if isinstance(l2_loss_fn, L2Loss):
        return OptimSpec.for_step(optimizer, l2_loss_fn.wd, l2_loss_fn.no_reg_param_name)
    return OptimSpec.for_step(optimizer)


def _refuse_regularised_tables(optimizer, l2_loss_fn):
    """row-sparse Adam moves a table in the batch's rows only; an L2 term over a table puts a gradient on every row, on either route"""
    from ..optim_spec import OptimSpec, regularises_tables
    spec = OptimSpec.from_optimizer(optimizer) if isinstance(optimizer, torch.optim.Optimizer) else None
    if spec is not None and (spec.sparse_rows or spec.rowwise_adam) and isinstance(l2_loss_fn, L2Loss) and \
            regularises_tables(l2_loss_fn.wd, l2_loss_fn.no_reg_param_name):
        raise ValueError("row-sparse Adam cannot train a regularised embedding table (weight decay %g reaches every row): pass "
                         "--no-reg-param-name _embedding to leave the tables out of the L2 term, or --wd 0" % l2_loss_fn.wd)


def _last_layer_step_applies(model, optimizer, l2_loss_fn, use_amp):
    """engine_last_layer_step stands in for the torch route's step: a SuperNet in last-layer mode (every parameter outside _final
    frozen) of one process with whole tables on the device, an L2Loss, and an optimizer OptimSpec.for_step accepts whose one group
    holds _final — an Adagrad also neither differentiable nor fused"""
    if use_amp or not hasattr(model, "engine_last_layer_step") or not isinstance(l2_loss_fn, L2Loss):
        return False
    from .dist import world_info
    if world_info()[1] > 1 or getattr(model, "_table_sharding", None) == "row" or getattr(model, "_place_embedding_on_cpu", False):
        return False
    spec = _optim_spec(optimizer, l2_loss_fn)
    if spec is None or spec.kind == "rmsprop" or spec.adagrad_tables or not model._last_layer_only():  # (RMSprop, AdamAdagradTables: the fine-tune keeps the torch route)
        return False
    g = optimizer.param_groups[0]
    if not {id(p) for p in model._final.parameters()} <= {id(p) for p in g["params"]}:
        return False
    # (only this route refuses a differentiable / fused Adagrad: _fused_step_applies takes it)
    return not (type(optimizer) is torch.optim.Adagrad and (g.get("differentiable", False) or g.get("fused")))


def _whole_table_optimizers_apply(model) -> bool:
    """weight decay and Adam / SGD in the fused step: whole tables, and one process — or several, when the model's engine_train_step
    runs them inside its data-parallel exchange step (`engine_dp_optimizers`, SuperNet: nasrec_amd/parallel.py).  A model whose fused
    step has no exchange for them would train every rank on its own share of the batch: the replicas would drift apart silently."""
    if getattr(model, "_table_sharding", None) == "row":
        return False
    from .dist import world_info
    return world_info()[1] <= 1 or bool(getattr(model, "engine_dp_optimizers", False))


def _ema_route(model, spec, l2_loss_fn):
    """why a step with a weight average keeps the torch route (WeightEMA.update() is dense and exact there), or None: the fused step
    averages the batch's table rows only, so it applies where the tables move in those rows alone (OptimSpec.rows_only) — Adagrad,
    row-sparse Adam, RMSprop or Adam with Adagrad on the tables, no regularised table — in one process with whole tables on the device"""
    from ..optim_spec import regularises_tables
    from .dist import world_info
    if not spec.rows_only:
        return "%s moves every table row every step" % ("dense Adam" if spec.kind == "adam" else "momentum SGD")
    if isinstance(l2_loss_fn, L2Loss) and regularises_tables(l2_loss_fn.wd, l2_loss_fn.no_reg_param_name):
        return "weight decay reaches the embedding tables: every row moves every step"
    if world_info()[1] > 1:
        return "data-parallel run"  # (paths="per-rank" included: it exists only there)
    if getattr(model, "_table_sharding", None) == "row":
        return "row-sharded tables"
    return None


def _decay_route(model, spec, l2_loss_fn, decay, ema=None):
    """why a step with decoupled weight decay keeps the torch route (DecoupledWeightDecay.apply() is dense and exact there), or None:
    the fused step decays the batch's table rows and lets the others rest, so it applies where _ema_route's conditions hold — and,
    when the decay reaches the tables, with neither a fused weight EMA (its rows' weights would change while they rest) nor an L2 term
    on the tables"""
    from ..optim_spec import regularises_tables
    why = _ema_route(model, spec, l2_loss_fn)
    if why is None and ema is not None and regularises_tables(decay.weight_decay, decay.no_reg_param_name):
        why = "a weight EMA is kept beside the step and the decay reaches the embedding tables"
    return why


def _fused_step_spec(model, optimizer, l2_loss_fn, use_amp, ema=None, decay=None):
    """the OptimSpec of the fused engine step that stands in for this model's torch step (OptimSpec.for_step), or None: the torch route.
    ema: a WeightEMA (utils/optim.py) kept beside the step — the spec then carries its decay, and the answer is None wherever the
    fused average is not exact (_ema_route).  decay: a DecoupledWeightDecay (utils/optim.py) applied in front of the update — the
    spec then carries its lambda as `dwd` and its no_reg_param_name, and the answer is None wherever the lazily paid decay is not
    exact (_decay_route)"""
    if decay is not None:
        spec = _fused_step_spec(model, optimizer, l2_loss_fn, use_amp, ema)
        if spec is None or _decay_route(model, spec, l2_loss_fn, decay, ema) is not None:
            return None
        if spec.wd and spec.no_reg != decay.no_reg_param_name:
            return None  # (one notion of "regularised" per step: the L2 term and the decay share no_reg_param_name)
        return spec._replace(dwd=float(decay.weight_decay), no_reg=decay.no_reg_param_name)
    if ema is not None:
        spec = _fused_step_spec(model, optimizer, l2_loss_fn, use_amp)
        if spec is None or _ema_route(model, spec, l2_loss_fn) is not None:
            return None
        return spec._replace(ema=float(ema.decay))
    if use_amp or not hasattr(model, "engine_train_step"):
        return None
    spec = _optim_spec(optimizer, l2_loss_fn)
    if spec is None or getattr(model, "_place_embedding_on_cpu", False):
        return None  # (the tables on the host: torch's optimizer updates them there)
    # the fused step updates the WHOLE dense arena and every touched embedding row: it only stands in for optimizer.step() when
    # every parameter trains and the optimizer's single group covers all of them (set_mode_to_finelune_last_only /
    # layernorm_calibrate / finetune_no_embedding, or an optimizer over a parameter subset, take the torch route)
    params = list(model.parameters())
    if not all(p.requires_grad for p in params):
        return None
    if {id(p) for p in params} != {id(p) for p in optimizer.param_groups[0]["params"]}:
        return None
    # weight decay, Adam and SGD need whole tables (_whole_table_optimizers_apply); row-sharded tables keep the torch route with them
    if (spec.wd or spec.moments) and not _whole_table_optimizers_apply(model):
        return None
    if not spec.wd:
        with torch.no_grad():
            if float(l2_loss_fn(model)) != 0.0:
                return None
    return spec


def _fused_step_applies(model, optimizer, l2_loss_fn, use_amp, ema=None, decay=None):
    return _fused_step_spec(model, optimizer, l2_loss_fn, use_amp, ema, decay) is not None


def _announce_decay_route(model, optimizer, l2_loss_fn, use_amp, ema, decay, fused):
    """one line per run: which route applies the decoupled weight decay, and why"""
    if getattr(decay, "_route_announced", False):
        return
    decay._route_announced = True
    if fused:
        print("Decoupled weight decay (lambda {}): fused step, lazily decayed embedding rows.".format(decay.weight_decay))
        return
    spec = _fused_step_spec(model, optimizer, l2_loss_fn, use_amp, ema)
    if spec is None:
        why = "the fused step does not apply"
    else:
        why = _decay_route(model, spec, l2_loss_fn, decay, ema) or "the fused step was switched off"
    print("Decoupled weight decay (lambda {}): torch route, dense DecoupledWeightDecay.apply() before every step ({}).".format(
        decay.weight_decay, why))


def _announce_ema_route(model, optimizer, l2_loss_fn, use_amp, ema, fused):
    """one line per run: which route averages the weights, and why"""
    if getattr(ema, "_route_announced", False):
        return
    ema._route_announced = True
    if fused:
        print("Weight EMA (decay {}): fused step, lazily averaged embedding rows.".format(ema.decay))
        return
    spec = _fused_step_spec(model, optimizer, l2_loss_fn, use_amp)
    why = "the fused step does not apply" if spec is None else (_ema_route(model, spec, l2_loss_fn) or "the fused step was switched off")
    print("Weight EMA (decay {}): torch route, dense WeightEMA.update() after every step ({}).".format(ema.decay, why))


def _announce_split_route(optimizer, l2_loss_fn, fused, switched_off=False):
    """one line per run with AdamAdagradTables (utils/optim.py): which route takes the step, and why"""
    from .optim import AdamAdagradTables
    if type(optimizer) is not AdamAdagradTables or getattr(optimizer, "_route_announced", False):
        return
    optimizer._route_announced = True
    g = optimizer.param_groups[0]
    head = "Adam + {}Adagrad on the tables (table lr = lr x {}, table eps {})".format(
        "row-wise " if g.get("table_rowwise", False) else "", g["table_lr_scale"], g["table_eps"])
    if optimizer.bf16_tables:
        if not fused:  # (AdamAdagradTables.step would raise at the first batch: say why before anything runs)
            raise ValueError("bf16 tables (--table-dtype bf16) train on the fused step only, and it does not apply here: they need "
                             "every parameter trainable under one AdamAdagradTables(table_rowwise=True), one process, no AMP, no "
                             "weight decay, no --ema / --decoupled-wd and no last-layer mode")
        print(head + ": fused step, exactly row-sparse table update; bf16 tables stored with stochastic rounding (seed {}).".format(
            g.get("table_seed", 0)))
        return
    if fused:
        print(head + ": fused step, exactly row-sparse table update.")
        return
    from ..optim_spec import regularises_tables
    why = "the fused step was switched off" if switched_off else "the fused step does not apply"
    if isinstance(l2_loss_fn, L2Loss) and regularises_tables(l2_loss_fn.wd, l2_loss_fn.no_reg_param_name):
        why = "weight decay reaches the embedding tables: every row has a gradient (--no-reg-param-name _embedding leaves them out)"
    print(head + ": torch route, AdamAdagradTables.step() ({}).".format(why))


def _announce_rowwise_adam_route(model, optimizer, l2_loss_fn, use_amp, fused, switched_off=False):
    """one line per run with RowwiseSparseAdam (utils/optim.py): which route takes the step, and why"""
    from .optim import RowwiseSparseAdam
    if type(optimizer) is not RowwiseSparseAdam or getattr(optimizer, "_route_announced", False):
        return
    optimizer._route_announced = True
    head = "Row-wise Adam (row-sparse Adam, one second-moment float per embedding row)"
    if fused:
        print(head + ": fused step, the batch's table rows only.")
        return
    why = "the fused step was switched off" if switched_off else "the fused step does not apply"
    if use_amp:
        why = "AMP keeps the torch route"
    print(head + ": torch route, RowwiseSparseAdam.step() on the rows of touch() ({}).".format(why))


def refuse_cowclip(model, optimizer, l2_loss_fn, use_amp=False, last_layer_step=False, table_dtype=None):
    """`--cowclip` at start-up: what CowClip is not built for is a ValueError that names the flag, never a silent route elsewhere —
    bf16 tables, an L2 term that reaches the embedding tables (its 2 wd W would be clipped with the gradient), tables on the host,
    row-sharded tables, a data-parallel run (the counts would have to be global), the last-layer fine-tune step and the opt-in
    persistent form of the batch-256 step"""
    from ..optim_spec import regularises_tables
    from .dist import world_info
    head = "--cowclip "
    if getattr(optimizer, "bf16_tables", False) or table_dtype in ("bf16", torch.bfloat16):
        raise ValueError(head + "with bf16 tables (--table-dtype bf16): CowClip reads fp32 table rows; not built for bf16 tables")
    if isinstance(l2_loss_fn, L2Loss) and regularises_tables(l2_loss_fn.wd, l2_loss_fn.no_reg_param_name):
        raise ValueError(head + "with --wd %r reaching the embedding tables: the L2 term's 2 wd W would be clipped with the gradient "
                         "(--no-reg-param-name _embedding leaves the tables out, or --wd 0)" % (l2_loss_fn.wd,))
    if getattr(model, "_place_embedding_on_cpu", False):
        raise ValueError(head + "with the embedding tables on the host (place_embedding_on_cpu): CowClip needs them on the device")
    if getattr(model, "_table_sharding", None) == "row":
        raise ValueError(head + "with --table-sharding row: a row-sharded table holds one rank's rows; CowClip needs whole tables")
    if world_info()[1] > 1:
        raise ValueError(head + "with a world size of %d: the ids' counts would have to be global; one process" % world_info()[1])
    if last_layer_step:
        raise ValueError(head + "with the last-layer fine-tune step: the tables are frozen there, nothing to clip")
    if os.environ.get("NASREC_PERSIST_DEFAULT", "0") == "1":
        raise ValueError(head + "with the persistent step (NASREC_PERSIST_DEFAULT=1): CowClip is not built into it; unset the variable")


def _announce_cowclip_route(cowclip, fused, use_amp=False, switched_off=False):
    """one line per run: which route applies CowClip, and why"""
    if getattr(cowclip, "_route_announced", False):
        return
    cowclip._route_announced = True
    head = "CowClip (r {}, zeta {})".format(cowclip.r, cowclip.zeta)
    if fused:
        print(head + ": fused step, the batch's summed table rows scaled in front of the optimizer.")
        return
    why = "the fused step was switched off" if switched_off else ("AMP keeps the torch route" if use_amp else "the fused step does not apply")
    print(head + ": torch route, CowClip.apply() before every step ({}).".format(why))


def _agreed_batches(train_loader, train_batch_size: int, world: int, gpu):
    """The batches of one epoch.  Single process: the loader as it is (incl. its short last batch, which the reference evaluates
    without training on it).  Data parallel: every rank reads its own shards, which differ in length — the ranks agree one step
    ahead (utils/dist.StepAgreement, off the compute stream) on whether ALL of them hold a FULL batch for the next step, and the
    epoch ends for everybody at the first step some rank cannot take: no rank enters a collective the others skip."""
    if world <= 1:
        yield from train_loader
        return
    from .dist import StepAgreement
    agree = StepAgreement(gpu)
    it = iter(train_loader)

    def fetch():
        try:
            b = next(it)
        except StopIteration:
            return None
        return b

    nxt = fetch()
    agree.post(nxt is not None and len(nxt[2]) == train_batch_size)
    while True:
        ok = agree.take()
        if not ok:
            return
        cur = nxt
        nxt = fetch()
        agree.post(nxt is not None and len(nxt[2]) == train_batch_size)  # travels while the step on `cur` runs
        yield cur


def train_and_test_one_epoch(model, epoch: int, optimizer: Any, lr_scheduler, train_loader, test_loader, loss_fn, l2_loss_fn,
                             train_batch_size: int, gpu: Union[int, None], display_interval: int = 100, test_interval: int = 2000,
                             max_train_steps: int = -1, max_eval_steps: int = -1, test_only_at_last_step: bool = False,
                             grad_clip_value: float = None, tb_writer=None, use_amp: bool = False, use_engine_step: Optional[bool] = None,
                             last_layer_step: bool = False, ema=None, decay=None, cowclip=None):
    """One epoch of training with tests in between; returns the reference's log dict (train_utils.py:181-390).
    `use_engine_step`: None = fused engine step whenever it applies, False = always the torch route.
    `last_layer_step`: a model in last-layer mode (set_mode_to_finelune_last_only) with a qualifying optimizer trains every full batch
    through SuperNet.engine_last_layer_step (_last_layer_step_applies); False (default) = as before.
    `ema`: a WeightEMA (utils/optim.py): every step that is taken updates it — inside the fused step where that is exact
    (_fused_step_spec), by `ema.update()` otherwise — and the tests run on the averaged weights (`ema.averaged()`); None = no average.
    `decay`: a DecoupledWeightDecay (utils/optim.py): every step that is taken multiplies the selected parameters that have a gradient
    by 1 - lr lambda in front of the optimizer's update — inside the fused step where the lazily paid decay is exact
    (_fused_step_spec), by `decay.apply(lr)` otherwise; None = no decay.
    `cowclip`: a CowClip (utils/optim.py) over the model's tables: every step that is taken holds the batch's table rows' gradients to
    cnt max(r ||w||, zeta) behind the global clip — inside the fused step wherever that step applies, by `cowclip.apply(cat_x)` in
    front of `optimizer.step()` otherwise; what it is not built for is refused here by the flag's name (refuse_cowclip).  Display
    steps print the share of touched rows clipped since the last one.  None = off: nothing changes."""
    _refuse_regularised_tables(optimizer, l2_loss_fn)
    if cowclip is not None:
        refuse_cowclip(model, optimizer, l2_loss_fn, use_amp, last_layer_step)
    _peek(test_loader)  # the reference peeks one test batch here (train_utils.py:224-225)
    model.train()
    logs = {k: [] for k in ("train_loss", "train_AUROC", "train_Accuracy", "test_loss", "test_AUROC", "test_Accuracy", "epoch", "iters")}
    if decay is not None and not decay.weight_decay:
        decay = None  # (lambda = 0 is "no helper")
    fused = _fused_step_applies(model, optimizer, l2_loss_fn, use_amp, ema, decay) if use_engine_step is None else bool(use_engine_step)
    if getattr(optimizer, "bf16_tables", False) and (use_amp or last_layer_step or ema is not None or decay is not None):
        raise ValueError("bf16 tables (--table-dtype bf16) run with neither AMP (use_amp), the last-layer fine-tune step, a weight EMA "
                         "(--ema) nor a decoupled weight decay (--decoupled-wd): none of them is built for bf16 tables")
    _announce_split_route(optimizer, l2_loss_fn, fused, switched_off=use_engine_step is False)
    _announce_rowwise_adam_route(model, optimizer, l2_loss_fn, use_amp, fused, switched_off=use_engine_step is False)
    if ema is not None:
        if fused and use_engine_step is not None and not _fused_step_applies(model, optimizer, l2_loss_fn, use_amp, ema):
            raise ValueError("use_engine_step=True with a weight EMA the fused step cannot keep exactly: leave use_engine_step=None")
        _announce_ema_route(model, optimizer, l2_loss_fn, use_amp, ema, fused)
    if decay is not None:
        if fused and use_engine_step is not None and not _fused_step_applies(model, optimizer, l2_loss_fn, use_amp, ema, decay):
            raise ValueError("use_engine_step=True with a decoupled weight decay the fused step cannot keep exactly: leave "
                             "use_engine_step=None")
        _announce_decay_route(model, optimizer, l2_loss_fn, use_amp, ema, decay, fused)
    if cowclip is not None:
        _announce_cowclip_route(cowclip, fused, use_amp, switched_off=use_engine_step is False)

    def cow_rows():  # (rows touched, rows clipped) so far on both routes: the engine's and the helper's counters are cumulative
        fused_rows = model.engine_cowclip_stats() if (fused and hasattr(model, "engine_cowclip_stats")) else (0, 0)
        return fused_rows[0] + cowclip.touched, fused_rows[1] + cowclip.clipped
    cow_seen = cow_rows() if cowclip is not None else (0, 0)  # ... at the last display step (an earlier epoch's rows are not this one's)
    # (a decoupled decay keeps the last-layer fine-tune on the torch route: the fused last-layer step has none)
    last_only = bool(last_layer_step) and not fused and use_engine_step is not False and decay is None and \
        _last_layer_step_applies(model, optimizer, l2_loss_fn, use_amp)
    bound = ema_bound = False
    scaler = torch.amp.GradScaler("cuda") if use_amp else None
    best_model, best_test_loss = None, 9999.99
    t_data0 = time.time()
    batch_num = -1
    from .dist import StepAgreement, allreduce_grads, any_rank, world_info
    world = world_info()[1]
    zero_l2 = None
    # the fused steps' optimizer, once: Adagrad's eps or Adam / SGD's hyperparameters, and the L2 term's weight decay (the learning rate
    # is read every step).  use_engine_step=True forces the fused step for an optimizer OptimSpec.for_step refuses: Adagrad with its eps.
    from ..optim_spec import OptimSpec
    spec = _optim_spec(optimizer, l2_loss_fn) if (fused or last_only) else None
    if fused and spec is None:
        wd = l2_loss_fn.wd if isinstance(l2_loss_fn, L2Loss) else 0.0
        spec = OptimSpec.of(float(optimizer.param_groups[0]["eps"]), wd, getattr(l2_loss_fn, "no_reg_param_name", None))
    opt_kw = {}
    if spec is not None:
        opt_kw = dict(weight_decay=spec.wd, no_reg_param_name=spec.no_reg)
        if spec.moments:
            opt_kw["optim"] = spec
        else:
            opt_kw["eps"] = spec.eps
    step_kw = dict(opt_kw, ema_decay=float(ema.decay)) if (ema is not None and fused) else opt_kw
    if decay is not None and fused:
        step_kw = dict(step_kw, decoupled_wd=float(decay.weight_decay), no_reg_param_name=decay.no_reg_param_name)
    if cowclip is not None and fused:
        step_kw = dict(step_kw, cowclip=(cowclip.r, cowclip.zeta))
    wd = spec.wd if spec is not None else 0.0
    for batch_num, (int_x, cat_x, y) in enumerate(_agreed_batches(train_loader, train_batch_size, world, gpu)):
        t_data1 = time.time()
        on_dev = int_x.is_cuda and cat_x.is_cuda and y.is_cuda and (not isinstance(gpu, int) or int_x.device.index == gpu)
        if not on_dev:  # (device-staged batches are there already: three no-op .to() calls are 6 us of a 300 us step)
            int_x, cat_x, y = int_x.to(gpu, non_blocking=True), cat_x.to(gpu, non_blocking=True), y.to(gpu, non_blocking=True)
        t_gpu0 = time.time()
        full = len(y) == train_batch_size  # a short last batch is evaluated but not trained on
        if last_only and full:
            if not bound:
                model._ensure_engine(int_x)
                model.engine_bind_optimizer(optimizer, last_layer=True)
                bound = True
            group = optimizer.param_groups[0]
            # the L2 term is only looked at on display steps: there it is get_l2_loss of the weights BEFORE the step, as the torch route has it
            l2_loss = None
            if batch_num % display_interval == 0 or batch_num == max_train_steps - 1:
                with torch.no_grad():
                    l2_loss = l2_loss_fn(model)
            loss = model.engine_last_layer_step(int_x, cat_x, y.view(-1), lr=float(group["lr"]), clip=grad_clip_value, **opt_kw)
            if ema is not None:
                ema.update()
            res = None
        elif fused and full:
            if not bound:  # lazy shapes + engine, then share the Adagrad accumulators (a resumed optimizer keeps its state)
                model._ensure_engine(int_x)
                model.engine_bind_optimizer(optimizer)
                bound = True
                if ema is not None:
                    model.engine_bind_ema(ema)
                    ema_bound = True
            if decay is not None and decay._flush is None:  # (a torch-route apply() in the middle of the fused run flushes first)
                model.engine_bind_decay(decay)
            group = optimizer.param_groups[0]
            loss = model.engine_train_step(int_x, cat_x, y.view(-1), lr=float(group["lr"]), clip=grad_clip_value, **step_kw)
            # the step's logits and the L2 term are only looked at on display steps: fetched there, not 3 900 times per epoch
            # (`torch.zeros` is a fill launch on the GPU, `engine_last_logits` a plan lookup)
            res = None
            if zero_l2 is None:
                zero_l2 = torch.zeros((), device=y.device)
            l2_loss = None if wd else zero_l2
        else:
            optimizer.zero_grad()
            with torch.autocast("cuda", enabled=use_amp):
                res = model(int_x, cat_x)
                loss = loss_fn(res, y)
                l2_loss = l2_loss_fn(model)
                total_loss = loss + l2_loss
            if full:
                if use_amp:
                    scaler.scale(total_loss).backward()
                    if world > 1:
                        # the DDP order: exchange the still-SCALED gradients, then unscale — every rank then sees the same inf / NaN
                        # (found_inf) and skips or takes the step together; unscaling first would let the overflowing rank skip
                        # alone while the others step on inf-averaged gradients
                        allreduce_grads(model)
                    scaler.unscale_(optimizer)
                    if grad_clip_value is not None:
                        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip_value)
                    if hasattr(optimizer, "touch"):
                        optimizer.touch(cat_x)
                    if decay is not None:
                        decay.apply(float(optimizer.param_groups[0]["lr"]))
                    if cowclip is not None:
                        cowclip.apply(cat_x)
                    scale0 = scaler.get_scale() if ema is not None else None
                    scaler.step(optimizer)
                    scaler.update()
                    if ema is not None and scaler.get_scale() >= scale0:  # (a skipped step halves the scale: nothing to average)
                        ema.update()
                else:
                    total_loss.backward()
                    if world > 1:  # the torch route has no exchange of its own: average the gradients over the ranks
                        allreduce_grads(model)
                    if grad_clip_value is not None:
                        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip_value)
                    if hasattr(optimizer, "touch"):  # (RowSparseAdam: the rows this batch touches)
                        optimizer.touch(cat_x)
                    if decay is not None:
                        decay.apply(float(optimizer.param_groups[0]["lr"]))
                    if cowclip is not None:
                        cowclip.apply(cat_x)
                    optimizer.step()
                    if ema is not None:
                        ema.update()
        t_gpu1 = time.time()
        last = batch_num == max_train_steps - 1

        if batch_num % display_interval == 0 or last:
            if res is None:
                res = model.engine_last_logits()
            if l2_loss is None:
                l2_loss = model.engine_last_l2()
            y_pred, y_true = res.detach(), y.detach()
            if any_rank(bool(torch.isnan(loss)), gpu):  # happens on KDD: report a diverged model (every rank leaves together)
                print("Loss NaN. Exiting...")
                logs["test_loss"].append(999.99)
                logs["test_AUROC"].append(-1)
                logs["test_Accuracy"].append(-1)
                return logs
            loss_v, l2_v = float(loss.detach()), float(l2_loss.detach())
            print(f"Epoch: {epoch:>d} L2: {l2_v:>7f} loss: {loss_v:>7f}  {batch_num}")
            lr_now = lr_scheduler.get_lr()
            print("Learning rate: {}".format(lr_now[0] if isinstance(lr_now, list) else lr_now))
            print("Data: {:.5f} (s), GPU: {:.5f} (s)".format(t_data1 - t_data0, t_gpu1 - t_gpu0))
            prob = torch.sigmoid(y_pred).view(-1)
            try:
                train_auroc = float(_auroc(y_true.view(-1), prob))
            except Exception:
                print("AUROC encountered issues. All training data has the same label.")
                train_auroc = 1.0
            train_acc = accuracy(y_true.view(-1), prob).item()
            print("Train Acc: {}, Train AUROC: {}".format(train_acc, train_auroc))
            if cowclip is not None:
                now = cow_rows()
                rows_seen, rows_clipped = now[0] - cow_seen[0], now[1] - cow_seen[1]
                cow_seen = now
                print("CowClip: {:.1f} % of {} touched rows clipped since the last display.".format(
                    100.0 * rows_clipped / max(rows_seen, 1), rows_seen))
            if tb_writer is not None:
                x = batch_num * train_batch_size
                tb_writer.add_scalar("Loss/train/epoch{}".format(epoch), loss_v, x)
                tb_writer.add_scalar("Acc/train/epoch{}".format(epoch), train_acc, x)
                tb_writer.add_scalar("AUROC/train/epoch{}".format(epoch), train_auroc, x)
                tb_writer.add_scalar("iters/epoch{}".format(epoch), x, x)
            logs["train_loss"].append(loss_v)
            logs["train_AUROC"].append(train_auroc)
            logs["train_Accuracy"].append(train_acc)
            logs["epoch"].append(epoch)
            logs["iters"].append(batch_num)

        if batch_num % test_interval == 0 or last:
            if (not test_only_at_last_step) or last:
                model.eval()
                t0 = time.time()
                if ema_bound:
                    model.engine_sync_ema(ema)
                with (ema.averaged() if ema is not None else contextlib.nullcontext()):  # (the averaged weights are what is tested)
                    test_acc, test_auroc, test_loss = test_one_epoch(model, test_loader, loss_fn, gpu, max_steps=max_eval_steps, use_amp=use_amp)
                print("{:.4f} seconds elasped for testing!".format(time.time() - t0))
                print("Test Acc: {}, Test AUROC: {}, Test Loss: {}".format(test_acc, test_auroc, test_loss))
                logs["test_loss"].append(test_loss)
                logs["test_AUROC"].append(test_auroc)
                logs["test_Accuracy"].append(test_acc)
                if test_loss < best_test_loss:
                    best_model, best_test_loss = copy.deepcopy(model), test_loss
                if tb_writer is not None:
                    x = batch_num * train_batch_size
                    tb_writer.add_scalar("Loss/test/epoch{}".format(epoch), test_loss, x)
                    tb_writer.add_scalar("Acc/test/epoch{}".format(epoch), test_acc, x)
                    tb_writer.add_scalar("AUROC/test/epoch{}".format(epoch), test_auroc, x)
                    tb_writer.add_scalar("Best Loss/test/epoch{}".format(epoch), best_test_loss, x)
            model.train()
        if max_train_steps != -1 and batch_num >= max_train_steps - 1:
            break
        lr_scheduler.step()
        t_data0 = time.time()
    else:
        print("Batch counter total: {}".format(batch_num))
    if bound:
        model.engine_sync_optimizer_steps(optimizer)
    if decay is not None and hasattr(model, "engine_flush_decay"):
        model.engine_flush_decay()  # (every table row current: whoever reads the tables next needs no flush of their own)
    if ema_bound:
        model.engine_sync_ema(ema)
    del best_model  # the reference rebinds a local name to a copy of it: no observable effect
    return logs


def _peek(loader):
    """first batch of a loader without leaving reader threads / device blocks behind (RoundRobinLoader.peek); any other iterable:
    the reference's `next(iter(loader))`"""
    peek = getattr(loader, "peek", None)
    return peek() if peek is not None else next(iter(loader))


def warmup_model(model: nn.Module, train_loader, gpu: Union[int, None]):
    """one forward pass: fixes every lazy shape (train_utils.py:392-410)"""
    model = model.to(gpu)
    int_x, cat_x, _ = _peek(train_loader)
    model(int_x.to(gpu), cat_x.to(gpu))
    return model


def warmup_supernet_model(model: nn.Module, train_loader, gpu, freeze_gc: bool = False):
    """full-path forward so that every candidate operator materialises (train_utils.py:413-433).  freeze_gc: see
    SupernetEngine.reserve — only for a process that keeps this one model for its whole life (the train_supernet CLI)"""
    assert isinstance(model, SuperNet), NotImplementedError("For 'warmup_supernet_model', the passed in model must be a 'SuperNet' object.")
    model = model.to(gpu)
    int_x, cat_x, _ = _peek(train_loader)
    model.configure_path_sampling_strategy("full-path")
    model(int_x.to(gpu), cat_x.to(gpu))
    eng = getattr(model, "_engine", None)
    if eng is not None and hasattr(eng, "reserve") and not getattr(eng, "host_embedding", False):
        eng.reserve(int(int_x.shape[0]), freeze_gc=freeze_gc)  # plan slots sized for the full path: sampled paths never grow an arena mid-step
    return model


def get_model_flops_and_params(model, train_loader, gpu):
    """(multiply-accumulates per sample of one forward pass, number of parameters).  The reference asks fvcore
    (train_utils.py:436-452), which counts one flop per MAC of Linear / matmul / bmm and ignores the rest; here the same
    quantity is read off the engine's launch plan for the model's current choice."""
    from .. import _lib as L
    from .. import plan as P
    model = model.to(gpu)
    int_x, cat_x, _ = _peek(train_loader)
    int_x, cat_x = int_x.to(gpu), cat_x.to(gpu)
    with torch.no_grad():
        model(int_x, cat_x)
    B = int(int_x.shape[0])
    eng = model._engine
    cp = eng.compile(model.choice, B, train=False)
    macs = 0
    for d in P.iter_ops(cp.fwd.descs):
        if isinstance(d, L.GemmDesc):
            macs += sum(d.seg[q].M * d.seg[q].N * d.seg[q].K for q in range(d.nseg) if d.seg[q].A)
        elif isinstance(d, L.MhaDesc):  # in/out projections + FFN (4 x 16x16 ... per token) and the two attention products
            macs += d.B * d.N * (3 * 256 + 256 + 256 + 256) + 2 * d.B * d.N * d.N * 16
        elif isinstance(d, L.DotTriDesc):
            macs += d.B * d.k1 * d.k1 * 16  # the reference's full bmm
        elif isinstance(d, L.FinalDesc):
            macs += d.B * sum(d.width[q] for q in range(d.nseg))
    params = sum(p.numel() for p in model.parameters())
    return macs / B, params


def get_model_latency(model, inputs, gpu, num_warmup_steps: int = 10, num_trials: int = 200):
    """(mean, std) seconds of an eval forward pass over the central 90 % of `num_trials` runs (train_utils.py:455-499)"""
    model = model.to(gpu)
    was_training = model.training
    model.eval()
    assert len(inputs) == 2, "Number of inputs should have exactly 2 items for RM models!"
    int_x, cat_x = inputs[0].to(gpu), inputs[1].to(gpu)
    samples = []
    with torch.no_grad():
        for i in range(num_warmup_steps + num_trials):
            t0 = time.time()
            model(int_x, cat_x)
            torch.cuda.synchronize(gpu)
            if i >= num_warmup_steps:
                samples.append(time.time() - t0)
    if was_training:
        model.train()
    samples = np.asarray(samples)
    lo, hi = np.percentile(samples, 5), np.percentile(samples, 95)
    kept = samples[(samples >= lo) & (samples <= hi)]
    return float(np.mean(kept)), float(np.std(kept))
