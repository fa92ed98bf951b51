"""SuperNet / SuperNetBlock — the reference's model API (nasrec/supernet/supernet.py) on top of the HIP engine.

Drop-in surface: constructor signature, `forward(int_feats, cat_feats, choices=None) -> logits [B,1]`,
`.choice`, path-sampling configuration and the global-`np.random` sampling order, mode setters, parameter getters,
`state_dict()` keys and `parameters()` order, lazy shapes fixed by the first forward (warm-up).  What differs is
*how* a forward runs: the whole choice is compiled into one launch plan (nasrec_amd/plan.py) and executed by
hand-written HIP kernels through the C-ABI; autograd sees one node for the whole network.

Gradient semantics of this `nn.Module` path are the reference's (dense `.grad` for every `nn.Embedding`, so the
unchanged `clip_grad_norm_` + `torch.optim.Adagrad` harness works).  The fast path used by `bench.py` is
`SuperNet.engine_train_step`, whose row-sparse table update is mathematically identical for weight_decay == 0.
"""
import copy
import json
from itertools import combinations
from typing import Any, List, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from .. import plan as P
from ..search_space import ops_config_lib, path_sampling_strategy_lib  # noqa: F401  (re-exported, supernet.py:134-207)
from ..utils.config import NUM_EMBEDDINGS_CRITEO
from .modules import (CleverMaskGenerator, CleverZeroTensorGenerator, DotProduct, ElasticLinear, ElasticLinear3D,  # noqa: F401
                      FactorizationMachine3D, SigmoidGating, Sum, Transformer, Zeros2D, Zeros3D)
from .utils import anypath_choice_fn, assert_valid_ops_config

_dense_unary_nodes = ["linear-2d", "zeros-2d"]
_dense_binary_nodes = ["sum", "sigmoid-gating"]
_dense_sparse_nodes = ["dot-product"]
_sparse_nodes = ["zeros-3d", "transformer", "linear-3d"]

assert_valid_ops_config(ops_config_lib)

DS_INTERACT_NUM_SPLITS = 8  # supernet.py:882


def _make_node(name, use_layernorm, dims, activation, embedding_dim, fixed):
    """supernet.py:53-113"""
    if name == "linear-2d":
        return ElasticLinear(use_layernorm=use_layernorm, max_dims_or_dims=dims, activation=activation, fixed=fixed)
    if name == "zeros-2d":
        return Zeros2D(use_layernorm=use_layernorm, max_dims_or_dims=dims, activation=activation, fixed=fixed)
    if name == "sigmoid-gating":
        return SigmoidGating(use_layernorm=use_layernorm, max_dims_or_dims=dims, activation=activation, fixed=fixed)
    if name == "sum":
        return Sum(use_layernorm=use_layernorm, max_dims_or_dims=dims, activation=activation, fixed=fixed)
    if name == "dot-product":
        return DotProduct(use_layernorm=use_layernorm, max_dims_or_dims=dims, embedding_dim=embedding_dim, fixed=fixed)
    if name == "zeros-3d":
        return Zeros3D(use_layernorm=use_layernorm, max_dims_or_dims=dims, fixed=fixed, embedding_dim=embedding_dim, activation=activation)
    if name == "transformer":
        return Transformer(use_layernorm=use_layernorm, max_dims_or_dims=dims, fixed=fixed, embedding_dim=embedding_dim, activation=activation)
    if name == "linear-3d":
        return ElasticLinear3D(use_layernorm=use_layernorm, max_dims_or_dims=dims, activation=activation, embedding_dim=embedding_dim, fixed=fixed)
    raise NotImplementedError("Block name {} is not supported in supernet!".format(name))


class _tracing_paused:
    """torch.jit.trace records every torch call it sees, also inside an autograd.Function's forward; the engine's host work (plan
    buffers carved out of byte arenas with `view(dtype)`, zero fills, copies into static buffers) is not part of the model's graph
    and trips the tracer's alias analysis.  Inside this block nothing is recorded; the Function itself stays the graph's one node."""

    def __enter__(self):
        self.state = torch._C._get_tracing_state()
        if self.state is not None:
            torch._C._set_tracing_state(None)

    def __exit__(self, *exc):
        if self.state is not None:
            torch._C._set_tracing_state(self.state)
        return False


class _SupernetFunction(torch.autograd.Function):
    """One autograd node for the whole network: forward = forward program, backward = backward program."""

    @staticmethod
    def forward(ctx, model, choice, int_x, cat_x, rows, *params):
        """rows: None, or (place_embedding_on_cpu) the looked-up embedding rows [B, Fs, 16] — then a differentiable input whose
        gradient torch carries back to the host tables"""
        eng = model._engine
        B = int(int_x.shape[0])
        with _tracing_paused():
            # (bf16 tables have no differentiable forward — SuperNet.forward refuses it: only torch.jit.trace arrives here with them,
            # and takes the forward-only plan)
            cp = eng.compile(choice, B, train=not eng.tables_bf16)
            eng.run_forward(cp, int_x, cat_x, rows=rows)
        out = cp.logits.view(B, 1).clone()  # (outside the pause: a result the tracer has not seen cannot become the node's output)
        ctx.has_rows = rows is not None
        cp.generation = getattr(cp, "generation", 0) + 1
        ctx.model, ctx.cp, ctx.cat_x, ctx.generation = model, cp, cat_x, cp.generation
        return out

    @staticmethod
    def backward(ctx, dlogits):
        model, cp = ctx.model, ctx.cp
        eng = model._engine
        if eng.tables_bf16:
            from .._lib import EngineError
            raise EngineError("bf16 tables have no backward through autograd: train them on the fused step (engine_train_step)")
        if getattr(cp, "evicted", False):
            raise RuntimeError("the launch plan of this forward was recycled for another sampled path before its backward ran (the "
                               "engine keeps 4 supernet plans): run backward before sampling further paths")
        if getattr(cp, "generation", 0) != ctx.generation:
            # the activations a backward needs live in the plan's static buffers (one plan per (choice, batch size)): a second
            # grad-enabled forward through the same plan has overwritten them
            raise RuntimeError("SuperNet.forward ran again with the same choice and batch size before the backward of an earlier "
                               "call: the saved activations of that call are gone; run backward (or sum the losses of separately "
                               "shaped calls) before the next forward")
        # only the last layer trains (set_mode_to_finelune_last_only): skip the network's backward altogether
        final_only = all(name.startswith("_final.") or not p.requires_grad for name, p in model._param_names)
        eng.run_backward(cp, dlogits, final_only=final_only)
        written = {"_final.weight", "_final.bias"} if final_only else set(cp.ctx.grad_params) | {"_final.weight", "_final.bias"}
        grads = []
        sg = cp.sparse0.grad_tensor().view(dlogits.shape[0], eng.Fs, 16) if (cp.sparse0.grad_written and not final_only) else None
        for name, p in model._param_names:
            if not p.requires_grad:
                grads.append(None)
            elif name.startswith("_embedding."):
                f = int(name.split(".")[1])
                if sg is None:
                    grads.append(None)
                else:  # dense gradient, exactly like nn.Embedding(sparse=False) (supernet.py:407)
                    grads.append(torch.zeros_like(p).index_add_(0, ctx.cat_x[:, f], sg[:, f]))
            elif name in written:
                grads.append(eng.grads[name].clone())
            else:
                grads.append(None)  # dead branch or unused parameter: autograd leaves .grad = None
        drows = sg.clone() if (ctx.has_rows and sg is not None) else None
        return (None, None, None, None, drows) + tuple(grads)


class ShardEmbedding(nn.Embedding):
    """This rank's rows [row_lo, row_hi) of a `whole_rows`-row table (SuperNet(table_sharding="row")).  Its values are always rows of a
    WHOLE table drawn the way the unsharded module draws it — one `normal_` of [whole_rows, dim] from the default generator of the
    weight's device, at the same point of the initialisation sequence — of which the rank keeps its range: with the ranks seeded alike
    (utils/dist.init_from_env) a sharded model starts, at any world size, from exactly the unsharded model's tables (and, the random
    stream having advanced by the same amount, from its dense weights too).  A subclass, so that the type-exact `init_weights` of the
    harness does not initialise a shard by itself (its fan would be the shard's: std sqrt(world) times too large, the same values on
    every rank); SuperNet.apply routes that call here."""

    def __init__(self, rows, dim, whole_rows, row_lo, row_hi, field):
        self.whole_rows, self.row_lo, self.row_hi, self.field = int(whole_rows), int(row_lo), int(row_hi), int(field)
        super().__init__(rows, dim)

    def _draw_whole_(self, std: float):
        with torch.no_grad():
            whole = torch.empty(self.whole_rows, self.weight.shape[1], dtype=self.weight.dtype, device=self.weight.device).normal_(0.0, std)
            self.weight.zero_()
            k = self.row_hi - self.row_lo
            if k > 0:
                self.weight[:k] = whole[self.row_lo:self.row_hi]

    def reset_parameters(self):  # nn.Embedding's constructor default: N(0, 1)
        if hasattr(self, "whole_rows"):
            self._draw_whole_(1.0)

    def xavier_normal_whole_(self):
        """torch.nn.init.xavier_normal_ of the WHOLE table: std = sqrt(2 / (whole_rows + dim))"""
        self._draw_whole_((2.0 / (self.whole_rows + self.weight.shape[1])) ** 0.5)


class SuperNet(nn.Module):
    """Top-level supernet (supernet.py:210-880)."""

    # engine_train_step runs weight decay and Adam / SGD inside the data-parallel exchange step when the process group has several
    # ranks (DataParallelStep's optimizer over the global batch): utils/train_utils._fused_step_applies may pick the fused route there
    engine_dp_optimizers = True

    def __init__(self, num_blocks: int, ops_config: Any, use_layernorm: bool, activation: str = "relu",
                 num_embeddings: List[int] = NUM_EMBEDDINGS_CRITEO, sparse_input_size: int = 26, embedding_dim: int = 16,
                 last_n_blocks_out: int = 1, path_sampling_strategy: str = "default", fixed: bool = False, fixed_choice: Any = None,
                 place_embedding_on_cpu: bool = False, anypath_choice: str = "uniform", supernet_training_steps: int = 0,
                 candidate_choices: Optional[List] = None, use_final_sigmoid: bool = False, table_sharding: Optional[str] = None,
                 matmul_precision: Optional[str] = None, table_dtype: torch.dtype = torch.float32):
        """table_dtype (not a reference argument): torch.float32, or torch.bfloat16 = the embedding tables are STORED as bf16 ([rows, 16]
        with 32-byte rows: half the memory and half the checkpoint).  They are initialised in fp32 exactly as ever and rounded to nearest
        even, one table at a time; the forward widens a row exactly and everything downstream stays fp32.  They train on the fused step
        with AdamAdagradTables(table_rowwise=True) alone (row-wise Adagrad in fp32 on the widened row, stored with stochastic rounding:
        utils/optim.stochastic_round_bf16); evaluation is the ordinary no-grad forward.  Refused with place_embedding_on_cpu,
        table_sharding="row" and use_final_sigmoid.
        matmul_precision (not a reference argument): "highest" | "high" | "medium"; None = the environment variable
        NASREC_MATMUL_PRECISION, else "highest".  What torch.set_float32_matmul_precision is to torch, for the engine: parameters,
        activations, optimizer state and checkpoints stay fp32 and products accumulate in fp32; "medium" permits the large-batch
        products of the Linear family — forward, input gradient, weight gradient; the throughput-regime GEMMs and, at batch >= 1024,
        the token-axis Linears (ElasticLinear3D, the token projections, _sparse_inp_proj) — to round their operands to bf16 on the way
        to the matrix cores, "high" to bf16 x 3 (hi + lo split, three products; the throughput GEMMs and the token-axis weight
        gradients take it, the token-axis forward and input-gradient products stay fp32).  Every other kernel, and every plan at batch
        <= 256, computes in fp32 whatever the value; "highest" is bit for bit the arithmetic without the argument.
        Under data parallelism every rank must pass the same value (utils/dist.py checks it at start-up).  use_amp=True keeps the torch
        route.
        table_sharding (not a reference argument): None = every process holds whole tables (the reference's layout); "row" = the
        rows of every table are split over the ranks of the process group (nasrec_amd/sharded_tables.py) — for tables that outgrow
        one GPU.  `_embedding[f]` then holds THIS rank's row range; `state_dict()` returns whole tables (a collective when world > 1);
        training goes through the fused engine step (Adagrad, weight decay 0), evaluation through the ordinary no-grad forward."""
        super().__init__()
        assert num_blocks >= 1, ValueError("Supernet must contain a minimum of 1 block, but found {}!".format(num_blocks))
        self._num_blocks = num_blocks
        self._ops_config = ops_config
        self._use_layernorm = use_layernorm
        self._activation = activation
        self._last_n_blocks_out = last_n_blocks_out
        self._sparse_input_size = sparse_input_size
        self._num_embeddings = num_embeddings
        self._embedding_dim = embedding_dim
        self._path_sampling_strategy = path_sampling_strategy
        self._macro_path_sampling_strategy = path_sampling_strategy_lib[path_sampling_strategy]["macro"]
        self._candidate_choices = candidate_choices
        self._fixed = fixed
        assert table_sharding in (None, "none", "row"), "table_sharding must be None or 'row'"
        self._table_sharding = "row" if table_sharding == "row" else None
        from .._lib import matmul_precision_name
        self._matmul_precision = matmul_precision_name(matmul_precision)  # (ValueError on anything else)
        self._sharded = self._sharded_ops = None
        if table_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("table_dtype %r: the tables are stored as torch.float32 or torch.bfloat16" % (table_dtype,))
        self._table_dtype = table_dtype
        if table_dtype == torch.bfloat16:
            for flag, on in (("place_embedding_on_cpu", place_embedding_on_cpu), ("table_sharding='row'", self._table_sharding == "row"),
                             ("use_final_sigmoid", use_final_sigmoid)):
                if on:
                    raise ValueError("table_dtype=torch.bfloat16 with %s: bf16 tables are whole tables on one device, read by the "
                                     "engine's gather and trained by its fused step" % flag)
            if embedding_dim != 16:
                raise ValueError("table_dtype=torch.bfloat16 needs embedding_dim 16 (32-byte rows), got %d" % embedding_dim)
        self._embedding = self._embedding_layers(sparse_input_size, num_embeddings, embedding_dim)
        self._final = nn.LazyLinear(1)
        self._final_sigmoid = nn.Sigmoid() if use_final_sigmoid else None
        self._place_embedding_on_cpu = place_embedding_on_cpu
        self._supernet_training_steps = supernet_training_steps
        self._anypath_choice_fn = anypath_choice_fn[anypath_choice]
        self._supernet_train_steps_counter = -1
        self._device_args = None
        if self._fixed and fixed_choice is not None:
            self.choice = fixed_choice
            self.macro_last_choice = fixed_choice["macro"]
        else:
            self.choice = []
            self.macro_last_choice = None
        if self._fixed:
            assert self._macro_path_sampling_strategy == "fixed-path", ValueError(
                "'fixed_path_strategy' should be explicitly specified when 'fixed' option is True.")
        blocks = []
        for idx in range(num_blocks):
            oc = ops_config[idx] if isinstance(ops_config, list) else ops_config
            blocks.append(SuperNetBlock(
                oc, use_layernorm, int(max(oc["dense_node_dims"])), int(max(oc["sparse_node_dims"])), embedding_dim, activation,
                path_sampling_strategy=path_sampling_strategy_lib[path_sampling_strategy]["micro"], fixed=fixed,
                fixed_micro_choice=None if (fixed_choice is None) or (not fixed) else fixed_choice["micro"][idx],
                anypath_choice=anypath_choice, supernet_training_steps=supernet_training_steps, sparse_input_size=sparse_input_size))
        self._blocks = nn.ModuleList(blocks)
        for m in self.modules():  # operators run on their own (opexec.run) take their owner's precision
            m.__dict__["_matmul_precision"] = self._matmul_precision
        # engine state (not part of the reference API)
        self._engine = None
        self._materialized = False
        self._param_names = []

    # ------------------------------------------------------------------------------------------------ parameters
    def get_dense_parameters(self):
        return list(self._blocks.parameters()) + list(self._final.parameters())

    def get_sparse_parameters(self):
        return list(self._embedding.parameters())

    def load_embeddings_from_dlrm(self, dlrm_ckpt_path=None):
        """supernet.py:368-383"""
        if dlrm_ckpt_path is not None:
            checkpoint = torch.load(dlrm_ckpt_path, map_location=torch.device("cpu"))
            assert "model_state_dict" in checkpoint.keys(), "Please use the DLRM checkpoint to load!"
            checkpoint = checkpoint["model_state_dict"]
            with torch.no_grad():
                for idx in range(len(self._embedding)):
                    w = self._embedding[idx].weight
                    w.copy_(checkpoint["embedding_layers.{}.weight".format(idx)].to(w.device))

    def _embedding_layers(self, sparse_input_size, num_embeddings, embedding_dim):
        if self._table_sharding == "row":
            out = []
            for i in range(sparse_input_size):
                lo, hi, rows = self._shard_rows(num_embeddings[i])
                out.append(ShardEmbedding(rows, embedding_dim, whole_rows=num_embeddings[i], row_lo=lo, row_hi=hi, field=i))
            return nn.ModuleList(out)
        out = []
        for i in range(sparse_input_size):
            emb = nn.Embedding(num_embeddings[i], embedding_dim)  # (nn.Embedding's own fp32 draw, whatever the storage type)
            if self._table_dtype == torch.bfloat16:
                emb.weight.data = emb.weight.data.to(torch.bfloat16)  # (nearest even; one table at a time: the peak overhead is one table)
            out.append(emb)
        return nn.ModuleList(out)

    def apply(self, fn):
        """nn.Module.apply; with row-sharded tables, the reference's `init_weights` (train_utils.py:70-89: xavier_normal_ on every
        nn.Embedding, type-exact) initialises the shards too — each as rows [lo, hi) of a WHOLE table drawn with the whole table's fan
        at the shard's place in the traversal (ShardEmbedding), so the random stream is consumed exactly as by the unsharded model."""
        if self._table_sharding == "row" and getattr(fn, "__name__", "") == "init_weights":
            def routed(m, _fn=fn):
                if type(m) is ShardEmbedding:
                    m.xavier_normal_whole_()
                else:
                    _fn(m)
            return super().apply(routed)
        if self._table_dtype == torch.bfloat16 and getattr(fn, "__name__", "") == "init_weights":
            # bf16 tables: the same xavier_normal_ draw in fp32 (the random stream is consumed as by the fp32 model), rounded to nearest
            # even into the table, one table at a time
            def rounded(m, _fn=fn):
                if type(m) is nn.Embedding and m.weight.dtype == torch.bfloat16:
                    with torch.no_grad():
                        m.weight.copy_(torch.nn.init.xavier_normal_(torch.empty(m.weight.shape, dtype=torch.float32, device=m.weight.device)))
                else:
                    _fn(m)
            return super().apply(rounded)
        return super().apply(fn)

    @staticmethod
    def _shard_rows(n):
        """(first row, end row, rows held) of this rank's range of an n-row table — RowShardedTables' placement: ceil(n / world)
        rows per rank; an empty range keeps one unused row so that every pointer is valid"""
        import math
        import torch.distributed as dist
        rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
        rp = max(1, math.ceil(int(n) / world))
        lo, hi = min(int(n), rank * rp), min(int(n), (rank + 1) * rp)
        return lo, hi, max(hi - lo, 1)

    def state_dict(self, *args, **kwargs):
        """row-sharded tables: `_embedding.f.weight` is returned WHOLE (all-gather of the shards — a collective when world > 1: every
        rank must call it), so checkpoints keep the reference's keys and shapes whatever the placement.  Fused steps with decoupled
        weight decay leave table rows owing their decay: they are paid first (engine_flush_decay)"""
        self.engine_flush_decay()
        sd = super().state_dict(*args, **kwargs)
        if self._table_sharding == "row" and self._sharded is not None and self._sharded.world > 1:
            prefix = kwargs.get("prefix", args[1] if len(args) > 1 else "")
            for f in range(self._sparse_input_size):
                sd["%s_embedding.%d.weight" % (prefix, f)] = self._sharded.whole_table(f)
        return sd

    def load_state_dict(self, state_dict, *args, **kwargs):
        self.engine_flush_decay()  # (what fused steps with decoupled weight decay left owing is paid on the OLD weights, not the loaded ones)
        if self._table_sharding == "row":  # whole tables in, this rank's rows kept
            state_dict = dict(state_dict)
            for f in range(self._sparse_input_size):
                k = "_embedding.%d.weight" % f
                if k in state_dict and int(state_dict[k].shape[0]) == int(self._num_embeddings[f]):
                    lo, hi, rows = self._shard_rows(self._num_embeddings[f])
                    t = state_dict[k][lo:hi]
                    if hi - lo < rows:
                        t = torch.cat([t, torch.zeros(rows - (hi - lo), t.shape[1], dtype=t.dtype, device=t.device)])
                    state_dict[k] = t
        return super().load_state_dict(state_dict, *args, **kwargs)

    # ------------------------------------------------------------------------------------------------ sampling
    def configure_path_sampling_strategy(self, strategy):
        assert strategy in ["full-path", "single-path", "any-path", "fixed-path", "evo-2shot-path", "default"], \
            "Strategy {} is not found!".format(strategy)
        self.__dict__.pop("_fixed_resolved", None)
        self._path_sampling_strategy = strategy
        self._macro_path_sampling_strategy = path_sampling_strategy_lib[strategy]["macro"]
        for block in self._blocks:
            block._micro_path_sampling_strategy = path_sampling_strategy_lib[strategy]["micro"]

    def _thresh(self):
        c, n = self._supernet_train_steps_counter, self._supernet_training_steps
        return 1.0 - c / (n + 1e-10) if (c < n and c > 0) else 0  # supernet.py:446-453

    def _get_choice(self):
        """supernet.py:432-511 — draws from the global np.random stream in the reference's order."""
        nb = self._num_blocks
        s = self._macro_path_sampling_strategy
        thresh = self._thresh()
        if s == "single-path":
            choice = ([self._get_full_path_choice(1 + i) for i in range(nb)] if np.random.random() < thresh
                      else [self._get_single_path_choice(1 + i) for i in range(nb)])
        elif s == "full-path":
            choice = [self._get_full_path_choice(1 + i) for i in range(nb)]
        elif s == "any-path":
            choice = ([self._get_full_path_choice(1 + i) for i in range(nb)] if np.random.random() < thresh
                      else [self._get_any_path_choice(1 + i) for i in range(nb)])
        elif s == "fixed-path" and self.macro_last_choice is None:
            if getattr(self, "_fixed_path_called", False):
                raise ValueError("Error! fixed-path choice should be generated only once for each supernet!")
            self._fixed_path_called = True
            choice = [self._get_fixed_path_choice(1 + i) for i in range(nb)]
        elif s == "fixed-path":
            choice = self.macro_last_choice
        elif s == "evo-2shot-path":
            assert self._candidate_choices is not None, "You must specify self._candidate_choices before using 'evo-2shot-path'!"
            cand = self._candidate_choices[np.random.randint(len(self._candidate_choices))]["choice"]
            for i in range(nb):
                self._blocks[i].configure_choice(cand["micro"][i])
            choice = cand["macro"]
        else:
            raise NotImplementedError("Path strategy {} is not supported!".format(s))
        if s != "full-path":
            self.macro_last_choice = choice
        return choice

    def _get_single_path_choice(self, n: int):
        """supernet.py:723-736 (the pair of gating inputs is drawn first)"""
        bi = np.random.choice(n, 2)
        return {"dense_idx": [np.random.choice(n)], "sparse_idx": [np.random.choice(n)],
                "dense_left_idx": [bi[0]], "dense_right_idx": [bi[1]]}

    def _any_like(self, n: int, fn):
        nd, ns = fn(n), fn(n)
        bi = np.random.choice(n, 2)
        return {"dense_idx": np.random.choice(n, nd, replace=False).reshape(-1).tolist(),
                "sparse_idx": np.random.choice(n, ns, replace=False).reshape(-1).tolist(),
                "dense_left_idx": bi[:1].reshape(-1).tolist(), "dense_right_idx": bi[1:].reshape(-1).tolist()}

    def _get_any_path_choice(self, n: int):
        """supernet.py:738-770"""
        return self._any_like(n, self._anypath_choice_fn)

    def _get_fixed_path_choice(self, n: int):
        """supernet.py:772-812 (always the uniform count sampler)"""
        return self._any_like(n, anypath_choice_fn["uniform"])

    def _get_full_path_choice(self, n: int):
        """supernet.py:814-824"""
        return {k: np.arange(n) for k in ("dense_idx", "sparse_idx", "dense_left_idx", "dense_right_idx")}

    def get_all_subnet_macro_choices(self, block_idx: int):
        """supernet.py:670-712"""
        m = 1 + block_idx
        out = {"dense_left_idx": [], "dense_right_idx": [], "dense_idx": [], "sparse_idx": []}
        for k in range(1, m + 1):
            out["dense_idx"] += list(combinations(list(range(m)), k))
        for k in range(1, m + 1):
            out["sparse_idx"] += list(combinations(list(range(m)), k))
        for k in range(1, min(2, m + 1)):
            out["dense_left_idx"] += list(combinations(list(range(m)), k))
            out["dense_right_idx"] += list(combinations(list(range(m)), k))
        return out

    def get_all_subnet_choices(self):
        """supernet.py:714-721"""
        out = {"macro": [], "micro": []}
        for i in range(self._num_blocks):
            out["macro"].append(self.get_all_subnet_macro_choices(i))
            out["micro"].append(self._blocks[i].get_all_subnet_micro_choices())
        return out

    def configure_choice(self, choice: Any):
        """supernet.py:842-848"""
        self.__dict__.pop("_fixed_resolved", None)
        self.choice = copy.deepcopy(choice)
        self.macro_last_choice = copy.deepcopy(choice["macro"])
        for idx in range(self._num_blocks):
            self._blocks[idx].configure_choice(choice["micro"][idx])

    # ------------------------------------------------------------------------------------------------ modes
    def set_mode_to_finelune_last_only(self):
        self._embedding.requires_grad_(False)
        self._blocks.requires_grad_(False)
        self._final.requires_grad_(True)

    def set_mode_to_normal_mode(self):
        self._embedding.requires_grad_(True)
        self._blocks.requires_grad_(True)
        self._final.requires_grad_(True)

    def set_mode_to_layernorm_calibrate(self):
        self._embedding.requires_grad_(False)
        self._blocks.requires_grad_(False)
        self._final.requires_grad_(False)
        for _, m in self._blocks.named_modules():
            if isinstance(m, nn.LayerNorm):
                m.requires_grad_(True)

    def set_mode_to_finetune_no_embedding(self):
        self._embedding.requires_grad_(False)
        self._blocks.requires_grad_(True)
        self._final.requires_grad_(True)

    # ------------------------------------------------------------------------------------------------ engine glue
    def _net_config(self):
        return P.NetConfig(self._num_blocks, self._ops_config, self._use_layernorm, self._activation, self._embedding_dim,
                           fixed=self._fixed, last_n_blocks_out=self._last_n_blocks_out,
                           use_final_sigmoid=self._final_sigmoid is not None)

    def _warm_choice(self):
        if self._fixed:
            return {"macro": self.macro_last_choice, "micro": [b._fixed_micro_choice for b in self._blocks]}
        return P.full_path_choice(self._net_config())

    def _materialize(self, Fd: int):
        """Fix every lazy shape exactly as the reference's warm-up forward does (train_utils.py:392-433): LazyLinear ->
        nn.Linear with the inferred in_features (created in forward order, so the RNG stream is consumed in the
        reference's order), projections whose input already has the target width are dropped."""
        if self._materialized:
            return
        cfg = self._net_config()
        shapes = P.infer_param_shapes(cfg, self._warm_choice(), Fd, self._sparse_input_size, self._num_embeddings)
        self._shapes = shapes
        from ..opexec import materialize_lazies
        materialize_lazies(self, shapes, delete_unused=True, device=self._embedding[0].weight.device)
        got = {k: tuple(v.shape) for k, v in nn.Module.state_dict(self).items()}
        want = {k: tuple(v) for k, v in shapes.items()}
        if self._table_sharding == "row":  # this rank's row ranges
            for f in range(self._sparse_input_size):
                want["_embedding.%d.weight" % f] = (self._shard_rows(self._num_embeddings[f])[2], self._embedding_dim)
        assert got == want, "materialised module tree does not match the inferred parameter set"
        self._materialized = True

    def _bind_engine(self, device):
        from ..engine import SupernetEngine
        params = dict(self.named_parameters())
        Fd = self._Fd
        host = bool(self._place_embedding_on_cpu) or self._table_sharding == "row"
        eng = SupernetEngine(self._net_config(), Fd, self._sparse_input_size, self._num_embeddings, device=device,
                             warm_choice=self._warm_choice(), host_embedding=host, matmul_precision=self._matmul_precision,
                             tables=None if host else [params["_embedding.%d.weight" % f].data for f in range(self._sparse_input_size)])
        eng.load_params({k: v.data for k, v in params.items() if not k.startswith("_embedding.")})
        # re-point every dense nn.Parameter at the engine's flat arena (optimizers update in place; kernels read the
        # same bytes each step — SURVEY §8b "no engine-side copy of weights may go stale")
        for name, p in params.items():
            if not name.startswith("_embedding."):
                p.data = eng.params[name]
        self._engine = eng
        self._sharded = self._sharded_ops = None
        self.__dict__.pop("_sharded_step", None)
        if self._table_sharding == "row":
            # the engine holds no table (host_embedding mode: the looked-up rows come with the batch); this rank's row ranges are the
            # nn.Embedding weights themselves, adopted by RowShardedTables; gather / dedup / row-Adagrad run on them with the
            # engine's kernels (EngineShardedOps)
            from ..sharded_tables import EngineShardedOps, RowShardedTables
            self._sharded = RowShardedTables(self._num_embeddings, device,
                                             shards=[params["_embedding.%d.weight" % f].data for f in range(self._sparse_input_size)])
            self._sharded_ops = EngineShardedOps(eng)
        self._param_names = [(n, p) for n, p in self.named_parameters() if not (host and n.startswith("_embedding."))]
        st = self.__dict__.pop("_stashed_opt_state", None)
        if st is not None:  # accumulators of the engine this one replaces
            if not eng.tables_bf16:  # (bf16 tables have no [rows, 16] state)
                eng._ensure_table_state()
            for n, t in st.items():
                if n.startswith("_embedding.") and eng.table_state is None:
                    continue
                tgt = eng.table_state[int(n.split(".")[1])] if n.startswith("_embedding.") else eng.state.get(n)
                if tgt is not None and tuple(tgt.shape) == tuple(t.shape):
                    tgt.copy_(t.to(tgt.device))

    def _ensure_engine(self, int_feats):
        if not self._materialized:
            self._Fd = int(int_feats.shape[1])
            self._materialize(self._Fd)
        dev = int_feats.device
        if dev.type != "cuda":
            from .._lib import EngineError
            raise EngineError("SuperNet.forward runs on the HIP engine: move the model and its inputs to a GPU "
                              "(there is no CPU fallback)")
        if self._engine is None or self._engine.device != dev:
            if self._final.weight.device != dev:
                self.to(dev)
            self._bind_engine(dev)

    def __deepcopy__(self, memo):
        self.engine_flush_decay()  # (the copy holds every table row current)
        eng, names, sh = self._engine, self._param_names, (self._sharded, self._sharded_ops, self.__dict__.pop("_sharded_step", None))
        # (the data-parallel step cached by engine_train_step drives THIS model's engine: the copy builds its own when it trains)
        dp = self.__dict__.pop("_dp_step", None)
        self._engine, self._param_names, self._sharded, self._sharded_ops = None, [], None, None
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                new.__dict__[k] = copy.deepcopy(v, memo)
        finally:
            self._engine, self._param_names, self._sharded, self._sharded_ops = eng, names, sh[0], sh[1]
            if sh[2] is not None:
                self.__dict__["_sharded_step"] = sh[2]
            if dp is not None:
                self.__dict__["_dp_step"] = dp
        return new  # the copy re-binds its own engine at its next forward

    def to(self, *args, **kwargs):
        if self._place_embedding_on_cpu:
            # supernet.py:826-840: every layer but the embeddings follows the device
            self._engine = None
            for name, child in self.named_children():
                if name != "_embedding":
                    child.to(*args, **kwargs)
            self._device_args = args
            return self
        eng = self._engine
        self.engine_flush_decay()  # (the copy that moves must hold every table row current)
        before = [p.data_ptr() for p in self.parameters() if not isinstance(p, nn.parameter.UninitializedParameter)] if eng is not None else None
        out = super().to(*args, **kwargs)
        if eng is not None:
            after = [p.data_ptr() for p in self.parameters() if not isinstance(p, nn.parameter.UninitializedParameter)]
            if before != after:  # storage really moved (device / dtype change): re-bind lazily
                self._stash_engine_state()
                self._engine = None
        return out

    def _stash_engine_state(self):
        """keep the fused path's Adagrad accumulators across a re-bind (they live only in the engine otherwise)"""
        eng = self._engine
        if eng is None:
            return
        st = {n: t.detach().clone() for n, t in eng.state.items()}
        if eng.table_state is not None:
            for f, t in enumerate(eng.table_state):
                st["_embedding.%d.weight" % f] = t.detach().clone()
        self._stashed_opt_state = st

    # ------------------------------------------------------------------------------------------------ forward
    def _resolve_choice(self, choices):
        """choice bookkeeping of supernet.py:513-529,585 / 605-618,650 without running anything"""
        d = self.__dict__
        if self._fixed and choices is None:
            # a fixed sub-network resolves to the same choice every time: after the first call the step hands back the SAME object
            # (the engine recognises it by identity and skips the plan-cache key), without walking the seven blocks and without
            # nn.Module.__setattr__ (2 us per assignment) — the harness calls this once per 0.3 ms training step
            hit = d.get("_fixed_resolved")
            if hit is not None and hit[0] is self.macro_last_choice and self._macro_path_sampling_strategy == "fixed-path":
                d["choice"] = hit[1]
                return hit[1]
        if not self._fixed:
            self._supernet_train_steps_counter += 1
        self.choice = {"micro": [], "macro": []}
        macro = self._get_choice() if choices is None else choices["macro"]
        self.choice["macro"] = macro
        for i, blk in enumerate(self._blocks):
            # the reference hands the *whole* micro list to every block (supernet.py:574,583), which cannot work;
            # an explicit `choices` is honoured per block here
            self.choice["micro"].append(blk._resolve_choice(None if choices is None else choices["micro"][i]))
        if self._fixed and choices is None and self._macro_path_sampling_strategy == "fixed-path" and self.macro_last_choice is macro:
            d["_fixed_resolved"] = (macro, self.choice)
        return self.choice

    def forward(self, int_feats: torch.Tensor, cat_feats: torch.Tensor, choices=None):
        choice = self._resolve_choice(choices)  # host-side bookkeeping first: a fixed net may sample its path here
        self._ensure_engine(int_feats)
        eng = self._engine
        rows = None
        if self._table_sharding == "row":
            if torch.is_grad_enabled() and any(p.requires_grad for _, p in self._param_names) and not torch.jit.is_tracing():
                from .._lib import EngineError
                raise EngineError("row-sharded tables: train through the fused engine step (engine_train_step: Adagrad, weight decay 0 — "
                                  "the route train_and_test_one_epoch takes for the published recipes); a differentiable forward "
                                  "would need the row gradients routed back to their owners by torch.autograd, which is not built. "
                                  "Evaluate under torch.no_grad().")
            rows, _ = self._sharded.lookup(cat_feats, lambda idx: self._sharded_ops.gather(self._sharded, idx))
            out = eng.forward(int_feats, cat_feats, choice, rows=rows).clone()
            return self._final_sigmoid(out) if self._final_sigmoid is not None else out
        if self._place_embedding_on_cpu:
            # supernet.py:418-428: ids to the host, lookup in host memory, rows to the device ("10~100x slow down", :253-254) — the
            # one place where the reference itself runs the stem on the CPU; everything downstream stays on the engine
            ids = cat_feats.cpu()
            rows = torch.stack([emb(ids[:, f]) for f, emb in enumerate(self._embedding)], dim=1).to(int_feats.device)
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for _, p in self._param_names)
        if needs_grad and self._table_dtype == torch.bfloat16 and not torch.jit.is_tracing():
            from .._lib import EngineError
            raise EngineError("bf16 tables: train through the fused engine step (engine_train_step with AdamAdagradTables("
                              "table_rowwise=True) — the route train_and_test_one_epoch takes for --table-dtype bf16); a differentiable "
                              "forward would hand torch.autograd a dense bf16 gradient the size of every table, which is neither the "
                              "rule (fp32 row-wise Adagrad, stored with stochastic rounding) nor affordable.  Evaluate under "
                              "torch.no_grad().")
        # torch.jit.trace (TensorBoard's writer.add_graph, main_train.py:137 / train_supernet.py:192; fvcore's FLOP counter,
        # train_utils.py:444-452): the network traces as ONE opaque node (prim::PythonOp) that consumes the inputs and every
        # parameter — the no-grad route would hand the tracer a result that depends on nothing it has seen
        if needs_grad or torch.jit.is_tracing():
            out = _SupernetFunction.apply(self, choice, int_feats, cat_feats, rows, *[p for _, p in self._param_names])
        else:
            out = eng.forward(int_feats, cat_feats, choice, rows=rows).clone()
        if self._final_sigmoid is not None:
            out = self._final_sigmoid(out)
        return out

    def fixed_forward(self, int_feats: torch.Tensor, cat_feats: torch.Tensor, choices: Any):
        return self.forward(int_feats, cat_feats, choices)

    def engine_train_step(self, int_feats, cat_feats, y, lr: float, clip: Optional[float] = 5.0, eps: float = 1e-2, graph=None,
                          weight_decay: float = 0.0, no_reg_param_name: Optional[str] = None, optim=None, ema_decay: float = 0.0,
                          decoupled_wd: float = 0.0, cowclip=None):
        """Fused step on the engine (forward, BCE, backward, clip_grad_norm_, Adagrad with row-sparse table update):
        the counterpart of train_utils.py:262-286 for optimizer == Adagrad (torch's own weight_decay == 0).  weight_decay != 0: the loss
        is BCE + get_l2_loss(self, weight_decay, no_reg_param_name) — every regularised parameter and every table row is decayed
        (engine_last_l2 = that term on the pre-step weights).  optim: an OptimSpec (nasrec_amd/optim_spec.py) of torch.optim.Adam / SGD
        replaces Adagrad (eps unused) — every table row moves every step, or with sparse_rows (utils/optim.RowSparseAdam) or
        table_kind "adagrad" / "rowwise_adagrad" / "rowwise_adagrad_bf16" (utils/optim.AdamAdagradTables: Adagrad on the tables at lr * table_lr_scale)
        or "rowwise_adam" (utils/optim.RowwiseSparseAdam: one second moment per table row) only the
        batch's rows, which weight decay must then leave out; engine_bind_optimizer / engine_sync_optimizer_steps share its
        state with the torch optimizer.  Both need whole tables; under data parallelism they run in the exchange step's optimizer over
        the global batch (nasrec_amd/parallel.py).  ema_decay != 0: the step also averages every parameter (utils/optim.WeightEMA's
        update, in the engine: engine_bind_ema / engine_sync_ema share the average with a WeightEMA) — one process, whole tables, and an
        optimizer whose tables move in the batch's rows only (Adagrad, row-sparse Adam, RMSprop; no regularised table).
        decoupled_wd != 0: utils/optim.DecoupledWeightDecay's apply(lr) in front of the update, in the engine — the parameters
        get_l2_loss's rule selects (no_reg_param_name) and the step reaches take p (1 - lr decoupled_wd); a table row outside the batch
        rests and pays the factors it missed when it is next in a batch or read.  Same conditions as ema_decay, and, when the decay
        reaches the tables, neither ema_decay nor an L2 term on the tables.  Between fused steps `_embedding.<f>.weight` holds rows that
        still owe: a RAW read of it needs engine_flush_decay() first.  forward (outside this step), state_dict,
        engine_sync_optimizer_steps and a bound DecoupledWeightDecay's apply (engine_bind_decay) flush by themselves.
        cowclip = (r, zeta): utils/optim.CowClip's apply(cat_feats) in front of the update, in the engine (csrc/cowclip.hip): the batch's
        summed table rows are held to cnt max(r ||w||, zeta) behind the global clip, under every optimizer.  One process, whole fp32
        tables on the device, no L2 term on the tables; engine_cowclip_stats() counts the rows touched and clipped."""
        if self._place_embedding_on_cpu:
            from .._lib import EngineError
            raise EngineError("engine_train_step needs the tables on the device; with place_embedding_on_cpu use forward / backward "
                              "and a torch optimizer")
        if cowclip is not None:
            import torch.distributed as dist
            from .._lib import EngineError
            if self._table_sharding == "row":
                raise EngineError("cowclip in the fused step needs whole tables: row-sharded tables hold one rank's rows (CowClip.apply() "
                                  "on the torch route needs whole tables too)")
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise EngineError("cowclip in the fused step covers one process: under data parallelism the counts would have to be global")
            cowclip = (float(cowclip[0]), float(cowclip[1]))
        if ema_decay or decoupled_wd:
            import torch.distributed as dist
            if self._table_sharding == "row" or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
                from .._lib import EngineError
                if decoupled_wd:
                    raise EngineError("the fused decoupled weight decay covers one process with whole tables: use "
                                      "DecoupledWeightDecay.apply() on the torch route")
                raise EngineError("the fused weight EMA covers one process with whole tables: use WeightEMA.update() on the torch route")
        choice = self._resolve_choice(None)
        self._ensure_engine(int_feats)
        self._engine._refuse_swapped("engine_train_step")
        # (graph=None: a fixed sub-network's step is replayed as a graph.  Launching the level-scheduled program instead is ~6 us faster per
        # step when the host does nothing else — bench.py, engine.prefers_graph — but this harness's host has a data pipe and a Python
        # loop to run: measured on TSV shards 832 k rows/s launched against 896 k replayed)
        graph = self._fixed if graph is None else graph
        d = self.__dict__  # (plain bookkeeping: nn.Module.__setattr__ costs 2 us per assignment)
        d["_engine_steps"] = d.get("_engine_steps", 0) + 1
        d["_last_step_batch"] = int(int_feats.shape[0])
        from ..optim_spec import OptimSpec
        spec = OptimSpec.of(eps, weight_decay, no_reg_param_name, optim, ema_decay, decoupled_wd)
        d["_last_step_key"] = (choice, clip, eps, graph, spec)
        d["_last_step_cowclip"] = cowclip
        d["_last_step_last_layer"] = False
        opt_kw = {}
        if spec.wd or spec.moments:
            if self._table_sharding == "row":
                from .._lib import EngineError
                raise EngineError("weight decay, Adam and SGD in the fused step need whole tables: row-sharded tables train them "
                                  "through the torch route")
            opt_kw = dict(weight_decay=spec.wd, no_reg_param_name=spec.no_reg, optim=optim)
        if cowclip is not None:  # (refused above for row-sharded tables and several ranks: from here on the one-process step)
            opt_kw = dict(opt_kw, cowclip=cowclip)
        if spec.dwd:
            return self._engine.train_step(int_feats, cat_feats, y, lr, choice, clip, eps, graph=graph, ema=spec.ema, weight_decay=spec.wd,
                                           no_reg_param_name=spec.no_reg, optim=optim, decoupled_wd=spec.dwd, cowclip=cowclip)
        if spec.ema:
            return self._engine.train_step(int_feats, cat_feats, y, lr, choice, clip, eps, graph=graph, ema=spec.ema, **opt_kw)
        if self._table_sharding == "row":
            from ..sharded_tables import ShardedTableStep
            st = self.__dict__.get("_sharded_step")
            key = (id(self._engine), int(int_feats.shape[0]), clip, eps)
            if st is None or st[0] != key:
                st = (key, ShardedTableStep(self._sharded_ops, self._sharded, int(int_feats.shape[0]), clip=clip, eps=eps))
                self.__dict__["_sharded_step"] = st
            return st[1].step(int_feats, cat_feats, y, lr, choice=choice)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            # one process per GPU (utils/dist.py): the batch is this rank's share of the global batch; same path on every rank
            from ..parallel import DataParallelStep
            dp = self.__dict__.get("_dp_step")
            key = (id(self._engine), int(int_feats.shape[0]), clip, eps, graph, spec)
            if dp is None or dp[0] != key:
                dp = (key, DataParallelStep(self._engine, choice if self._fixed else None, int(int_feats.shape[0]), clip=clip, eps=eps, graph=graph,
                                            **opt_kw))
                self.__dict__["_dp_step"] = dp
            return dp[1].step(int_feats, cat_feats, y, lr, choice=None if self._fixed else choice)
        return self._engine.train_step(int_feats, cat_feats, y, lr, choice, clip, eps, graph=graph, **opt_kw)

    def _last_layer_only(self):
        """set_mode_to_finelune_last_only: every parameter outside _final is frozen"""
        return all(n.startswith("_final.") or not p.requires_grad for n, p in self.named_parameters()) and \
            all(p.requires_grad for n, p in self.named_parameters() if n.startswith("_final."))

    def engine_last_layer_step(self, int_feats, cat_feats, y, lr: float, clip: Optional[float] = 5.0, eps: float = 1e-2,
                               weight_decay: float = 0.0, no_reg_param_name: Optional[str] = None, optim=None):
        """Fused step of last-layer fine-tuning (the searcher's candidate scoring, set_mode_to_finelune_last_only): forward, BCE,
        d loss / d _final, clip_grad_norm_ and the optimizer — Adagrad (eps), or an OptimSpec of torch.optim.Adam / SGD — on
        _final.{weight, bias} alone, in the engine (SupernetEngine.last_layer_step).  weight_decay: get_l2_loss's gradient on
        _final.weight (the frozen parameters take none).  Returns the (device) loss.  One process with whole tables only;
        engine_bind_optimizer(optimizer, last_layer=True) / engine_sync_optimizer_steps share the state with the torch optimizer."""
        from .._lib import EngineError
        if self._place_embedding_on_cpu:
            raise EngineError("engine_last_layer_step needs the tables on the device; with place_embedding_on_cpu use forward / backward "
                              "and a torch optimizer")
        import torch.distributed as dist
        if self._table_sharding == "row" or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise EngineError("the fused last-layer step covers one process with whole tables: row-sharded tables and data-parallel "
                              "runs train the last layer through the torch route")
        if not self._last_layer_only():
            raise EngineError("engine_last_layer_step trains _final alone: every other parameter must be frozen "
                              "(set_mode_to_finelune_last_only); use engine_train_step or the torch route")
        choice = self._resolve_choice(None)
        self._ensure_engine(int_feats)
        d = self.__dict__
        d["_last_layer_steps"] = d.get("_last_layer_steps", 0) + 1
        d["_last_step_batch"] = int(int_feats.shape[0])
        d["_last_step_last_layer"] = True  # (engine_last_logits: the plan the engine ran, SupernetEngine.last_layer_plan)
        return self._engine.last_layer_step(int_feats, cat_feats, y, lr, choice, clip, eps, weight_decay=float(weight_decay or 0.0),
                                            no_reg_param_name=no_reg_param_name, optim=optim, graph=self._fixed)

    def engine_last_logits(self):
        """logits [B, 1] of the most recent engine_train_step (what `model(int_x, cat_x)` returned inside that step)"""
        B = self._last_step_batch
        if self.__dict__.get("_last_step_last_layer"):  # (engine_last_layer_step)
            return self._engine.last_layer_plan.logits.view(B, 1)
        choice, clip, eps, graph, spec = self._last_step_key
        if self._table_sharding == "row":
            return self._sharded_ops.cp.logits.view(B, 1)
        dp = self.__dict__.get("_dp_step")
        if dp is not None and dp[1].exchange:
            return dp[1].last_plan().logits.view(B, 1)
        cp = self._engine.compile(choice, B, train=True, clip=clip, eps=eps, graph=graph, spec=spec, cowclip=self.__dict__.get("_last_step_cowclip"))
        return cp.logits.view(B, 1)

    def engine_last_l2(self):
        """(device) get_l2_loss(self, weight_decay, no_reg_param_name) of the pre-step weights of the most recent engine_train_step —
        the `L2:` the reference prints (train_utils.py:262-266); exactly 0 when that step had weight_decay == 0"""
        key = self.__dict__.get("_last_step_key")
        wd = key[-1].wd if key is not None else 0.0
        eng = self._engine
        if not wd or getattr(eng, "wd_l2_sumsq", None) is None:
            return torch.zeros((), device=self._final.weight.device)
        return (eng.wd_l2_sumsq[0] * wd).to(torch.float32)

    def engine_bind_optimizer(self, optimizer, last_layer: bool = False):
        """Share the optimizer state between a torch optimizer and the engine.  Adagrad: existing `sum` state (a resumed checkpoint) is
        copied into the engine's accumulators, then `optimizer.state[p]["sum"]` aliases them, so `optimizer.state_dict()` stays a
        faithful checkpoint while the fused step does the updates.  torch.optim.Adam / SGD / LazyRMSprop (OptimSpec.for_step): the engine's moment
        arrays and step counters take the optimizer's state — a parameter without state (never stepped) starts from zero — and the
        state of every parameter that has some aliases them.  last_layer: the same for engine_last_layer_step, over _final.{weight,
        bias} only: the frozen parameters' state is left as it is.  LazyRMSprop: every row of an existing square_avg is current (torch
        keeps it so), so a table's row stamps start at that table's step count; the optimizer gets the engine's flush as its hook
        (utils/optim.LazyRMSprop), and last_layer keeps the Adagrad accumulators: that step has no RMSprop.  AdamAdagradTables: the
        dense parameters as with Adam; a table shares `sum` with the engine's Adagrad accumulators (table_state) and its step counter
        with the state's `step`, and the engine holds no moment array of a table; with table_rowwise the `sum` is the engine's
        table_row_state, one float per row, and an existing `sum` of another shape is refused (ValueError).  RowwiseSparseAdam: as
        RowSparseAdam, but a table's exp_avg_sq is the engine's [rows] array; an exp_avg_sq of the other form (a RowSparseAdam's
        state under a row-wise plan, or the reverse) is refused (ValueError)."""
        eng = self._engine
        assert eng is not None, "run one forward first (lazy shapes)"
        from ..optim_spec import OptimSpec
        spec = OptimSpec.for_step(optimizer)
        if spec is None or not spec.moments or (last_layer and (spec.kind == "rmsprop" or spec.adagrad_tables)):
            spec = OptimSpec.of()  # (the Adagrad accumulators: also what an optimizer the fused step does not reproduce gets)
        if spec.moments and not last_layer and self._table_sharding == "row":
            from .._lib import EngineError
            raise EngineError("Adam / SGD in the fused step need whole tables on the device")
        slots, counters = self._state_slots(spec, last_layer)  # (raises for the other Adam form: nothing is bound then)
        self.__dict__["_bound"] = (spec, bool(last_layer))
        self._bound_optimizer_steps = getattr(self, "_last_layer_steps" if last_layer else "_engine_steps", 0)
        if counters is None:
            for p, views, _ in slots:
                st, tgt = optimizer.state[p], views["sum"]
                if "sum" in st and st["sum"].data_ptr() != tgt.data_ptr():
                    tgt.copy_(st["sum"].to(tgt.device).view_as(tgt))
                st["sum"] = tgt
                st.setdefault("step", torch.tensor(0.0))
            return
        counts = torch.zeros(counters.numel(), dtype=torch.float32)
        with torch.cuda.stream(eng.stream):
            for p, views, k in slots:
                st = optimizer.state.get(p)
                for key, tgt in views.items():
                    src = st.get(key) if st else None
                    if src is None:
                        tgt.zero_()
                    elif src.data_ptr() != tgt.data_ptr():
                        if key == "exp_avg_sq" and src.dim() != tgt.dim():
                            # (row-sparse Adam's [rows, 16] under the row-wise rule or the reverse: view_as would fail or, worse, fit)
                            raise ValueError("engine_bind_optimizer: the optimizer's exp_avg_sq of a table has shape %s, %s keeps %s"
                                             % (tuple(src.shape), "row-wise Adam (RowwiseSparseAdam)" if spec.rowwise_adam else
                                                "row-sparse Adam (RowSparseAdam)", tuple(tgt.shape)))
                        if key == "sum" and tuple(src.shape) != tuple(tgt.shape):
                            # (an element-wise checkpoint under the row-wise rule or the reverse: nothing may be reshaped or broadcast)
                            raise ValueError("engine_bind_optimizer: the optimizer's `sum` of a table has shape %s, the %s rule keeps %s"
                                             % (tuple(src.shape), "row-wise" if spec.table_rowwise else "element-wise",
                                                tuple(tgt.shape)))
                        tgt.copy_(src.to(tgt.device).view_as(tgt))
                if st:
                    if spec.kind in ("adam", "rmsprop"):
                        counts[k] = float(st.get("step", 0.0))
                    elif st.get("momentum_buffer") is not None:
                        counts[k] = 1.0  # (SGD keeps no count: "has a buffer" is what the engine needs)
            counters.copy_(counts.to(eng.device))
            if spec.kind == "rmsprop":
                eng._lazy_alpha = float(spec.alpha)
                for f, stamp in enumerate(eng.lazy_stamps):
                    stamp.fill_(int(counts[eng.param_index["_embedding.%d.weight" % f]]))
        eng.stream.synchronize()
        if spec.kind == "rmsprop":
            optimizer._lazy_flush = eng.flush_lazy_rows
        self._alias_state(optimizer, spec, slots, counts)

    def engine_bind_ema(self, ema):
        """Share a WeightEMA (utils/optim.py) with the engine: its shadows are copied into the engine's arrays (every row current as
        of `num_updates`: the stamps and the count start there), `ema.shadow[name]` then aliases them, and the WeightEMA gets the
        engine's hooks: `state_dict()` and `averaged()` flush first, `averaged()` exchanges in one launch, and a torch-route
        `update()` in the middle of a fused run flushes, averages densely and advances the engine's count and stamps."""
        eng = self._engine
        assert eng is not None, "run one forward first (lazy shapes)"
        from .._lib import EngineError
        if self._table_sharding == "row" or self._place_embedding_on_cpu:
            raise EngineError("the fused weight EMA needs whole tables on the device")
        eng.ensure_ema_state(ema.decay)
        eng.flush_ema_rows()  # (a second binding, e.g. the next epoch's: what the rows owe is paid before their stamps are set)
        names = [n for n, _ in self.named_parameters()]
        missing = [n for n in names if n not in eng.params]
        if missing:
            raise EngineError("engine_bind_ema: the engine holds no parameter %s" % missing[:3])
        with torch.no_grad(), torch.cuda.stream(eng.stream):
            for n in names:
                tgt, src = eng.ema_view(n), ema.shadow[n]
                if src.data_ptr() != tgt.data_ptr():
                    tgt.copy_(src.to(tgt.device).view_as(tgt))
                ema.shadow[n] = tgt
            for stamp in eng.ema_stamps:
                stamp.fill_(int(ema.num_updates))
            eng.ema_count.fill_(int(ema.num_updates))
        eng.stream.synchronize()

        def advance():
            with torch.cuda.stream(eng.stream):
                eng.ema_count.add_(1)
                for stamp in eng.ema_stamps:
                    stamp.add_(1)  # (every row was flushed and averaged densely: all stamps equal the count)
            eng.stream.synchronize()
        ema._hooks = dict(flush=eng.flush_ema_rows, swap=eng.swap_ema, advance=advance)  # (the model keeps no reference to `ema`)

    def engine_flush_decay(self):
        """Pay what fused steps with decoupled weight decay (engine_train_step(..., decoupled_wd=)) left owing: afterwards every row of
        `_embedding.<f>.weight` holds its current value.  One streaming launch over the tables when something is owed, else nothing."""
        eng = self.__dict__.get("_engine")
        if eng is not None and eng._decay_dirty:
            eng.flush_decay_rows()

    def engine_cowclip_stats(self):
        """(rows touched, rows clipped) by the fused steps with `cowclip=` since the engine was built (waits for the device)"""
        eng = self.__dict__.get("_engine")
        return eng.cowclip_stats() if eng is not None else (0, 0)

    def engine_bind_decay(self, decay):
        """Give a DecoupledWeightDecay (utils/optim.py) the engine's flush as its hook: a torch-route `apply()` in the middle of a fused
        run then multiplies tables whose rows are all current (the model keeps no reference to `decay`)"""
        decay._flush = self.engine_flush_decay

    def engine_sync_ema(self, ema):
        """read `num_updates` back from the engine's count (the fused steps since engine_bind_ema)"""
        eng = self._engine
        if eng is None or getattr(eng, "ema_count", None) is None:
            return
        torch.cuda.synchronize(eng.device)
        ema.num_updates = int(eng.ema_count.cpu()[0])

    _FINAL = ("_final.weight", "_final.bias")

    def _state_slots(self, spec, last_layer: bool):
        """what engine_bind_optimizer / engine_sync_optimizer_steps share: [(parameter, {state key: engine array}, counter index)] for the
        parameters the fused step updates (the whole model, or _final alone), and the engine's step counters (None: Adagrad)"""
        eng = self._engine
        params = dict(self.named_parameters())
        if not spec.moments:
            if last_layer:
                return [(params[n], {"sum": eng.state[n]}, None) for n in self._FINAL], None
            eng._ensure_table_state()
            slots = []
            for name, p in params.items():
                if name.startswith("_embedding."):
                    f = int(name.split(".")[1])
                    tgt = self._sharded.state[f] if self._table_sharding == "row" else eng.table_state[f]
                elif name in eng.state:
                    tgt = eng.state[name]
                else:
                    continue
                slots.append((p, {"sum": tgt}, None))
            return slots, None
        if last_layer:
            arrays = eng.ensure_last_layer_state(spec.kind)
            return [(params[n], {k: arrays[k][i] for k in spec.state_keys}, i) for i, n in enumerate(self._FINAL)], eng.ll_steps
        rule = spec.table_rule
        split = rule.state != "moments"  # (AdamAdagradTables: a table's state is Adagrad's sum — rule.state; its counter the state's step)
        eng.ensure_moments_state(spec.kind, tables=not split, rowwise_v=spec.rowwise_adam)
        if split:
            eng._ensure_split_table_state(spec)

        def views(n):
            if split and n.startswith("_embedding."):
                return {"sum": getattr(eng, rule.state)[int(n.split(".")[1])]}
            return {k: eng.moments_view(k, n) for k in spec.state_keys}
        return [(p, views(n), eng.param_index[n]) for n, p in params.items() if n in eng.param_index], eng.opt_steps

    @staticmethod
    def _alias_state(optimizer, spec, slots, counts):
        """Adam / SGD: the state of every parameter the engine has stepped (counts > 0) aliases the engine's arrays, as torch creates it on
        a parameter's first step"""
        for p, views, k in slots:
            # (a bf16 table has its state from the optimizer's constructor — no step() of its own ever creates it: it aliases the
            # engine's accumulators at once, so the constructor's zeros are not kept beside them)
            if counts[k] <= 0 and not (spec.bf16_tables and "sum" in views):
                continue
            st = optimizer.state[p]
            st.update(views)
            if spec.kind in ("adam", "rmsprop"):
                st["step"] = torch.tensor(float(counts[k]), dtype=torch.float32)

    def engine_sync_optimizer_steps(self, optimizer):
        """add the fused steps taken since engine_bind_optimizer to the optimizer's per-parameter step counters
        (Adam / SGD: the counters of the engine, and state entries for the parameters stepped for the first time)"""
        spec, last_layer = self.__dict__.get("_bound", (None, False))
        self.engine_flush_decay()
        if spec is not None and spec.moments:
            self._engine.flush_lazy_rows()  # (RMSprop: the state about to be aliased is read with every row current; else a no-op)
            self._engine.stream.synchronize()
            torch.cuda.synchronize(self._engine.device)
            slots, counters = self._state_slots(spec, last_layer)
            self._alias_state(optimizer, spec, slots, counters.detach().cpu())
            return
        steps = getattr(self, "_last_layer_steps" if last_layer else "_engine_steps", 0)
        done = steps - getattr(self, "_bound_optimizer_steps", 0)
        if done:
            params = dict(self.named_parameters())
            for p in ([params[n] for n in self._FINAL] if last_layer else self.parameters()):
                st = optimizer.state.get(p)
                if st is not None and "step" in st:
                    st["step"] = st["step"] + float(done)
            self._bound_optimizer_steps = steps


class SuperNetBlock(nn.Module):
    """One choice block (supernet.py:884-1381)."""

    def __init__(self, ops_config: Any, use_layernorm: bool, max_dims_or_dims_dense: int, max_dims_or_dims_sparse: int,
                 embedding_dim: int, activation: str = "relu", path_sampling_strategy: str = "single-path", fixed: bool = False,
                 fixed_micro_choice=None, anypath_choice: str = "uniform", supernet_training_steps: int = 0,
                 sparse_input_size: int = 26):
        super().__init__()
        self._ops_config = ops_config
        self._num_nodes = ops_config["num_nodes"]
        self._dense_nodes = ops_config["dense_nodes"]
        self._sparse_nodes = ops_config["sparse_nodes"]
        self._node_names = ops_config["node_names"]
        self._dense_node_dims = ops_config["dense_node_dims"]
        self._sparse_node_dims = ops_config["sparse_node_dims"]
        self._zero_nodes = ops_config["zero_nodes"]
        self._sparse_input_size = sparse_input_size
        self._use_layernorm = use_layernorm
        self._max_dims_or_dims_dense = max_dims_or_dims_dense
        self._max_dims_or_dims_sparse = max_dims_or_dims_sparse
        self._embedding_dim = embedding_dim
        self._activation = activation
        self._micro_path_sampling_strategy = path_sampling_strategy
        self._fixed = fixed
        self._fixed_micro_choice = fixed_micro_choice
        self._anypath_choice_fn = anypath_choice_fn[anypath_choice]
        self._supernet_training_steps = supernet_training_steps
        self._device_args = None
        self._supernet_train_steps_counter = -1
        self._nodes = nn.ModuleList()
        self.micro_last_choice = self._fixed_micro_choice if self._fixed else None
        if self._fixed:
            choice = self._get_choice()
            self._fixed_micro_choice = choice
            choice_nodes = choice["active_nodes"]
        else:
            choice, choice_nodes = None, list(range(self._num_nodes))
        for i in range(self._num_nodes):
            if i not in choice_nodes:
                self._nodes.append(nn.ModuleList([]))
                continue
            name = self._node_names[i]
            if name in _dense_binary_nodes + _dense_unary_nodes + _dense_sparse_nodes:
                dims = choice["dense_in_dims"] if self._fixed else self._max_dims_or_dims_dense
            elif name in _sparse_nodes:
                dims = choice["sparse_in_dims"] if self._fixed else self._max_dims_or_dims_sparse
            else:
                raise NotImplementedError("Block name {} is not supported in supernet!".format(name))
            self._nodes.append(_make_node(name, use_layernorm, int(dims), activation, embedding_dim, fixed))
        if self._fixed and choice["dense_sparse_interact"] == 0:
            self.project_emb_dim, self.project_emb_dim_layernorm = None, None
        else:
            self.ds_interact_expanded_dim = DS_INTERACT_NUM_SPLITS * self._embedding_dim
            self.project_emb_dim = nn.LazyLinear(self.ds_interact_expanded_dim, bias=not use_layernorm)
            self.project_emb_dim_layernorm = nn.LayerNorm(self.ds_interact_expanded_dim, eps=1e-5) if use_layernorm else None
        if self._fixed and choice["deep_fm"] == 0:
            self.deep_fm, self.deep_fm_output_ln = None, None
        else:
            self.deep_fm_dims = max(self._dense_node_dims) if not self._fixed else choice["dense_in_dims"]
            self.deep_fm = FactorizationMachine3D(fixed=self._fixed, use_layernorm=self._use_layernorm, max_dims_or_dims=int(self.deep_fm_dims))
        self.choice = []

    def forward(self, tensors, choices=None):
        """supernet.py:1067-1162 / fixed_forward :1185-1242: tensors = [dense [B,D], sparse [B,N,16], dense_left, dense_right] ->
        (dense_out, sparse_out).  Inside a SuperNet the block is part of the network's launch plan; called on its own it compiles
        a single-block plan from the same emitter (plan.block_walk) and runs it on the HIP engine."""
        from .. import opexec
        choice = self._resolve_choice(choices)
        dense_t, sparse_t, left_t, right_t = tensors
        self.materialize([t.shape for t in tensors], choice, dense_t.device)
        key = json.dumps(choice, sort_keys=True, default=lambda o: o.tolist() if hasattr(o, "tolist") else o.item())
        dense_out, sparse_out = opexec.run(self, self._emitter(choice), [dense_t, sparse_t, left_t, right_t], key_extra=(key,))
        return dense_out, sparse_out

    def fixed_forward(self, tensors, choices):
        return self.forward(tensors, choices)

    def _emitter(self, ch):
        from .. import opexec
        cfg = opexec.OpConfig(self._use_layernorm, self._activation, self._fixed)
        ops = self._ops_config

        def emit(ctx, ins):
            d, s, l, r = ins
            dv, sv = P.block_walk(ctx, cfg, "op", ops, ch, [P.Seg(d, 0, d.width)], d.width, [P.Seg(s, 0, s.N)], s.N,
                                  [P.Seg(l, 0, l.width)], l.width, [P.Seg(r, 0, r.width)], r.width)
            return [dv, sv]
        return emit

    def materialize(self, in_shapes, choice=None, device=None):
        """What the reference's first forward does to the module tree (host logic only).  Lazy shapes come from the first
        inputs; a weight-sharing block materialises every node (the reference warms it up on the full path,
        train_utils.py:413-433), a fixed block only what its choice reaches."""
        from .. import opexec
        if opexec.has_lazies(self):
            warm = (choice if choice is not None else self._fixed_micro_choice) if self._fixed else \
                {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in self._get_full_path_choice().items()}
            opexec.materialize_lazies(self, opexec.infer_shapes(self._emitter(warm), in_shapes), device=device)

    def _get_choice(self):
        """supernet.py:1009-1061"""
        c, n = self._supernet_train_steps_counter, self._supernet_training_steps
        thresh = 1.0 - c / (n + 1e-10) if (c < n and c > 0) else 0
        s = self._micro_path_sampling_strategy
        if s == "single-path":
            choice = self._get_full_path_choice() if np.random.random() < thresh else self._get_single_path_choice()
        elif s == "full-path":
            choice = self._get_full_path_choice()
        elif s == "any-path":
            choice = self._get_full_path_choice() if np.random.random() < thresh else self._get_any_path_choice()
        elif s == "fixed-path" and self.micro_last_choice is None:
            if getattr(self, "_fixed_path_called", False):
                raise ValueError("Error! fixed-path choice should be generated only once for each supernet!")
            self._fixed_path_called = True
            choice = self._get_fixed_path_choice()
        elif s in ("fixed-path", "evo-2shot-path"):
            choice = self.micro_last_choice
        else:
            raise NotImplementedError("Path strategy {} is not supported!".format(s))
        if s != "full-path":
            self.micro_last_choice = choice
        return choice

    def _resolve_choice(self, choices):
        """supernet.py:1067-1076: draw (or take) the micro choice, then advance the block's own step counter"""
        choice = self._get_choice() if choices is None else choices
        self.choice = choice
        if not self._fixed:
            self._supernet_train_steps_counter += 1
        return choice

    def get_all_subnet_micro_choices(self):
        """supernet.py:1164-1183"""
        out = {"active_nodes": [], "dense_in_dims": [], "sparse_in_dims": [], "dense_sparse_interact": [0, 1]}
        for s in self._sparse_nodes:
            for d in self._dense_nodes:
                out["active_nodes"].append((d, s))
        out["dense_in_dims"] = [(x,) for x in self._dense_node_dims]
        out["sparse_in_dims"] = [(x,) for x in self._sparse_node_dims]
        return out

    def _get_single_path_choice(self):
        """supernet.py:1244-1263"""
        while True:
            choice = {"active_nodes": sorted([np.random.choice(self._dense_nodes)] + [np.random.choice(self._sparse_nodes)]),
                      "dense_in_dims": np.random.choice(self._dense_node_dims),
                      "sparse_in_dims": np.random.choice(self._sparse_node_dims),
                      "dense_sparse_interact": np.random.choice([0, 1]), "deep_fm": np.random.choice([0, 1])}
            if choice["active_nodes"] != self._zero_nodes:
                return choice

    def _get_full_path_choice(self):
        """supernet.py:1265-1276"""
        return {"active_nodes": np.arange(self._num_nodes), "dense_in_dims": np.max(self._dense_node_dims),
                "sparse_in_dims": np.max(self._sparse_node_dims), "dense_sparse_interact": 1, "deep_fm": 1}

    def _get_any_path_choice(self):
        """supernet.py:1278-1303"""
        while True:
            nd = self._anypath_choice_fn(len(self._dense_nodes))
            ns = self._anypath_choice_fn(len(self._sparse_nodes))
            dn = np.random.choice(self._dense_nodes, nd, replace=False).tolist()
            sn = np.random.choice(self._sparse_nodes, ns, replace=False).tolist()
            choice = {"active_nodes": sorted(dn + sn), "dense_in_dims": np.random.choice(self._dense_node_dims),
                      "sparse_in_dims": np.random.choice(self._sparse_node_dims),
                      "dense_sparse_interact": np.random.choice([0, 1]), "deep_fm": np.random.choice([0, 1])}
            if choice["active_nodes"] != self._zero_nodes:
                return choice

    def _get_fixed_path_choice(self):
        """supernet.py:1305-1313"""
        return self._get_single_path_choice()

    def configure_choice(self, choice):
        """supernet.py:1316-1318"""
        self.choice = copy.deepcopy(choice)
        self.micro_last_choice = copy.deepcopy(choice)
