"""SupernetEngine — executes compiled plans (nasrec_amd/plan.py) on one MI355X through the C-ABI.

Ownership: PyTorch owns every byte of device memory (parameters, gradients, optimizer state, activations);
the engine owns launch plans, a HIP stream and captured hipGraphs.  Dense parameters live in ONE flat fp32 buffer
(gradients and Adagrad state in two more of the same layout) so that the global-norm clip, the optimizer and the
data-parallel all-reduce are single passes; the embedding tables stay separate [rows,16] tensors and are updated
row-sparsely (identical to the dense reference update when weight_decay == 0).

There is no CPU path here: everything below needs the HIP library and a GPU.
"""
import copy
import ctypes as C
import json
import math
import os
from typing import Dict, List, Optional

import torch

from . import _lib as L
from . import plan as P
from . import schedule as S
from .optim_spec import OptimSpec

E = 16
# largest (global) batch whose row-gradient dedup runs in two halves (csrc/dedup_bodies.h; <= L.DEDUP_IDS_MAX_B); 0 = the one-launch kernels
DEDUP_SPLIT_MAX_B = min(int(os.environ.get("NASREC_DEDUP_SPLIT_MAX_B", "2048")), L.DEDUP_IDS_MAX_B)
# the id half of a level-scheduled step (B <= 256) as an ITEM of the joint forward + backward program (A/B knob: 0 = on the staging launch)
_IDS_AS_ITEM = os.environ.get("NASREC_IDS_AS_ITEM", "1") != "0"
# NASREC_WL_TUNE=1: time a handful of level schedules of a fixed batch-256 training plan at compile time (_tune_levels).  Off by default: on the
# round-6 bodies the model's own schedule is within 0.4 % of the best candidate (0.2172 against 0.2163 ms per joint program), and the replays
# write the engine-wide gradient arena — a compile() in the middle of a step sequence must not do that.
_WL_TUNE = os.environ.get("NASREC_WL_TUNE", "0") == "1"
_WL_TUNE_MARGIN = float(os.environ.get("NASREC_WL_TUNE_MARGIN", "0.004"))
# the worklist descriptors of a fixed batch-256 plan live in device memory, uploaded once (ABI 17, nasrec_worklist_prepare): a launch that passes
# its 4 KB descriptor by value reads it from a fresh, cold copy in the kernel-argument ring (tools/micro/kernarg_probe.hip: + 0.75 - 1.6 us)
_WL_RESIDENT = os.environ.get("NASREC_WL_RESIDENT", "1") != "0"
_FUSE_FINAL = os.environ.get("NASREC_FUSE_FINAL", "1") != "0"  # joint program: final logit + the per-sample part of its backward as one operator
# clip + Adagrad of a fixed sub-network over the ranges of the parameters its backward reaches, not the whole arena (A/B knob)
_FIXED_OPT_TABLE = os.environ.get("NASREC_FIXED_OPT_TABLE", "1") != "0"


def _ptr_array(descs):
    arr = (C.c_void_p * len(descs))()
    for i, d in enumerate(descs):
        arr[i] = C.addressof(getattr(d, "launch_as", d))  # (a worklist whose descriptor lives in device memory: _resident_worklists)
    return arr


class Program:
    """An ordered list of descriptors; runs with one host call (nasrec_program_run) or as a captured hipGraph."""

    def __init__(self, descs: List):
        self.descs = list(descs)
        self.arr = _ptr_array(self.descs)
        self.n = len(self.descs)
        self.graph = None

    def run(self, stream_ptr):
        lib = L.load()
        L.check(lib.nasrec_program_run(stream_ptr, self.arr, self.n))

    def capture(self, stream_ptr):
        lib = L.load()
        g = C.c_void_p()
        L.check(lib.nasrec_graph_create(stream_ptr, self.arr, self.n, C.byref(g)))
        self.graph = g

    def replay(self, stream_ptr):
        L.check(L.load().nasrec_graph_launch(self.graph, stream_ptr))

    def __del__(self):
        try:
            if self.graph is not None:
                L.load().nasrec_graph_destroy(self.graph)
        except Exception:
            pass


class CompiledPlan:
    # (the dense chunk table of the plan's optimizer tail, for reports: bench.py)
    chunk_tab = property(lambda self: self.tail.chunk_tab)
    nchunks = property(lambda self: self.tail.nchunks)


class TailBuffers:
    """work buffers of the optimizer tail (_optimizer_descs), allocated on first use: a plan's own, or one set that every program of a
    data-parallel run shares (parallel.EngineDP).  Never replaced once set: the programs built earlier hold their raw addresses."""
    leader = gsum = emb_partial = dense_partial = dd_order = dd_lists = dd_counts = dd_heads = emb_partial2 = None


class OptimizerTail:
    """What the clip + optimizer launches of a plan read besides the engine's own arrays: the optimizer (an OptimSpec), the chunk table of
    the dense ranges the norm and the update walk (None: the whole arena), the plan's weight-decay / moments chunk tables and the work
    buffers.  compile builds one per plan; a data-parallel optimizer runs over a plan's (`over`).  _optimizer_descs leaves `dedup_ids`
    (the id-only half of the row dedup) or None."""
    wd_add = wd_set = wd_union = wd_tab = mom_chunks = mom_inc = mom_tab = None  # (_weight_decay_tables, _moments_tables)
    wd_tables = mom_tables = mom_names = ()

    def __init__(self, spec, arena=None, chunks=(None, 0), bufs=None):
        self.spec, self.arena = spec, arena
        self.chunk_tab, self.nchunks = chunks
        self.bufs = bufs if bufs is not None else TailBuffers()
        self.dedup_ids = None
        self.cowclip = None  # (r, zeta) of a plan with CowClip in front of its optimizer (compile), else None

    def over(self, chunks, bufs):
        """this plan's optimizer and chunk tables over another dense chunk table and a data-parallel run's work buffers"""
        t = copy.copy(self)
        t.arena, t.bufs, t.dedup_ids = None, bufs, None
        t.chunk_tab, t.nchunks = chunks
        return t


_ITEMSIZE = {torch.float32: 4, torch.int64: 8, torch.int32: 4, torch.uint8: 1, torch.float64: 8}


class ArenaRef:
    """A buffer of a plan slot's arena: address and size now, the torch view only if somebody asks for one.  A sampled supernet path
    compiles ~2000 buffers per step and the plan only ever needs their ADDRESSES (descriptors carry raw pointers); creating a
    tensor view for each cost 2.5 ms of host time per step (40 % of the plan compile).  Anything else (`.view`, `.copy_`, `.double`,
    ...) goes to the lazily created tensor."""
    __slots__ = ("_chunk", "_off", "_n", "_dtype", "_ptr", "_t")

    def __init__(self, chunk, off, n, dtype, ptr):
        self._chunk, self._off, self._n, self._dtype, self._ptr, self._t = chunk, off, n, dtype, ptr, None

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n

    def tensor(self):
        if self._t is None:
            self._t = self._chunk[self._off:self._off + self._n * _ITEMSIZE[self._dtype]].view(self._dtype)
        return self._t

    def __getattr__(self, name):
        return getattr(self.tensor(), name)


class _RawDeviceBytes:
    """n bytes of device memory at ptr, as the CUDA array interface torch.as_tensor understands (zero-copy; the tensor's storage keeps this
    object alive, and the memory is freed with it)."""

    def __init__(self, ptr, n):
        self.ptr, self.n = int(ptr), int(n)
        self.pid = os.getpid()  # (a forked child — multiprocessing.Manager() of a test, a DataLoader worker — inherits this object but not a usable HIP
        #                         runtime: its garbage collector must not free the parent's memory.  Found as a segfault of a Manager server.)
        self.__cuda_array_interface__ = {"shape": (self.n,), "typestr": "|u1", "data": (self.ptr, False), "version": 2, "strides": None}

    def __del__(self):  # (when the last tensor view of the memory is gone: torch keeps this object alive through the storage)
        try:
            import sys
            if self.ptr and not sys.is_finalizing() and os.getpid() == self.pid:  # (at interpreter exit the HIP runtime may already be gone: the driver reclaims the memory)
                L.load().nasrec_free_uncached(C.c_void_p(self.ptr))
            self.ptr = 0
        except Exception:
            pass


class Arena:
    """Device memory of one plan slot: buffers are bump-allocated out of a few large chunks that live as long as the engine, so
    compiling a plan costs no allocator calls (a sampled supernet path almost never repeats: every step compiles a plan with
    ~10^3 buffers of new sizes, which sent the caching allocator to hipMalloc / hipFree and their device synchronisations).
    Slots are recycled in stream order: a plan's kernels are enqueued behind those of the plan that used the slot before."""

    CHUNK = 256 << 20  # bytes

    def __init__(self, device, uncached: bool = False):
        """uncached: the chunks are UNCACHED device memory (nasrec_alloc_uncached; wrapped as torch tensors through the CUDA array
        interface, freed with the arena): the arena of a persistent step, whose items hand buffers to each other inside one launch"""
        self.device = device
        self.uncached = bool(uncached)
        self.chunks: List[torch.Tensor] = []
        self.base: List[int] = []
        self.cur, self.off = 0, 0

    def reset(self):
        self.cur, self.off = 0, 0

    def _grow(self, nbytes):
        n = max(self.CHUNK, nbytes) if not self.uncached else max(64 << 20, (nbytes + (1 << 20) - 1) & ~((1 << 20) - 1))
        if self.uncached:
            with torch.cuda.device(self.device):
                ptr = C.c_void_p()
                L.check(L.load().nasrec_alloc_uncached(n, C.byref(ptr)))
            c = torch.as_tensor(_RawDeviceBytes(ptr.value, n), device=self.device)
            assert c.data_ptr() == ptr.value and c.numel() == n and c.dtype == torch.uint8
        else:
            c = torch.empty(n, dtype=torch.uint8, device=self.device)
        self.chunks.append(c)
        self.base.append(c.data_ptr())

    def ranges(self):
        """[(first byte, one past the last)] of the arena's chunks"""
        return [(b, b + c.numel()) for b, c in zip(self.base, self.chunks)]


    def alloc(self, numel: int, dtype=torch.float32) -> ArenaRef:
        numel = int(numel)
        nbytes = (numel * _ITEMSIZE[dtype] + 255) & ~255
        while True:
            if self.cur < len(self.chunks):
                c = self.chunks[self.cur]
                if self.off + nbytes <= c.numel():
                    r = ArenaRef(c, self.off, numel, dtype, self.base[self.cur] + self.off)
                    self.off += nbytes
                    return r
                self.cur += 1
                self.off = 0
                continue
            self._grow(nbytes)

    def used_bytes(self) -> int:
        return sum(c.numel() for c in self.chunks[:self.cur]) + self.off

    def reserve(self, nbytes: int):
        """grow to at least nbytes now (one allocator call per chunk, outside any timed or latency-sensitive region)"""
        while sum(c.numel() for c in self.chunks) < nbytes:
            self._grow(self.CHUNK)


# The buffers of a level-scheduled training plan (fixed sub-network, batch <= 256) live in UNCACHED device memory: a step of ~27 dependent
# launches hands every activation from one kernel to the next exactly once, and a store that goes through to memory leaves nothing for the
# kernel boundary to write back — 0.2485 -> 0.2447 / 0.2458 ms per cfg-2 step in four A/B pairs (profiles/r06_ab_uc_arena.txt), bit-identical
# results.  It is also what lets the persistent step (NASREC_OP_PERSIST) hand buffers over INSIDE a launch.  NASREC_UC_ARENA=0: torch's allocator.
_UC_ARENA = os.environ.get("NASREC_UC_ARENA", "1") == "1"
_UC_FLAT = os.environ.get("NASREC_UC_FLAT", "g")


def _on_device(fn):
    """run an engine entry point with the engine's device current: raw kernel launches, memsets, graph capture and event
    creation all act on the CURRENT device, whatever device the caller left selected (main_train.py --gpu N, N != 0)"""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        if torch.cuda.current_device() == self.device.index:
            return fn(self, *a, **kw)
        with torch.cuda.device(self.device):
            return fn(self, *a, **kw)
    return wrapped


class SupernetEngine:
    def __init__(self, cfg: P.NetConfig, Fd: int, Fs: int, num_embeddings: List[int], device="cuda:0", warm_choice=None,
                 world_size: int = 1, tables: Optional[List[torch.Tensor]] = None, host_embedding: bool = False,
                 matmul_precision: Optional[str] = None):
        """matmul_precision: "highest" | "high" | "medium" (None: the environment variable NASREC_MATMUL_PRECISION, else "highest") —
        what torch.set_float32_matmul_precision is to torch: tensors, accumulation and results stay fp32, the value PERMITS the
        throughput-regime GEMM launches of every plan to feed the matrix cores bf16 operands ("medium") or bf16 x 3 ("high"); every
        other launch stays fp32 (include/nasrec_hip.h NASREC_PRECISION_*).  "highest" is bit for bit the arithmetic without it.
        host_embedding: the tables live in host memory (SuperNet(place_embedding_on_cpu=True), supernet.py:231,418-428): the engine
        holds no table, the caller hands the looked-up rows [B, Fs, 16] to every forward and receives their gradient; only the
        forward / backward programs are available in this mode (the fused optimizer step needs the tables on the device)."""
        L.load()
        self.matmul_precision = L.matmul_precision_name(matmul_precision)
        if not torch.cuda.is_available():
            raise L.EngineError("SupernetEngine needs a GPU: there is no CPU fallback")
        self.cfg, self.Fd, self.Fs = cfg, Fd, Fs
        self.num_embeddings = [int(n) for n in num_embeddings[:Fs]]
        # hard limits of the kernels, raised here instead of corrupting later: the row-gradient dedup packs ids into 32 bits
        # (csrc/embedding.hip; ids are range-checked against the table by the gather, so rows < 2^31 makes the cast exact), a
        # descriptor carries at most MAX_TABLES table pointers
        for f, n in enumerate(self.num_embeddings):
            if not 0 < n < (1 << 31):
                raise ValueError("embedding table %d has %d rows: the engine supports 1 .. 2^31 - 1 rows per table" % (f, n))
        if Fs > L.MAX_TABLES:
            raise ValueError("%d sparse fields: the engine supports at most %d" % (Fs, L.MAX_TABLES))
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.world_size = world_size
        self.stream = torch.cuda.Stream(device=self.device)
        # the persistent step (NASREC_OP_PERSIST: the joint program's items in one launch, dependencies resolved in the kernel): built, bit-identical
        # to the level launches, and SLOWER on the cfg-2 step (0.274 against 0.245 ms: workgroups are dispatched in index order, and the ones
        # waiting for a dependency hold the chip's 768 slots against items that could run — DESIGN.md, profiles/r06_persist_*): opt-in
        self.persist = S.PERSIST and os.environ.get("NASREC_PERSIST_DEFAULT", "0") == "1"
        self._persist_errs = []
        self._last_plan = None
        # batch <= 256 (fixed sub-networks): operators that do not depend on each other share heterogeneous launches
        # (nasrec_amd/schedule.py); NASREC_WORKLIST=0 keeps one launch per operator (A/B runs, bit-identical results)
        self.level_schedule = os.environ.get("NASREC_WORKLIST", "1") != "0"
        # opt-in: drop forward operators nobody reads (schedule.eliminate_dead_forward); off = every reference operator runs
        self.dead_code_elimination = os.environ.get("NASREC_DCE", "0") == "1"
        if cfg.fixed:
            assert warm_choice is not None, "fixed mode needs the fixed choice"
            self.warm_choice = warm_choice
        else:
            self.warm_choice = P.full_path_choice(cfg)
        self.shapes = P.infer_param_shapes(cfg, self.warm_choice, Fd, Fs, self.num_embeddings)
        self.dense_names = [n for n in self.shapes if not n.startswith("_embedding.")]
        # flat dense arena, every parameter 16-byte aligned
        self.offsets, off = {}, 0
        for n in self.dense_names:
            self.offsets[n] = off
            numel = 1
            for s in self.shapes[n]:
                numel *= s
            off += (numel + 3) // 4 * 4
        self.flat_numel = off
        with torch.cuda.stream(self.stream):
            # A fixed sub-network's gradient arena lives in uncached memory like its plan's buffers (_UC_ARENA): every gradient is written once
            # by the backward and read once by the optimizer's launches — 0.2447 -> 0.2426 ms per cfg-2 step, three A/B pairs
            # (profiles/r06_ab_uc_arena.txt).  NASREC_UC_FLAT = letters of the flat arenas to place there: g(radients), s(tate), p(arameters).
            uc = _UC_FLAT if (cfg.fixed and off * 4 <= (64 << 20) and _UC_ARENA) else ""
            self._uc_flat_arena = Arena(self.device, uncached=True) if uc else None

            def flat(tag):
                if tag in uc:
                    t = self._uc_flat_arena.alloc(off).tensor()
                    t.zero_()
                    return t
                return torch.zeros(off, dtype=torch.float32, device=self.device)
            self.flat_p, self.flat_g, self.flat_s = flat("p"), flat("g"), flat("s")
            self.host_embedding = bool(host_embedding)
            if self.host_embedding:
                self.tables = []
            elif tables is not None:  # adopt the caller's nn.Embedding storage (no copy; PyTorch keeps ownership)
                # (fp32, or all of them bf16 — SuperNet(table_dtype=torch.bfloat16): [rows, 16] with 32-byte rows, read by the gather and
                # written by the row-wise Adagrad of the fused step alone; every other consumer refuses them, _refuse_bf16_tables)
                for t, n in zip(tables, self.num_embeddings):
                    assert t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous() and tuple(t.shape) == (n, E)
                    assert t.dtype == tables[0].dtype, "the tables are fp32 or bf16, not a mixture"
                self.tables = list(tables)
            else:
                self.tables = [torch.zeros(n, E, dtype=torch.float32, device=self.device) for n in self.num_embeddings]
            self.table_state: Optional[List[torch.Tensor]] = None
            self.table_row_state: Optional[List[torch.Tensor]] = None  # (row-wise Adagrad on the tables: one float per row)
            self.lr_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
            self.clip_out = torch.ones(2, dtype=torch.float32, device=self.device)  # [coef, total_norm]
            self.oob = torch.zeros(2, dtype=torch.int32, device=self.device)  # [index out of range, dedup hash partition overflow]
        self.tables_bf16 = bool(self.tables) and self.tables[0].dtype == torch.bfloat16
        self.params: Dict[str, torch.Tensor] = {}
        self.grads: Dict[str, torch.Tensor] = {}
        self.state: Dict[str, torch.Tensor] = {}
        for n in self.dense_names:
            shp = self.shapes[n]
            numel = 1
            for s in shp:
                numel *= s
            o = self.offsets[n]
            self.params[n] = self.flat_p[o:o + numel].view(shp)
            self.grads[n] = self.flat_g[o:o + numel].view(shp)
            self.state[n] = self.flat_s[o:o + numel].view(shp)
        for f in range(len(self.tables)):
            self.params["_embedding.%d.weight" % f] = self.tables[f]
        self._plans: Dict[str, CompiledPlan] = {}
        self._pcache: Dict[str, tuple] = {}
        self._spare_arenas: List[Arena] = []
        self.stream.synchronize()

    # -------------------------------------------------------------------------------------------------------
    @_on_device
    def load_params(self, src: Dict[str, torch.Tensor]):
        """copy values (any device/dtype) into the engine's storage; keys = reference state_dict names"""
        with torch.cuda.stream(self.stream):
            for k, v in src.items():
                if k not in self.params:
                    raise KeyError("unexpected parameter %s" % k)
                self.params[k].copy_(torch.as_tensor(v).to(torch.float32).reshape(self.params[k].shape))
        missing = [k for k in self.params if k not in src]
        self.stream.synchronize()
        return missing

    @_on_device
    def init_weights(self, seed: int = 0):
        """train_utils.py:70-89 applied to this parameter set: xavier_normal_ tables, xavier_uniform_ 2-D weights
        (nn.Linear and the MultiheadAttention projections alike), zero biases; LayerNorm stays at its constructor
        value (1, or LN_INIT = 0.17 for the two Transformer norms, modules.py:598,636-640) with zero bias."""
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        with torch.cuda.stream(self.stream):
            for name, p in self.params.items():
                is_ln = ("_ln" in name) or ("layernorm" in name)
                if name.startswith("_embedding."):
                    std = (2.0 / (p.shape[0] + p.shape[1])) ** 0.5
                    if p.dtype == torch.bfloat16:  # (drawn in fp32 as ever, then rounded to nearest even: one table of overhead)
                        p.copy_(torch.empty(p.shape, dtype=torch.float32, device=p.device).normal_(0.0, std, generator=g))
                    else:
                        p.normal_(0.0, std, generator=g)
                elif is_ln:
                    if name.endswith(".weight"):
                        p.fill_(0.17 if ("_attn_ln" in name or "_attn_fc_ln" in name) else 1.0)
                    else:
                        p.zero_()
                elif p.dim() == 2:
                    bound = (6.0 / (p.shape[0] + p.shape[1])) ** 0.5
                    p.uniform_(-bound, bound, generator=g)
                else:
                    p.zero_()
            self.flat_s.zero_()
            if self.table_state is not None:
                for t in self.table_state:
                    t.zero_()
            if self.table_row_state is not None:
                for t in self.table_row_state:
                    t.zero_()
        self.stream.synchronize()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        if self._decay_dirty:
            self.flush_decay_rows()
        self.stream.synchronize()
        return {k: v.detach().cpu().clone() for k, v in self.params.items()}

    def _refuse_bf16_tables(self, what: str):
        """bf16 tables are read by the gather and written by the fused row-wise Adagrad (OptimSpec.table_kind "rowwise_adagrad_bf16")
        alone: every other kernel that takes a table indexes fp32 rows of 64 bytes, and is refused before anything is launched"""
        if getattr(self, "tables_bf16", False):
            raise L.EngineError("bf16 tables: %s reads and writes fp32 table rows; bf16 tables train with AdamAdagradTables("
                                "table_rowwise=True) on the fused step (engine_train_step) and nothing else" % what)

    def _ensure_table_state(self):
        self._refuse_bf16_tables("Adagrad's [rows, 16] table state (the Adagrad apply launch, adagrad_rows, weight decay's phase 1)")
        if self.table_state is None:
            with torch.cuda.stream(self.stream):
                self.table_state = [torch.zeros_like(t) for t in self.tables]

    def _ensure_table_row_state(self):
        """row-wise Adagrad's accumulators (OptimSpec.table_kind "rowwise_adagrad"): per table one fp32 per row, zero, on first use.
        Never `table_state`: the Adagrad apply launch and weight decay's phase 1 index that as [rows, 16]."""
        if getattr(self, "table_row_state", None) is None:
            with torch.cuda.stream(self.stream):
                self.table_row_state = [torch.zeros(t.shape[0], dtype=torch.float32, device=self.device) for t in self.tables]

    def _ensure_split_table_state(self, spec):
        """the tables' state of a split-optimizer spec: `table_row_state` for the row-wise rule, `table_state` for the element-wise one"""
        getattr(self, "_ensure_" + spec.table_rule.state)()  # (_ensure_table_state / _ensure_table_row_state: fp32 whatever the tables' storage type)

    # -------------------------------------------------------------------------------------------------------
    @_on_device
    def compile(self, choice, B: int, train: bool, clip: Optional[float] = 5.0, eps: float = 1e-2, graph: bool = False,
                grad_scale: Optional[float] = None, defer_dw: bool = True, row_grad_out: Optional[torch.Tensor] = None,
                local_optimizer: bool = True, spec: Optional[OptimSpec] = None, cowclip=None) -> CompiledPlan:
        """row_grad_out: storage [B * Fs * 16] the backward writes the per-sample embedding-row gradients into (a data-parallel step
        hands in the head of its all-gather send buffer: no copy between the backward and the exchange); local_optimizer = False: the
        plan gets no clip + Adagrad program of its own (a data-parallel step runs its optimizer over the GLOBAL batch).
        spec: the optimizer (nasrec_amd/optim_spec.py, OptimSpec.of); None = Adagrad with `eps`.  Weight decay adds get_l2_loss's
        gradient (_weight_decay_descs), Adam / SGD replace Adagrad (_moments_descs).  With local_optimizer = False the spec only shapes
        the plan's chunk tables (_weight_decay_tables, _moments_tables), which the data-parallel optimizer program reads
        (parallel.EngineDP.dp_optimizer)
        cowclip: (r, zeta) = CowClip on the summed table rows in front of the optimizer (_cowclip_descs), part of the plan's key: a
        step with other values, or with none, is another plan"""
        rgo = row_grad_out.data_ptr() if row_grad_out is not None else None
        spec = spec if spec is not None else OptimSpec.of(eps)
        if cowclip is not None:
            cowclip = (float(cowclip[0]), float(cowclip[1]))
            self._refuse_cowclip(spec, train, local_optimizer, B)
        if spec.wd and not train:
            raise L.EngineError("weight decay is part of the fused training step's optimizer: it needs train=True")
        if spec.moments and not train:
            raise L.EngineError("Adam / SGD are the fused training step's optimizer: they need train=True")
        if spec.dwd and not (train and local_optimizer):
            raise L.EngineError("decoupled weight decay is part of the one-process fused training step's optimizer")
        if spec.bf16_tables != (self.tables_bf16 and train):
            if not self.tables_bf16:
                raise L.EngineError("table_kind %r is the rule of bf16 tables: this engine's tables are fp32" % (spec.table_kind,))
            self._refuse_bf16_tables("a training plan with %s" % ("Adagrad" if not spec.moments else
                                                                 "dense or row-sparse %s%s" % (spec.kind, " + " + spec.table_kind if spec.table_kind else "")))
        if self.tables_bf16 and train:
            if spec.wd:
                self._refuse_bf16_tables("weight decay (its two phases, and the moments launch's phase 1 behind them)")
            if spec.ema:
                self._refuse_bf16_tables("the fused weight EMA")
            if spec.dwd:
                self._refuse_bf16_tables("the fused decoupled weight decay")
            if not local_optimizer:
                self._refuse_bf16_tables("the data-parallel step")
            if self.persist and self.level_schedule and self.cfg.fixed and B <= 256:
                self._refuse_bf16_tables("the persistent step (NASREC_PERSIST_DEFAULT=1)")
        fast = (id(choice), B, train, clip, eps, graph, grad_scale, defer_dw, rgo, local_optimizer, spec, cowclip)
        hit = self._last_plan
        if self.cfg.fixed and hit is not None and hit[0] == fast and hit[1] is choice:  # fixed sub-network, same choice object: skip the JSON key
            return hit[2]
        key = json.dumps([choice, B, train, clip, eps, graph, grad_scale, defer_dw, rgo, local_optimizer, spec] +
                         ([list(cowclip)] if cowclip is not None else []), sort_keys=True, default=_jsonable)
        if key in self._plans:
            self._last_plan = (fast, choice, self._plans[key])
            return self._plans[key]
        arena = None
        # (weight decay: the default launches — the persistent step is an opt-in that has not been built for it)
        persist = bool(self.persist and self.level_schedule and self.cfg.fixed and B <= 256 and train and local_optimizer and not spec.wd
                       and not spec.moments and not spec.dwd)
        if self.cfg.fixed and B <= 256 and train and self.level_schedule and (_UC_ARENA or persist):
            arena = Arena(self.device, uncached=True)  # (see _UC_ARENA; the persistent step needs it whatever the knob says)
        if not self.cfg.fixed:
            # Sampled paths rarely repeat: a small cache of plan slots, each with its own arena.  Evicting a plan needs no device
            # synchronisation: its slot is reused by a plan whose kernels are enqueued, in stream order, behind the evicted one's
            # (a caller that kept an autograd graph on the evicted plan is told so in backward: cp.evicted).
            if len(self._plans) >= 4:
                old = self._plans.pop(next(iter(self._plans)))
                old.evicted = True
                arena = old.arena
                old.arena = None
                self._last_plan = None
                # a plan is a web of closures over its context: cut it open so reference counting frees the ~10^4 objects now
                # instead of leaving them to the cyclic collector (whose full passes stalled a step for 17-56 ms)
                octx = getattr(old, "ctx", None)
                if octx is not None:
                    octx.closures = []
                    octx.deferred = []
                    octx.mha_reduce = []
                    octx.keep = []
                    octx.sk_workspace = None
            if arena is None:
                arena = self._spare_arenas.pop() if self._spare_arenas else Arena(self.device)
            arena.reset()
        cfg = self.cfg
        with torch.cuda.stream(self.stream):
            cp = CompiledPlan()
            cp.arena, cp.evicted = arena, False
            cp.tail = OptimizerTail(spec, arena)
            cp.tail.cowclip = cowclip
            ctx = P.Ctx(B, self.device, self.params, self.grads, shape_only=False, train=train)
            ctx.sk_workspace = self._sk_workspace
            ctx.matmul_precision = L.PRECISION_BY_NAME[self.matmul_precision]
            # parked weight-gradient batches are for one-launch-per-operator plans; the level scheduler places the products itself
            ctx.defer_dw = defer_dw and getattr(self, "park_weight_grads", True) and not (self.level_schedule and cfg.fixed and B <= 256)
            ctx.arena = arena
            ctx._pcache = self._pcache  # parameter name -> (shape, address): the arenas never move
            if (self.level_schedule and cfg.fixed and B <= 256) or getattr(self, "mha_bwd_form", 0) == 4:
                ctx.mha_bwd_form = 4
            cp.ctx = ctx
            new = (lambda n, dt=torch.float32: arena.alloc(n, dt).tensor()) if arena is not None else \
                (lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=self.device))
            cp.int_x = new(B * self.Fd).view(B, self.Fd)
            cp.cat_x = new(B * self.Fs, torch.int64).view(B, self.Fs)
            cp.y = new(B)
            cp.logits = new(B)
            cp.loss = new(1)
            cp.dlogits = new(B)
            int_buf = P.Buf(ctx, B * self.Fd, need_grad=False, tensor=cp.int_x)
            dense0 = P.DV(int_buf, 0, self.Fd, self.Fd)
            sbuf = ctx.buf(B * self.Fs * E)
            if row_grad_out is not None:
                assert row_grad_out.numel() == B * self.Fs * E and row_grad_out.dtype == torch.float32 and row_grad_out.is_contiguous()
                sbuf.g = row_grad_out
            sparse0 = P.SV(sbuf, 0, self.Fs, self.Fs * E)
            cp.sparse0 = sbuf
            ctx.raw_sparse = sbuf
            g = L.EmbedDesc()
            g.kind = L.OP_EMBED_GATHER
            g.B, g.Fs = B, self.Fs
            g.idx = cp.cat_x.data_ptr()
            g.table_dtype = L.TABLE_DTYPE_BF16 if self.tables_bf16 else L.TABLE_DTYPE_F32  # (the stage descriptor below copies it)
            if not self.host_embedding:
                for f in range(self.Fs):
                    g.table[f] = self.tables[f].data_ptr()
                    g.rows[f] = self.num_embeddings[f]
                g.out = sbuf.t.data_ptr()
                g.oob = self.oob.data_ptr()
            # the gather rides on the per-step staging launch (which holds the caller's id tensor anyway); cp.gather is the
            # stand-alone descriptor for the paths that stage by other means
            cp.gather = g
            st = L.StageDesc()
            st.kind = L.OP_STAGE_INPUTS
            st.B, st.Fd, st.Fs = B, self.Fd, self.Fs
            st.int_dst, st.cat_dst, st.y_dst = cp.int_x.data_ptr(), cp.cat_x.data_ptr(), cp.y.data_ptr()
            if not self.host_embedding:
                st.gather = g
            cp.stage = st
            d_last, s_last = P.network_walk(ctx, cfg, choice, dense0, sparse0)
            # final logit (supernet.py:592-598 / 657-664)
            fsegs, K = P.final_segments(d_last, s_last)
            w = ctx.param("_final.weight", (1, K))
            bptr = ctx.param("_final.bias", (1,))
            fd = L.FinalDesc()
            fd.kind = L.OP_FINAL_FWD
            fd.B, fd.nseg = B, len(fsegs)
            fd.w, fd.bias, fd.logits = w, bptr, cp.logits.data_ptr()
            for q, (s, ts) in enumerate(fsegs):
                fd.seg[q], fd.width[q], fd.ld[q], fd.off[q], fd.tok_stride[q] = s.view.ptr, s.width, s.view.ld, s.koff, ts
            ctx.emit(fd)
            if cfg.use_final_sigmoid:
                raise NotImplementedError("use_final_sigmoid is never enabled by the reference CLIs")
            scheduled = self.level_schedule and cfg.fixed and B <= 256
            cp.fwd_levels = cp.bwd_levels = None
            cp.dead_forward = []
            if train:  # (the backward program decides which forward results are read: built further down, before the packing)
                if spec.table_rule.state != "moments":  # (Adagrad's table state: Adam / SGD keep theirs in `moments` instead)
                    self._ensure_split_table_state(spec)
                self._build_training_tail(cp, ctx, w, bptr, fsegs, B, K, grad_scale)
            fwd_list = list(ctx.fwd)
            if self.dead_code_elimination and cfg.fixed:
                fwd_list, cp.dead_forward = S.eliminate_dead_forward(fwd_list, ctx.bwd if train else [])
            if scheduled:
                fwd_list = S.order_two_term_accumulates(fwd_list)
                fwd_descs, cp.fwd_levels = S.pack(S.chain_accumulates(fwd_list))
                self._resident_worklists(cp, fwd_descs)
            else:
                fwd_descs = fwd_list
            cp.fwd = Program(fwd_descs)
            cp.used_params = list(ctx.used_params)
            if train:
                bd, pre = cp.bce, cp._pre
                # The training programs fold BCEWithLogits into the final-logit backward (the first closure to run); bwd_core
                # keeps the plain one (d loss / d logits supplied by torch.autograd).
                fi = next(i for i, dsc in enumerate(ctx.bwd) if isinstance(dsc, L.FinalDesc))
                plain = ctx.bwd[fi]
                assert plain.kind == L.OP_FINAL_BWD
                fused = L.FinalDesc.from_buffer_copy(plain)
                fused.logits, fused.y, fused.loss, fused.dlogits_out = cp.logits.data_ptr(), cp.y.data_ptr(), cp.loss.data_ptr(), cp.dlogits.data_ptr()
                fused.grad_scale = bd.grad_scale
                cp.bce = bd
                bwd_descs = pre[1:] + ctx.bwd[:fi] + [fused] + ctx.bwd[fi + 1:]
                # forward + backward of a training step as ONE scheduled program: what the forward leaves off its critical path (a
                # block output no later block reads, second passes) runs beside the first backward levels
                # clip + Adagrad (built before the packing: the id-only half of its row dedup is an operator of the step like any other)
                odescs = []
                cp.ids_on_stage = False
                if local_optimizer:
                    odescs = self._optimizer_descs(cp.tail, B, cp.cat_x, sbuf.grad_tensor() if (sbuf.grad_written and not self.host_embedding)
                                                   else None, clip, eps)
                # decoupled weight decay: the batch's rows pay what they owe in front of the launch that gathers them
                cp.decay0 = cp.tail.decay0 if (local_optimizer and spec.dwd) else None
                ids_in_program = []
                ids = cp.tail.dedup_ids
                if ids is not None:
                    if scheduled and _IDS_AS_ITEM:
                        # ... which depends on nothing but the staged ids and is read by nothing before the optimizer: the level scheduler puts
                        # it where it costs least (beside a Transformer backward), off both the staging launch and the step's tail
                        ids_in_program = [ids]
                    elif B <= 256:  # on the staging launch (which holds the caller's ids)
                        cp.stage.dedup_ids = ids
                        cp.ids_on_stage = True
                    else:           # in-stream programs (large batch): in front of the launch that needs it
                        odescs = [ids] + odescs
                cp.fb = None
                if scheduled:
                    # (alloc: a forward product with several levels of slack may be re-cut into split-K items — only in the JOINT
                    # program, where the backward's latency-bound levels are there to hide it)
                    jf, jb = self._fuse_final(fwd_list, bwd_descs, fused) if _FUSE_FINAL else (fwd_list, bwd_descs)
                    jf, jb = self._fuse_head(jf, jb)
                    fb_descs = None
                    cp.persistent = False
                    cp.level_tuning = None
                    if persist:
                        try:
                            if spec.ema:
                                raise S.PersistRefused("a weight-EMA plan keeps the default launches")
                            fb_descs, cp.fb_levels = S.pack_persistent(
                                ids_in_program + jf + jb, lambda nb: torch.empty(max(int(nb), 16), dtype=torch.uint8, device=self.device),
                                arena.ranges, alloc=ctx.alloc)
                            cp.persistent = True
                            self._persist_errs += [d.err_tensor for d in fb_descs if isinstance(d, L.PersistDesc)]
                        except S.PersistRefused as e:
                            import warnings
                            warnings.warn("persistent step refused (%s): one launch per level instead" % (e,))
                    if fb_descs is None:
                        # (level launches only: same-target input gradients become chained items — the persistent form takes the program as it is)
                        joint = S.chain_accumulates(ids_in_program + jf + jb)
                        fb_descs, cp.fb_levels = S.pack(joint, alloc=ctx.alloc)
                        if _WL_TUNE and S.BALANCE:
                            fb_descs, cp.level_tuning = self._tune_levels(joint, ctx.alloc, fb_descs)
                    self._resident_worklists(cp, fb_descs)
                    cp.fb = Program(fb_descs)
                    bwd_descs, cp.bwd_levels = S.pack(S.chain_accumulates(bwd_descs))
                    self._resident_worklists(cp, bwd_descs)
                cp.bwd = Program(bwd_descs)
                cp.bwd_tail_start = len(pre) - 1 + ctx.bwd_tail_start  # cp.bwd.descs[this:] = the parked weight-gradient products
                cp.bwd_marks = [(b, len(pre) - 1 + idx) for b, idx in ctx.block_marks]  # block b's gradients complete after cp.bwd.descs[:idx]
                cp.bwd_core = Program(pre[1:] + ctx.bwd)  # dlogits supplied by the caller (autograd path)
                # fine-tune-last-layer mode (SuperNet.set_mode_to_finelune_last_only, the searcher's candidate evaluation):
                # only d loss / d _final is wanted, i.e. the weight part of the final-logit backward and nothing else
                last = L.FinalDesc.from_buffer_copy(plain)
                for q in range(L.MAX_SEGS):
                    last.dseg[q] = None
                tail = [ctx.bwd[fi + 1]] if plain.nsplit > 1 else []  # (the partial-sum launch of a split final backward)
                cp.bwd_final_only = Program(pre[1:] + [last] + tail)
                cp.opt = Program(odescs)
                if graph:
                    cp.step = Program((cp.fb.descs if cp.fb is not None else cp.fwd.descs + cp.bwd.descs) + cp.opt.descs)
                    cp.step.capture(self.stream.cuda_stream)
            elif graph:
                cp.fwd.capture(self.stream.cuda_stream)
        # launches of the plan's programs that run the bf16 body (0 at "highest"; forward + backward, each launch once)
        cp.bf16_launches = P.bf16_launches(cp.fwd.descs) + (P.bf16_launches(cp.bwd.descs) if train else 0)
        # ... and the large-batch token-axis launches among them that run theirs (csrc/token_linear_bf16.hip), counted apart
        cp.bf16_token_launches = P.bf16_token_launches(cp.fwd.descs) + (P.bf16_token_launches(cp.bwd.descs) if train else 0)
        if graph or arena is None or cfg.fixed:
            self.stream.synchronize()  # these plans are built (zero-filled, captured) on the private stream, and replayed on the caller's
        self._plans[key] = cp
        self._last_plan = (fast, choice, cp)
        return cp

    def _resident_worklists(self, cp, descs):
        """nasrec_worklist_prepare for every worklist launch of `descs` (a fixed plan: the pointers inside the items never change): the
        descriptor objects stay what they are (reports, tests, the data-parallel readiness model read them), a Program launches their
        `launch_as` — the device-resident form — instead"""
        if not _WL_RESIDENT:
            return
        lists = [d for d in descs if isinstance(d, L.WorklistDesc) and not hasattr(d, "launch_as")]
        if not lists:
            return
        lib = L.load()
        sz = (C.sizeof(L.WorklistDesc) + 255) & ~255
        buf = torch.empty(sz * len(lists), dtype=torch.uint8, device=self.device)
        if not hasattr(cp, "_wl_resident"):
            cp._wl_resident = []
        cp._wl_resident.append(buf)  # (owned by the plan)
        self.stream.synchronize()  # (the copies below are synchronous on the null stream)
        for i, d in enumerate(lists):
            dv = L.WorklistDevDesc()
            L.check(lib.nasrec_worklist_prepare(C.addressof(d), buf.data_ptr() + i * sz, C.addressof(dv)))
            d.launch_as = dv

    def _tune_levels(self, prog_in, alloc, default_descs):
        """The balancing pass of schedule.pack places slack operators by a duration MODEL whose least certain entries are the Transformer
        bodies (one workgroup per sample: how much of their time other items can share depends on what those items are).  A fixed
        sub-network's batch-256 plan is compiled once and run for an epoch, so the model's Transformer durations are treated as knobs:
        the joint program is packed for a handful of settings (schedule.TUNE_MHA_NS), every distinct schedule is replayed on the plan's
        own (zero-filled) buffers, and the fastest one wins if it beats the default by more than the timing noise.  Any schedule gives
        the same bits (same bodies, same operands, dependencies respected: tests/test_parity_gpu.py), so this only moves time.
        Returns (descriptors, report)."""
        sp = self.stream.cuda_stream

        def sig(descs):
            return hash(b"".join(bytes(d) for d in descs))

        def run_ms(prog, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            for _ in range(reps):
                prog.run(sp)
            e1.record(self.stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        keep = list(S._MHA_NS)
        cands = [("default", default_descs)]
        seen = {sig(default_descs)}
        try:
            for ns in S.TUNE_MHA_NS:
                S._MHA_NS[:] = list(ns) + keep[len(ns):]
                descs, _ = S.pack(prog_in, alloc=alloc)
                h = sig(descs)
                if h not in seen:
                    seen.add(h)
                    cands.append((",".join(str(v) for v in ns), descs))
        finally:
            S._MHA_NS[:] = keep
        if len(cands) == 1:
            return default_descs, {"candidates": 1, "chosen": "default"}
        progs = [(name, descs, Program(descs)) for name, descs in cands]
        for _, _, pg in progs:
            run_ms(pg, 5)  # descriptors and code warm
        times = {name: [] for name, _, _ in progs}
        for _ in range(5):  # interleaved rounds: clock and cache drift hits every candidate alike
            for name, _, pg in progs:
                times[name].append(run_ms(pg, 20))
        med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
        best = min(med, key=med.get)
        if med[best] > med["default"] * (1.0 - _WL_TUNE_MARGIN):
            best = "default"
        chosen = next(descs for name, descs, _ in progs if name == best)
        return chosen, {"candidates": len(progs), "chosen": best, "ms": {k: round(v, 5) for k, v in med.items()}}

    def _build_training_tail(self, cp, ctx, w, bptr, fsegs, B, K, grad_scale):
        """BCE descriptor, the final-logit backward closure, the backward program (ctx.bwd) and, for a supernet, the path's chunk
        table: everything the forward packing has to know about (which forward results the backward reads)"""
        cfg, arena = self.cfg, cp.arena
        bd = L.BceDesc()
        bd.kind = L.OP_BCE
        bd.B = B
        bd.grad_scale = grad_scale if grad_scale is not None else 1.0 / B
        bd.logits, bd.y, bd.loss, bd.dlogits = cp.logits.data_ptr(), cp.y.data_ptr(), cp.loss.data_ptr(), cp.dlogits.data_ptr()
        pre = [bd]

        def final_bwd():
            e = L.FinalDesc()
            e.kind = L.OP_FINAL_BWD
            e.B, e.nseg = B, len(fsegs)
            e.w, e.bias, e.dlogits = w, bptr, cp.dlogits.data_ptr()
            e.dw, e.dbias = self.grads["_final.weight"].data_ptr(), self.grads["_final.bias"].data_ptr()
            for q, (s, ts) in enumerate(fsegs):
                gp, acc = ctx.gtarget(s.view)
                e.seg[q], e.dseg[q], e.width[q], e.ld[q], e.off[q], e.dseg_accumulate[q] = s.view.ptr, gp, s.width, s.view.ld, s.koff, acc
                e.tok_stride[q] = ts
            if B > 256:
                # d loss / d _final over a large batch: nsplit batch slices in parallel -> partial [nsplit, K + 1], summed in
                # fixed order by the launch behind it (one workgroup per 16 columns walked 4096 rows in 132 us)
                e.nsplit = max(2, min(32, B // 128))
                part = ctx.alloc(e.nsplit * (K + 1))
                e.dw = part.data_ptr()
                r = L.ReduceRowsDesc()
                r.kind = L.OP_REDUCE_ROWS
                r.R, r.C, r.ld, r.in_ = e.nsplit, K + 1, K + 1, part.data_ptr()
                r.ndst = 2
                r.dst[0], r.dst_off[0], r.dst_len[0] = self.grads["_final.weight"].data_ptr(), 0, K
                r.dst[1], r.dst_off[1], r.dst_len[1] = self.grads["_final.bias"].data_ptr(), K, 1
                ctx.emit(e)
                ctx.emit(r)
                return
            ctx.emit(e)

        ctx.on_backward(final_bwd)
        ctx.build_backward()
        cp.path_spans = None
        t = cp.tail
        if not cfg.fixed:
            # Paths differ from step to step.  torch skips parameters whose grad is None (everything outside the path),
            # so zero_grad, the norm and Adagrad touch ONLY the arena ranges this path trains — the same arithmetic on
            # the path's share of the arena (a quarter of it for a `default` xlarge path).  Gradients left over from
            # other paths outside these ranges are never read.
            names = [n for n in list(ctx.grad_params) + ["_final.weight", "_final.bias"] if not n.startswith("_embedding.")]
            cp.path_spans = [(self.offsets[n], self.params[n].numel()) for n in dict.fromkeys(names)]
            flat = P.path_chunks(cp.path_spans)
            t.chunk_tab, t.nchunks = self._const_table(flat, arena, pre), len(flat) // 2
            ms = P.memset_desc(self.flat_g)
            ms.chunks, ms.nchunks = t.chunk_tab.data_ptr(), t.nchunks
            pre.append(ms)
        elif _FIXED_OPT_TABLE:
            # A fixed sub-network can hold parameters no gradient ever reaches (the reference leaves their grad None: in
            # ea_criteo_kaggle_xlarge_best_1shot.json all of block 5, 1.2 M of the 2.2 M dense parameters — no later block selects it).
            # Their gradient stays zero, and Adagrad with g = 0 changes neither state nor parameter: the norm and the update walk a chunk
            # table of the trained ranges only (half the bytes of the optimizer's bandwidth-bound pass).  Written once, here.
            names = [n for n in list(ctx.grad_params) + ["_final.weight", "_final.bias"] if not n.startswith("_embedding.")]
            spans = [(self.offsets[n], self.params[n].numel()) for n in dict.fromkeys(names)]
            if sum(n for _, n in spans) < 0.9 * self.flat_numel:
                flat = P.path_chunks(spans, chunk=1024)  # (small pieces: a workgroup per piece keeps ~10^3 workgroups on the pass)
                t.chunk_tab, t.nchunks = self._const_table(flat, arena, pre), len(flat) // 2
        if t.spec.wd:
            self._weight_decay_tables(t, ctx, arena, pre)
        if t.spec.moments:
            self._moments_tables(cp, ctx, arena, pre)
        if t.spec.dwd:
            self._decay_tables(t, ctx, arena, pre)
        cp.bce, cp._pre = bd, pre

    def _const_table(self, flat, arena, pre):
        """an int64 table holding `flat`: a sampled path's lives in the plan slot's arena and is written by launches in front of every
        step (`pre`: the slot is reused by other paths); a fixed sub-network's is written once, now"""
        n = max(1, len(flat))
        if not self.cfg.fixed:
            tab = arena.alloc(n, torch.int64).tensor()
            pre += P.const_i64_descs(tab.data_ptr(), flat)
            return tab
        tab = torch.empty(n, dtype=torch.int64, device=self.device)
        lib = L.load()
        for dsc in P.const_i64_descs(tab.data_ptr(), flat):
            L.check(lib.nasrec_launch(self.stream.cuda_stream, C.addressof(dsc)))
        self.stream.synchronize()  # (the descriptors carry the values: they must outlive their launches)
        return tab

    WD_BLOCKS = 2048  # workgroups of the two weight-decay launches (8 per CU: the table pass is a stream over W and its state)

    def _weight_decay_tables(self, t, ctx, arena, pre):
        """Chunk tables of a plan with weight decay (csrc/weight_decay.hip): the regularised dense ranges the backward reaches (g += 2 wd W)
        and the ones it does not (g = 2 wd W: get_l2_loss walks named_parameters(), on the path or off it), and the union of the reached
        and the regularised ranges, over which Adagrad runs (torch skips grad = None: 1-D parameters off the path).  The clip's sum of
        squares keeps the reached ranges only — a fixed sub-network gets that table whatever its share of the arena."""
        names = [n for n in list(ctx.grad_params) + ["_final.weight", "_final.bias"] if not n.startswith("_embedding.")]
        reached = list(dict.fromkeys(names))
        reg, t.wd_tables = P.regularised(self.shapes, t.spec.no_reg)
        on = set(reached)

        def chunks(ns):
            return P.path_chunks([(self.offsets[n], self.params[n].numel()) for n in ns], chunk=1024)
        parts = [chunks([n for n in reg if n in on]), chunks([n for n in reg if n not in on]), chunks(list(dict.fromkeys(reached + reg)))]
        if t.chunk_tab is None:
            parts.append(chunks(reached))
        tab = self._const_table([v for part in parts for v in part], arena, pre)
        ptrs, off = [], 0
        for part in parts:
            ptrs.append((tab.data_ptr() + 8 * off, len(part) // 2))
            off += len(part)
        t.wd_add, t.wd_set, t.wd_union = ptrs[:3]
        if t.chunk_tab is None:
            t.chunk_tab, t.nchunks = tab[off - len(parts[3]):off], ptrs[3][1]
        t.wd_tab = tab
        self._row_bitmap()
        if getattr(self, "_wd_part", None) is None:
            with torch.cuda.stream(self.stream):
                self._wd_part = torch.zeros(2 * self.WD_BLOCKS, dtype=torch.float64, device=self.device)
                self._wd_counter = torch.zeros(1, dtype=torch.int32, device=self.device)
                self.wd_l2_sumsq = torch.zeros(1, dtype=torch.float64, device=self.device)
            self.stream.synchronize()

    def _row_bitmap(self, sink: bool = False):
        """engine-wide bitmap of touched table rows, 64-row tiles (csrc/weight_decay.hip, csrc/optim_moments.hip): every plan leaves it
        all zero behind its step.  sink: one of the same size that is written and never read"""
        name = "_wd_sink" if sink else "_wd_bitmap"
        t = getattr(self, name, None)
        if t is None:
            words = sum(2 * ((n + 63) // 64) for n in self.num_embeddings)
            with torch.cuda.stream(self.stream):
                t = torch.zeros(max(1, words), dtype=torch.int32, device=self.device)
            self.stream.synchronize()
            setattr(self, name, t)
        return t

    def ensure_moments_state(self, kind: str, tables: bool = True, rowwise_v: bool = False):
        """Adam's exp_avg / exp_avg_sq or SGD's momentum_buffer for the dense arena (flat, the layout of flat_p) and for every table,
        allocated on first use, zero; and the per-parameter step counters (dense parameters in dense_names order, then the tables).
        tables = False (the split optimizer, OptimSpec.table_kind): the dense arena's arrays only — the tables' state is Adagrad's
        `table_state` (row-wise: `table_row_state`), and no moment array the size of a table is allocated ([] until a plan that needs them asks).
        "rmsprop": square_avg, and `lazy_stamps` — per table one int32 per row, the table's step count at which that row's square_avg
        is current (csrc/optim_moments.hip); engine-private, never part of optimizer.state.
        rowwise_v (row-wise Adam, OptimSpec.table_kind "rowwise_adam"): a table's exp_avg_sq is ONE float per row, [rows] — the
        [rows, 16] array is never allocated; an engine keeps one form, and asking for the other is refused.
        -> {state key: (flat arena, [table arrays])}"""
        if tables:
            self._refuse_bf16_tables("%s on every table row (its table moments)" % kind)
        keys = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",)}.get(kind, ("momentum_buffer",))
        st = self.__dict__.setdefault("moments", {})
        held = st.get("exp_avg_sq", (None, []))[1]
        if tables and kind == "adam" and held and (held[0].dim() == 1) != bool(rowwise_v):
            raise L.EngineError("this engine holds the tables' exp_avg_sq %s: Adam's second moment per %s on the tables needs an engine "
                                "of its own (RowSparseAdam / torch.optim.Adam and RowwiseSparseAdam do not share table moments)"
                                % (("per row ([rows])", "element") if held[0].dim() == 1 else ("per element ([rows, 16])", "row")))
        with torch.cuda.stream(self.stream):
            for k in keys:
                if k not in st:
                    st[k] = (torch.zeros(self.flat_numel, dtype=torch.float32, device=self.device), [])
                if tables and not st[k][1]:
                    if rowwise_v and k == "exp_avg_sq":
                        st[k][1].extend(torch.zeros(t.shape[0], dtype=torch.float32, device=self.device) for t in self.tables)
                    else:
                        st[k][1].extend(torch.zeros_like(t) for t in self.tables)
            if kind == "rmsprop" and getattr(self, "lazy_stamps", None) is None:
                self.lazy_stamps = [torch.zeros(n, dtype=torch.int32, device=self.device) for n in self.num_embeddings]
            if getattr(self, "opt_steps", None) is None:
                self.opt_steps = torch.zeros(len(self.dense_names) + self.Fs, dtype=torch.float32, device=self.device)
                self._mom_counter = torch.zeros(1, dtype=torch.int32, device=self.device)
                self.param_index = {n: i for i, n in enumerate(self.dense_names)}
                for f in range(self.Fs):
                    self.param_index["_embedding.%d.weight" % f] = len(self.dense_names) + f
        self.stream.synchronize()
        return {k: st[k] for k in keys}

    def moments_view(self, key: str, name: str):
        """engine storage of moment `key` of parameter `name` (shape of the parameter; a table's exp_avg_sq under row-wise Adam: [rows])"""
        flat, tabs = self.moments[key]
        if name.startswith("_embedding."):
            if not tabs:
                raise L.EngineError("no %s of %s: with Adagrad on the tables (OptimSpec.table_kind) their state is table_state, "
                                    "Adagrad's sum (row-wise: table_row_state)" % (key, name))
            return tabs[int(name.split(".")[1])]
        o, n = self.offsets[name], self.params[name].numel()
        return flat[o:o + n].view(self.params[name].shape)

    def _tile_layout(self, d, owns):
        """table[f], rows[f] and the untouched-row pass's layout of 64-row tiles on descriptor `d`: table f owns the tiles
        [tile_off[f], tile_off[f + 1]) where owns(f), none otherwise (the pass leaves it alone) -> bit mask of the tables that own tiles"""
        mask, tile = 0, 0
        for f in range(self.Fs):
            d.table[f], d.rows[f], d.tile_off[f] = self.tables[f].data_ptr(), self.num_embeddings[f], tile
            if owns(f):
                mask |= 1 << f
                tile += (self.num_embeddings[f] + 63) // 64
        d.tile_off[self.Fs] = tile
        return mask

    def _flush_desc(self):
        """RMSprop's flush launch (phase 2): every row of every table, in 64-row tiles"""
        m = L.OptMomentsDesc()
        m.kind, m.phase, m.algo = L.OP_OPT_MOMENTS, 2, L.OPTIM_RMSPROP
        m.nblocks, m.Fs, m.table_step0 = self.WD_BLOCKS, self.Fs, len(self.dense_names)
        m.beta2 = self._lazy_alpha
        self._tile_layout(m, lambda f: True)
        for f in range(self.Fs):
            m.tv[f], m.tm[f] = self.moments["square_avg"][1][f].data_ptr(), self.lazy_stamps[f].data_ptr()
        m.bitmap = self._row_bitmap().data_ptr()
        m.step, m.lr = self.opt_steps.data_ptr(), self.lr_dev.data_ptr()
        return m

    def flush_lazy_rows(self):
        """RMSprop: bring square_avg of every table row current (a row outside the batches owes it alpha^n since its stamp) — what a
        reader of the state needs: optimizer.state_dict(), a torch step on the aliased state, the broadcast to replicas.  One streaming
        launch on the engine's stream, waited for; a no-op before the first RMSprop plan and when nothing is owed."""
        if getattr(self, "lazy_stamps", None) is None or getattr(self, "_lazy_alpha", None) is None:
            return
        m = self._flush_desc()
        L.check(L.load().nasrec_opt_moments(self.stream.cuda_stream, C.addressof(m)))
        self.stream.synchronize()  # (the reader may sit on another stream)

    MOM_CHUNK = 1024  # elements per dense chunk of the Adam / SGD launch (one parameter per chunk)

    def _moments_tables(self, cp, ctx, arena, pre):
        """Chunk table of a plan with Adam / SGD (csrc/optim_moments.hip): [offset, length, parameter] triples over the parameters the
        step updates — the reached ones (torch skips grad = None) plus, with weight decay, the regularised ones — then the step-counter
        indices of those parameters and of the tables that move: all of them when the path's backward reaches the embedding stem, else
        (grad None in torch) only the regularised ones with weight decay, none without.  Always a table: unlike Adagrad, g = 0 is not a
        no-op.  Row-sparse Adam (spec.sparse_rows) counts the same steps; its tables move in the batch's rows only (_moments_descs)."""
        if self.host_embedding:
            raise L.EngineError("Adam / SGD in the fused step need the embedding tables on the device")
        t = cp.tail
        spec = t.spec
        rule = spec.table_rule
        if rule.rows_only and spec.wd and P.regularised(self.shapes, spec.no_reg)[1]:
            raise L.EngineError("%s with a regularised table: the L2 term puts a gradient on every row; leave the tables out "
                                "(no_reg_param_name='_embedding') or use weight_decay=0" % rule.phrase)
        self.ensure_moments_state(spec.kind, tables=rule.state == "moments", rowwise_v=spec.rowwise_adam)
        names = [n for n in list(ctx.grad_params) + ["_final.weight", "_final.bias"] if not n.startswith("_embedding.")]
        if spec.wd:
            names += P.regularised(self.shapes, spec.no_reg)[0]
        names = list(dict.fromkeys(names))
        trip = []
        for n in names:
            off, cnt, k = self.offsets[n], self.params[n].numel(), self.param_index[n]
            for o in range(0, cnt, self.MOM_CHUNK):
                trip += [off + o, min(self.MOM_CHUNK, cnt - o), k]
        if cp.sparse0.grad_written:
            t.mom_tables = list(range(self.Fs))
        else:
            t.mom_tables = sorted(t.wd_tables) if spec.wd else []
        inc = [self.param_index[n] for n in names] + [len(self.dense_names) + f for f in t.mom_tables]
        tab = t.mom_tab = self._const_table(trip + inc, arena, pre)
        t.mom_chunks = (tab.data_ptr(), len(trip) // 3)
        t.mom_inc = (tab.data_ptr() + 8 * len(trip), len(inc))
        t.mom_names = names

    @staticmethod
    def _optim_scalars(d, spec):
        """algo and hyperparameters of an Adam / SGD spec on an OptMomentsDesc or a LastLayerStepDesc"""
        if spec.table_kind and spec.kind not in spec.table_rule.kinds:  # (an unknown table_kind goes with no kind)
            raise L.EngineError("table_kind %r with %s: the tables' own rules (Adagrad, row-wise Adagrad, row-wise Adam) go with Adam on "
                                "the dense parameters" % (spec.table_kind, spec.kind))
        d.algo = {"adam": L.OPTIM_ADAM, "rmsprop": L.OPTIM_RMSPROP}.get(spec.kind, L.OPTIM_SGD)
        d.eps, d.momentum, d.nesterov = spec.eps, spec.momentum, int(bool(spec.nesterov))
        d.beta1, d.beta2 = spec.beta1, (spec.alpha if spec.kind == "rmsprop" else spec.beta2)  # (RMSprop's alpha travels in beta2)

    def _moments_descs(self, t, Bg, cat_x, gsum, clip_desc, rank_layout=None):
        """the two NASREC_OP_OPT_MOMENTS launches of a plan with Adam / SGD: (phase 0 in place of the Adagrad apply launch, phase 1).
        rank_layout: (samples per rank, floats between the ranks' chunks) of `gsum` (_optimizer_descs).
        What differs between the tables' rules is read from spec.table_rule (optim_spec.TableRule).  A rows-only rule: no table owns a
        tile, and phase 1 is None unless weight decay left unreached ranges of g to restore — phase 0 then counts the steps itself;
        with them phase 1 runs in its no-table-moves form on all its workgroups (the ranges of a supernet are millions of floats).
        RMSprop: m is unused and the slots of `tm` carry the stamps.  Adagrad on the tables: tv carries the rule's state array, tm
        nothing (bf16 tables: the rounding's seed in tm[0]'s storage — constant from step to step: the kernel reads the step count on
        the device).  Row-wise Adam: tm carries exp_avg [rows, 16], tv exp_avg_sq [rows]."""
        spec = t.spec
        st = self.moments
        rule = spec.table_rule
        lazy = rule.rows_only  # (the tables move in the batch's rows only)
        split = rule.state != "moments"  # (Adagrad's accumulators, table_state or table_row_state, stand in for the tables' moments)
        if rule.bf16 != self.tables_bf16:
            raise L.EngineError("table_kind %r on %s tables" % (spec.table_kind, "bf16" if self.tables_bf16 else "fp32"))
        m = L.OptMomentsDesc()
        m.kind, m.phase = L.OP_OPT_MOMENTS, 0
        self._optim_scalars(m, spec)
        m.dense_blocks = min(2048, t.mom_chunks[1])
        m.sparse_rows, m.table_algo = int(bool(spec.sparse_rows)), rule.table_algo
        if split:
            m.table_eps, m.table_lr_scale = spec.table_eps, spec.table_lr_scale
        m.nblocks = self.WD_BLOCKS if (t.mom_tables or lazy) else 1  # (no table moves: phase 1 only counts the step and restores g)
        m.B, m.Fs = (Bg, self.Fs) if gsum is not None else (0, self.Fs)
        m.table_step0 = len(self.dense_names)
        m.wd = spec.wd
        m.clip = clip_desc
        m.chunks, m.nchunks = t.mom_chunks
        m.p, m.g = self.flat_p.data_ptr(), self.flat_g.data_ptr()
        if spec.kind == "rmsprop":
            first, second = (None, self.lazy_stamps), st["square_avg"]
            self._lazy_alpha = float(spec.alpha)
        else:
            first, second = (st["exp_avg"], st["exp_avg_sq"]) if spec.kind == "adam" else (st["momentum_buffer"], None)
        m.m = first[0].data_ptr() if first[0] is not None else None
        m.v = second[0].data_ptr() if second is not None else None
        if gsum is not None:
            m.idx, m.leader, m.gsum = cat_x.data_ptr(), t.bufs.leader.data_ptr(), gsum
            if rank_layout:
                m.rank_B, m.rank_stride = rank_layout
        self._tile_layout(m, lambda f: f in t.mom_tables and not lazy)  # (a table that does not move owns no tile)
        for f in range(self.Fs):
            if split:  # (Adagrad's accumulators; the kernel never looks at tm)
                m.tv[f] = getattr(self, rule.state)[f].data_ptr()
                continue
            m.tm[f] = first[1][f].data_ptr()
            if second is not None:
                if second[1][f].dim() != (1 if rule.rowwise else 2):  # (the kernel indexes tv by row or by element: never the other array)
                    raise L.EngineError("exp_avg_sq of table %d has shape %s under table_kind %r" % (f, tuple(second[1][f].shape), spec.table_kind))
                m.tv[f] = second[1][f].data_ptr()
        if rule.bf16:
            m.sr_seed = spec.table_seed  # (over tm[0], which the loop above left null)
        m.reg_mask = sum(1 << f for f in t.wd_tables) if spec.wd else 0
        m.bitmap = self._row_bitmap().data_ptr()
        m.step = self.opt_steps.data_ptr()
        m.inc, m.n_inc = t.mom_inc
        if spec.wd:
            m.zero_chunks, m.n_zero = t.wd_set
        m.counter = self._mom_counter.data_ptr()
        m.lr, m.coef = self.lr_dev.data_ptr(), self.clip_out.data_ptr()
        if lazy and not m.n_zero:
            return m, None
        m1 = L.OptMomentsDesc.from_buffer_copy(m)
        m1.phase = 1
        return m, m1

    def _weight_decay_descs(self, t, Bg, cat_x, gsum, eps, clip_partial, rank_layout=None):
        """the two NASREC_OP_WEIGHT_DECAY launches of a plan: (phase 0, in front of the clip; phase 1, behind the touched rows' Adagrad).
        rank_layout: (samples per rank, floats between the ranks' chunks) of `gsum` (_optimizer_descs)"""
        self._refuse_bf16_tables("weight decay (its two phases)")
        w = L.WeightDecayDesc()
        w.kind, w.phase, w.nblocks = L.OP_WEIGHT_DECAY, 0, self.WD_BLOCKS
        w.wd, w.eps = t.spec.wd, eps
        w.B, w.Fs = (Bg, self.Fs) if gsum is not None else (0, self.Fs)
        if gsum is not None:
            w.idx, w.leader, w.gsum = cat_x.data_ptr(), t.bufs.leader.data_ptr(), gsum
            if rank_layout:
                w.rank_B, w.rank_stride = rank_layout
        mask = w.reg_mask = self._tile_layout(w, lambda f: f in t.wd_tables)
        if self.table_state is not None:  # (read by phase 1 only, which Adam / SGD plans do not launch)
            for f in range(self.Fs):
                w.state[f] = self.table_state[f].data_ptr()
        w.bitmap = self._row_bitmap().data_ptr()
        if t.spec.moments and mask != (1 << self.Fs) - 1:
            # Adam / SGD mark the touched rows of EVERY table, in a layout over all tables: phase 0's marks (over the regularised
            # tables) would land on other rows' bits there, so they go to a bitmap nobody reads
            w.bitmap = self._row_bitmap(sink=True).data_ptr()
        w.p, w.g = self.flat_p.data_ptr(), self.flat_g.data_ptr()
        (w.add_chunks, w.n_add), (w.set_chunks, w.n_set) = t.wd_add, t.wd_set
        w.block_part, w.counter = self._wd_part.data_ptr(), self._wd_counter.data_ptr()
        w.clip_partial, w.l2_sumsq = clip_partial, self.wd_l2_sumsq.data_ptr()
        w.lr, w.coef = self.lr_dev.data_ptr(), self.clip_out.data_ptr()
        w1 = L.WeightDecayDesc.from_buffer_copy(w)
        w1.phase = 1
        return w, w1

    def _optimizer_descs(self, t, Bg, cat_x, sparse_grad, clip, eps, rank_layout=None):
        """clip_grad_norm_ + the optimizer of `t` (an OptimizerTail; train_utils.py:285-286): row-sparse on the tables, flat on the dense
        arena.  One fixed sequence: the reduce stage (row dedup + the sums of squares), weight decay's phase 0, the apply stage (clip +
        Adagrad, or phase 0 of Adam / SGD) and the phase-1 stage (weight decay's, or Adam / SGD's).  eps: Adagrad's.
        rank_layout (data-parallel step): (samples per rank, floats between the ranks' chunks) of `sparse_grad` when it is the receive
        buffer of an all-gather that carries more than the rows (parallel.py); None = one contiguous [Bg, Fs, 16] array.  Weight decay and
        Adam / SGD read and write the summed rows where the dedup left them: in that layout (Bg <= DEDUP_SPLIT_MAX_B, summed in place) or
        in the contiguous gsum (the one-launch kernels).
        Leaves `t.dedup_ids` (the id-only half of the row dedup, to be launched once the ids are in `cat_x`) or None."""
        spec, b = t.spec, t.bufs
        assert spec.moments or spec.eps == eps, "Adagrad's eps: the spec's and the argument disagree"
        t.dedup_ids = None
        nb = (Bg + 255) // 256
        new = (lambda n, dt=torch.float32: t.arena.alloc(n, dt).tensor()) if t.arena is not None else \
            (lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=self.device))
        nblk = max(1, min(256, (self.flat_numel + 256 * 8 - 1) // (256 * 8)))
        tab, ntab = t.chunk_tab, t.nchunks
        if tab is not None:
            nblk = max(1, min(256, ntab))
        if b.leader is None:
            b.leader = new(Bg * self.Fs, torch.int32)
            b.gsum = new(Bg * self.Fs * E)
            b.emb_partial = new(self.Fs * nb)
            b.dense_partial = new(256 + (1 if spec.wd else 0))  # (weight decay: + phase 0's share of the norm)
        rows = sparse_grad is not None
        if rows:
            dd = L.EmbDedupDesc()
            dd.kind = L.OP_EMB_DEDUP
            dd.B, dd.Fs = Bg, self.Fs
            dd.idx, dd.dout = cat_x.data_ptr(), sparse_grad.data_ptr()
            dd.leader, dd.gsum, dd.sumsq_partial = b.leader.data_ptr(), b.gsum.data_ptr(), b.emb_partial.data_ptr()
            dd.overflow = self.oob.data_ptr() + 4
        sq = L.SumsqDesc()
        sq.kind = L.OP_SUMSQ
        sq.nblocks, sq.n = nblk, self.flat_numel
        sq.x, sq.partial = self.flat_g.data_ptr(), b.dense_partial.data_ptr()
        if tab is not None:
            sq.chunks, sq.nchunks = tab.data_ptr(), ntab
        cc = L.ClipCoefDesc()
        cc.kind = L.OP_CLIP_COEF
        cc.n_a, cc.n_b = nblk, (self.Fs * nb if rows else 0)
        cc.max_norm = float(clip) if clip is not None else 0.0
        cc.partial_a, cc.partial_b, cc.out = b.dense_partial.data_ptr(), b.emb_partial.data_ptr(), self.clip_out.data_ptr()
        wd_part = None
        if spec.wd:
            cc.n_a = nblk + 1  # partial_a[nblk]: what the L2 gradient adds to the norm's sum of squares (weight-decay phase 0)
            wd_part = b.dense_partial.data_ptr() + 4 * nblk
        ad = L.AdagradDenseDesc()
        ad.kind = L.OP_ADAGRAD_DENSE
        ad.eps, ad.n = eps, self.flat_numel
        ad.p, ad.g, ad.state = self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_s.data_ptr()
        ad.lr, ad.coef = self.lr_dev.data_ptr(), self.clip_out.data_ptr()
        if tab is not None:
            ad.chunks, ad.nchunks = tab.data_ptr(), ntab
        if spec.wd:  # Adagrad over the reached AND the regularised ranges
            (ad.chunks, ad.nchunks), ntab = t.wd_union, t.wd_union[1]
        if rows:
            ar = L.AdagradRowsDesc()
            ar.kind = L.OP_ADAGRAD_ROWS
            ar.B, ar.Fs, ar.eps = Bg, self.Fs, eps
            ar.idx, ar.leader, ar.gsum = cat_x.data_ptr(), b.leader.data_ptr(), b.gsum.data_ptr()
            for f in range(self.Fs):
                ar.table[f] = self.tables[f].data_ptr()
                ar.state[f] = self.table_state[f].data_ptr() if self.table_state is not None else None  # (None: an Adam / SGD plan)
                ar.rows[f] = self.num_embeddings[f]
            ar.lr, ar.coef = self.lr_dev.data_ptr(), self.clip_out.data_ptr()
            app = L.OptApplyDesc()
            app.kind = L.OP_OPT_APPLY
            # (2.2 M parameters of the batch-256 bench network: 256 / 512 / 1024 / 2048 / 4096 workgroups -> 15.3 / 10.9 / 8.6 / 9.5 / 10.8 us)
            cap = 1024 if self.flat_numel <= (4 << 20) else 2048
            app.dense_blocks = min(cap, ntab if tab is not None else (self.flat_numel + 255) // 256)
            app.clip, app.dense, app.rows = cc, ad, ar
        # the reduce stage, and where the summed rows are for weight decay and Adam / SGD
        if rows and Bg <= DEDUP_SPLIT_MAX_B:
            # Two halves (csrc/dedup_bodies.h): leaders, duplicate lists and their order depend on the ids only — t.dedup_ids runs
            # as soon as the ids are there (B <= 256: on the staging launch; a data-parallel step: behind the ids all-gather, beside the
            # forward) — and one launch behind the backward sums the duplicate rows IN PLACE and squares what the clip needs.
            capn = 256
            while capn < Bg:
                capn *= 2
            if b.dd_order is None:
                b.dd_order = new(self.Fs * capn, torch.int32)
                b.dd_lists = new(self.Fs * capn, torch.int32)
                b.dd_counts = new(self.Fs * 2, torch.int32)
                b.dd_heads = new(self.Fs * capn, torch.int32) if capn > 256 else None
            row_blocks = max(1, min(512, (Bg * self.Fs * 4 + 255) // 256))
            if b.emb_partial2 is None:
                b.emb_partial2 = new(self.Fs + row_blocks)
            assert b.emb_partial2.numel() >= self.Fs + row_blocks, "the work buffers are sized by the first program that uses them"
            ids = L.DedupIdsDesc()
            ids.kind, ids.B, ids.Fs, ids.cap = L.OP_DEDUP_IDS, Bg, self.Fs, capn
            ids.idx, ids.leader = cat_x.data_ptr(), b.leader.data_ptr()
            ids.order, ids.lists, ids.counts = b.dd_order.data_ptr(), b.dd_lists.data_ptr(), b.dd_counts.data_ptr()
            ids.heads = b.dd_heads.data_ptr() if b.dd_heads is not None else None
            t.dedup_ids = ids
            r2 = L.OptReduce2Desc()
            r2.kind, r2.B, r2.Fs, r2.cap = L.OP_OPT_REDUCE2, Bg, self.Fs, capn
            r2.rank_B, r2.rank_stride = rank_layout if rank_layout else (0, 0)
            r2.row_blocks = row_blocks
            r2.rows, r2.leader = sparse_grad.data_ptr(), b.leader.data_ptr()
            r2.order, r2.lists, r2.counts, r2.heads = ids.order, ids.lists, ids.counts, ids.heads
            r2.sumsq_partial = b.emb_partial2.data_ptr()
            r2.sumsq = sq
            app.clip.partial_b, app.clip.n_b = b.emb_partial2.data_ptr(), self.Fs + row_blocks
            app.rows.gsum = sparse_grad.data_ptr()  # summed in place: a leader's row holds its sum
            app.rows.rank_B, app.rows.rank_stride = r2.rank_B, r2.rank_stride
            reduce, gsum, layout = [r2], sparse_grad.data_ptr(), rank_layout
        elif rows:
            if rank_layout:  # (the one-launch kernels read the rows where the all-gather left them; their sums go to the contiguous gsum)
                dd.rank_B, dd.rank_stride = rank_layout
            reduce = [dd, sq]  # (global batch of a data-parallel step: chunked dedup + merge, two launches)
            if Bg <= 256:  # (NASREC_DEDUP_SPLIT_MAX_B below 256) the five launches collapse into the two the grid-wide dependencies require
                red = L.OptReduceDesc()
                red.kind = L.OP_OPT_REDUCE
                red.dedup, red.sumsq = dd, sq
                reduce = [red]
            gsum, layout = b.gsum.data_ptr(), None
        else:  # (no gradient reaches the embedding stem: no touched rows)
            reduce, gsum, layout = [sq], None, None
        wd0, phase1 = None, None
        if spec.wd:
            wd0, phase1 = self._weight_decay_descs(t, Bg, cat_x, gsum, eps, wd_part, layout)
        if spec.moments:
            m0, phase1 = self._moments_descs(t, Bg, cat_x, gsum, app.clip if rows else cc, layout)
            apply = [m0]
        else:
            apply = [app] if rows else [cc, ad]
        ema0, ema1 = [], []
        if spec.ema:
            # the weight average (csrc/weight_ema.hip): the batch's rows pay what they owe once the leaders are known and before
            # anything moves them; every parameter is averaged behind the last launch that writes one
            ema0, ema1 = self._ema_step_descs(spec, Bg if rows else 0, cat_x, b.leader)
        dec1 = []
        if spec.dwd:
            # decoupled weight decay (csrc/decoupled_decay.hip): torch's order — the L2 term's gradient of the weights as they were,
            # then p (1 - lr lambda), then the update
            dec1 = self._decay_step_descs(t, Bg, rows, cat_x, b.leader)
        cw0, cw1 = [], []
        if rows and t.cowclip is not None:
            # CowClip (csrc/cowclip.hip): the ids are counted beside the reduce stage; the leaders' summed rows are scaled directly in
            # front of the apply stage, behind the decoupled decay, whose launch has paid a touched row's debt: current weights
            if rank_layout:
                raise L.EngineError("cowclip: the summed rows of a data-parallel step lie in a rank layout, and the counts would have to be global")
            cw0, cw1 = self._cowclip_descs(t, Bg, cat_x, b.leader, gsum, app.clip)
        return cw0 + reduce + ema0 + ([wd0] if wd0 is not None else []) + dec1 + cw1 + apply + ([phase1] if phase1 is not None else []) + ema1

    def _refuse_cowclip(self, spec, train=True, local_optimizer=True, B=0):
        """what a plan with CowClip (`cowclip`, the harness's --cowclip) is not built for: refused by name, never routed elsewhere"""
        if not train:
            raise L.EngineError("cowclip is part of the fused training step's optimizer: it needs train=True")
        if self.host_embedding:
            raise L.EngineError("cowclip in the fused step needs the embedding tables on the device (place_embedding_on_cpu keeps them "
                                "on the host): CowClip.apply() on the torch route is the dense form")
        if self.tables_bf16:
            self._refuse_bf16_tables("cowclip (it reads fp32 table rows)")
        if not local_optimizer:
            raise L.EngineError("cowclip covers the one-process step: under data parallelism the counts would have to be global")
        if spec.wd and P.regularised(self.shapes, spec.no_reg)[1]:
            raise L.EngineError("cowclip with an L2 term on the embedding tables: the term's 2 wd W would be clipped with the gradient "
                                "(no_reg_param_name='_embedding' leaves the tables out)")
        if self.persist and self.level_schedule and self.cfg.fixed and B <= 256:
            raise L.EngineError("cowclip is not built into the persistent step (NASREC_PERSIST_DEFAULT=1): the default launches take it")

    def ensure_cowclip_state(self):
        """CowClip's scratch: cowclip_cnt[f], one uint32 word per row of table f (4 bytes x the rows of all tables: 135 MB at Criteo
        size), zero-filled once — the clip launch leaves it all zero after every step; cowclip_stat, two words: rows touched, rows
        clipped since construction."""
        if getattr(self, "cowclip_cnt", None) is not None:
            return
        with torch.cuda.stream(self.stream):
            self.cowclip_cnt = [torch.zeros(n, dtype=torch.int32, device=self.device) for n in self.num_embeddings]
            self.cowclip_stat = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.stream.synchronize()

    def cowclip_stats(self):
        """(rows touched, rows clipped) by the fused steps with CowClip since construction (waits for the device)"""
        if getattr(self, "cowclip_stat", None) is None:
            return 0, 0
        a = self.cowclip_stat.tolist()
        return int(a[0]) & 0xFFFFFFFF, int(a[1]) & 0xFFFFFFFF

    def _cowclip_descs(self, t, Bg, cat_x, leader, gsum, clip_desc):
        """([count], [clip]): the two NASREC_OP_COWCLIP launches of a plan with t.cowclip over the contiguous [Bg, Fs, 16] `gsum`"""
        self.ensure_cowclip_state()
        c = L.CowClipDesc()
        c.kind, c.phase, c.B, c.Fs = L.OP_COWCLIP, 0, Bg, self.Fs
        c.r, c.zeta = t.cowclip
        c.idx, c.leader, c.gsum = cat_x.data_ptr(), leader.data_ptr(), gsum
        for f in range(self.Fs):
            c.table[f], c.cnt[f], c.rows[f] = self.tables[f].data_ptr(), self.cowclip_cnt[f].data_ptr(), self.num_embeddings[f]
        c.clip = clip_desc
        c.stat = self.cowclip_stat.data_ptr()
        c1 = L.CowClipDesc.from_buffer_copy(c)
        c1.phase = 1
        return [c], [c1]

    DECAY_DENSE_BLOCKS = 1024  # workgroups on the dense ranges (EMA_DENSE_BLOCKS: the same stream)
    DECAY_REBASE = 1.0         # -level at which a step flushes first: a stamp's quantisation (|L| 2^-24) stays below one rounding of a weight
    _decay_dirty = False       # a fused step with decoupled weight decay ran since the last flush: table rows may owe
    _decay_mask = 0
    _decay_owed = 0.0          # host mirror of -level (an upper bound: a step that skips the stem moves no level)

    def ensure_decay_state(self):
        """The lazily paid decoupled weight decay's state (csrc/decoupled_decay.hip): `decay_level`, one fp64 word per table = the sum
        of log1p(-lr lambda) over the steps in which that table decayed; `decay_stamps[f]`, one float per row = the fp32 value of the
        level at which that row's weights are current; and the last-arrival counter.  All zero: every row current."""
        if self.host_embedding:
            raise L.EngineError("the fused decoupled weight decay needs the embedding tables on the device")
        self._refuse_bf16_tables("the fused decoupled weight decay")
        if getattr(self, "decay_level", None) is not None:
            return
        with torch.cuda.stream(self.stream):
            self.decay_stamps = [torch.zeros(n, dtype=torch.float32, device=self.device) for n in self.num_embeddings]
            self.decay_level = torch.zeros(max(1, self.Fs), dtype=torch.float64, device=self.device)
            self._decay_counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._row_bitmap()
        self.stream.synchronize()

    def _decay_tables(self, t, ctx, arena, pre):
        """Chunk table of a plan with decoupled weight decay: the selected dense ranges (P.regularised: get_l2_loss's rule) that the
        backward reaches — torch's `p.grad is not None`; and the selected tables"""
        self.ensure_decay_state()
        reached = set(n for n in list(ctx.grad_params) + ["_final.weight", "_final.bias"] if not n.startswith("_embedding."))
        reg, t.dwd_tables = P.regularised(self.shapes, t.spec.no_reg)
        flat = P.path_chunks([(self.offsets[n], self.params[n].numel()) for n in reg if n in reached], chunk=1024)
        t.dwd_tab = self._const_table(flat, arena, pre)
        t.dwd_chunks = (t.dwd_tab.data_ptr(), len(flat) // 2)

    def _decay_desc(self, phase: int, mask: int, lam: float = 0.0):
        d = L.DecoupledDecayDesc()
        d.kind, d.phase, d.Fs, d.mask, d.lambda_ = L.OP_DECOUPLED_DECAY, phase, self.Fs, mask, lam
        d.nblocks = self.WD_BLOCKS
        self._tile_layout(d, lambda f: phase == 2 and bool((mask >> f) & 1))
        for f in range(self.Fs):
            d.stamp[f] = self.decay_stamps[f].data_ptr()
        d.bitmap = self._row_bitmap().data_ptr()
        d.p = self.flat_p.data_ptr()
        d.level, d.lr, d.counter = self.decay_level.data_ptr(), self.lr_dev.data_ptr(), self._decay_counter.data_ptr()
        return d

    def _decay_step_descs(self, t, Bg, rows, cat_x, leader):
        """[decay] of a training plan with spec.dwd: phase 1 over the plan's dense ranges and the batch's leaders; leaves the
        catch-up (phase 0, whose ids the step patches in: it runs in front of the staging launch) in t.decay0 and the decay in
        t.decay1.  rows False: no gradient reaches the stem, no table decays (torch: `p.grad is None`) — the forward still gathers the
        batch's rows, so the catch-up runs all the same."""
        tables = sum(1 << f for f in t.dwd_tables)
        mask = tables if rows else 0
        d0, d1 = self._decay_desc(0, tables, t.spec.dwd), self._decay_desc(1, mask, t.spec.dwd)
        d0.B, d0.idx = Bg, cat_x.data_ptr()
        if mask:
            d1.B, d1.idx, d1.leader = Bg, cat_x.data_ptr(), leader.data_ptr()
        d1.chunks, d1.n_chunks = t.dwd_chunks
        d1.dense_blocks = max(1, min(self.DECAY_DENSE_BLOCKS, d1.n_chunks))
        t.decay0, t.decay1, t.decay_mask = (d0 if tables else None), d1, mask
        return [d1]

    @_on_device
    def flush_decay_rows(self):
        """bring every table row current (a row outside the batches owes the factors of the steps it rested through) and re-base the
        stamps and levels to 0: what a reader of the table weights needs.  One streaming launch, waited for; a no-op when no fused
        step with decoupled weight decay ran since the last flush."""
        if not self._decay_dirty:
            return
        torch.cuda.current_stream(self.device).synchronize()
        d = self._decay_desc(2, self._decay_mask)
        L.check(L.load().nasrec_decoupled_decay(self.stream.cuda_stream, C.addressof(d)))
        self.stream.synchronize()  # (the reader may sit on another stream)
        self._decay_dirty, self._decay_mask, self._decay_owed = False, 0, 0.0

    def _decay_begin(self, cp, lr: float):
        """host bookkeeping of a fused step with decoupled weight decay, before anything is launched"""
        t = cp.tail
        lam = t.spec.dwd
        if not float(lr) * lam < 1.0 or lr < 0:
            raise L.EngineError("decoupled weight decay: lr %r x lambda %r is not inside [0, 1)" % (lr, lam))
        t.decay1.lr_max = float(lr)
        if not t.decay_mask:
            return
        owes = -math.log1p(-float(lr) * lam)
        if self._decay_dirty and (t.decay_mask != self._decay_mask or self._decay_owed + owes > self.DECAY_REBASE):
            self.flush_decay_rows()
        self._decay_dirty, self._decay_mask = True, t.decay_mask
        self._decay_owed += owes

    EMA_DENSE_BLOCKS = 1024  # workgroups on the dense arena (the apply launch's measured optimum for the same stream of 2.2 M floats)

    def ensure_ema_state(self, decay: float):
        """The weight average of utils/optim.WeightEMA in the engine: `ema_flat` (the layout of flat_p) and `ema_tables[f]`, both
        initialised from the current parameters; `ema_stamps[f]`, one int32 per row = the update number at which that row's average
        is current; `ema_count` = updates applied (csrc/weight_ema.hip).  One decay per engine."""
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise L.EngineError("weight EMA: decay %r is not inside (0, 1)" % (decay,))
        if self.host_embedding:
            raise L.EngineError("the fused weight EMA needs the embedding tables on the device")
        self._refuse_bf16_tables("the fused weight EMA (its fp32 shadow tables)")
        have = getattr(self, "ema_decay", None)
        if have is not None:
            if have != decay:
                raise L.EngineError("weight EMA: this engine averages with decay %r, not %r" % (have, decay))
            return
        with torch.cuda.stream(self.stream):
            self.ema_flat = self.flat_p.detach().clone()
            self.ema_tables = [t.detach().clone() for t in self.tables]
            self.ema_stamps = [torch.zeros(n, dtype=torch.int32, device=self.device) for n in self.num_embeddings]
            self.ema_count = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._ema_counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._row_bitmap()
        self.stream.synchronize()
        self.ema_decay, self.ema_swapped = decay, False

    def ema_view(self, name: str):
        """engine storage of the average of parameter `name` (shape of the parameter)"""
        if name.startswith("_embedding."):
            return self.ema_tables[int(name.split(".")[1])]
        o, n = self.offsets[name], self.params[name].numel()
        return self.ema_flat[o:o + n].view(self.params[name].shape)

    def _ema_desc(self, phase: int):
        d = L.WeightEmaDesc()
        d.kind, d.phase, d.Fs, d.decay = L.OP_WEIGHT_EMA, phase, self.Fs, self.ema_decay
        d.dense_blocks = max(1, min(self.EMA_DENSE_BLOCKS, (self.flat_numel // 4 + 255) // 256))
        d.nblocks = self.WD_BLOCKS
        self._tile_layout(d, lambda f: phase >= 2)
        for f in range(self.Fs):
            d.shadow[f], d.stamp[f] = self.ema_tables[f].data_ptr(), self.ema_stamps[f].data_ptr()
        d.bitmap = self._row_bitmap().data_ptr()
        d.p, d.s, d.n = self.flat_p.data_ptr(), self.ema_flat.data_ptr(), self.flat_numel
        d.count, d.counter = self.ema_count.data_ptr(), self._ema_counter.data_ptr()
        return d

    def _ema_step_descs(self, spec, Bg, cat_x, leader):
        """([catch-up], [update]) of a training plan with spec.ema: phases 0 and 1 over the batch's leaders (Bg = 0: no gradient
        reaches the stem, no row moves — the update still averages the dense arena and counts, and the tables' rows owe)"""
        self.ensure_ema_state(spec.ema)
        out = []
        for phase in (0, 1):
            d = self._ema_desc(phase)
            d.B = Bg
            if Bg:
                d.idx, d.leader = cat_x.data_ptr(), leader.data_ptr()
            out.append([d])
        return out

    def _ema_launch(self, phase: int):
        d = self._ema_desc(phase)
        L.check(L.load().nasrec_weight_ema(self.stream.cuda_stream, C.addressof(d)))
        self.stream.synchronize()  # (the reader may sit on another stream)

    @_on_device
    def flush_ema_rows(self):
        """bring the average of every table row current (a row outside the batches owes decay^n since its stamp): what a reader of
        the shadow needs.  One streaming launch, waited for; a no-op without EMA state."""
        if getattr(self, "ema_decay", None) is not None:
            torch.cuda.current_stream(self.device).synchronize()
            self._ema_launch(2)

    @_on_device
    def swap_ema(self):
        """exchange the parameters with their average, every row flushed first: one launch.  Called twice it restores both, bit for
        bit; in between train_step and last_layer_step refuse (the engine would train the averaged weights)."""
        if getattr(self, "ema_decay", None) is None:
            raise L.EngineError("swap_ema: this engine keeps no weight average (ensure_ema_state)")
        torch.cuda.current_stream(self.device).synchronize()
        self._ema_launch(3)
        self.ema_swapped = not self.ema_swapped

    def _refuse_swapped(self, what):
        if getattr(self, "ema_swapped", False):
            raise L.EngineError("%s while the parameters hold their weight average (swap_ema / WeightEMA.averaged): leave it first" % what)

    @_on_device
    def reserve(self, B: int, train: bool = True, choice=None, freeze_gc: bool = False):
        """Size every plan slot for the LARGEST path at batch B (default: the warm-up choice = the full path) and allocate the
        engine-level workspaces, so that no sampled path of a run has to grow an arena (an allocator call + device
        synchronisation in the middle of a step: 1-2 ms spikes in the per-step times).  Host work only; nothing is launched.
        freeze_gc (opt-in, for a process that keeps ONE engine for its whole life — bench.py, the train_supernet CLI): move
        everything alive now into the cyclic collector's permanent generation, so that its full passes walk the few plans in flight
        instead of ~10^6 long-lived objects (17-56 ms stalls per step otherwise).  Frozen objects are never collected: a process that
        builds engine after engine (eval_subnet_from_supernet: one SuperNet per candidate) must leave it off."""
        if self.cfg.fixed:
            return 0
        cp = self.compile(choice if choice is not None else self.warm_choice, B, train)
        need = cp.arena.used_bytes() + Arena.CHUNK
        key = next(k for k, v in self._plans.items() if v is cp)
        self._plans.pop(key)
        cp.evicted = True
        self._last_plan = None
        arenas = [cp.arena] + list(self._spare_arenas)
        cp.arena = None
        # the warm plan is a web of closures over its context, which holds the parameter / gradient dicts, the arena and a bound
        # method of this engine: cut it open so that reference counting frees it now (and nothing of it is frozen below)
        wctx = getattr(cp, "ctx", None)
        if wctx is not None:
            wctx.closures, wctx.deferred, wctx.mha_reduce, wctx.keep = [], [], [], []
            wctx.sk_workspace = None
            wctx.arena = None
            wctx.params = wctx.grads = None
        cp.ctx = None
        cp = wctx = None  # (not `del`: `cp` is read by the generator expression above, and the module also builds under Cython)
        live = len(self._plans)
        while len(arenas) + live < 4:
            arenas.append(Arena(self.device))
        for a in arenas:
            a.reserve(need)
        for v in self._plans.values():
            if v.arena is not None:
                v.arena.reserve(need)
        self._spare_arenas = arenas
        self._sk_workspace()
        if freeze_gc:
            import gc
            gc.collect()
            gc.freeze()
        return need

    def _sk_workspace(self):
        """partial-tile workspace of the balanced GEMM schedule (100 MB): one per engine — the launches of a program run in
        stream order, and each one's second pass has consumed the buffer before the next launch writes it"""
        if getattr(self, "_sk_ws", None) is None:
            self._sk_ws = torch.empty(L.SK_WORKSPACE_FLOATS, dtype=torch.float32, device=self.device)
        return self._sk_ws

    # -------------------------------------------------------------------------------------------------------
    def _sp(self):
        """Launches go to the CALLER's current stream (no cross-stream event pair per step: each one costs a barrier packet
        and ~10 us of GPU idle); the private stream only builds and captures plans."""
        return torch.cuda.current_stream(self.device).cuda_stream

    @staticmethod
    def _fuse_final(fwd_list, bwd_descs, fused):
        """joint forward + backward program: the final logit's forward and the per-sample part of its backward (d loss / d features =
        (sigmoid(logit) - y) / B * w: supernet.py:592-598 under BCEWithLogitsLoss) become ONE operator (NASREC_OP_FINAL_FUSED: the
        wavefront that sums a sample's logit writes its feature gradients too), so the backward pass starts one launch boundary
        earlier; the parts that need every sample's logit (d w, d bias, the loss) stay a FINAL_BWD with dseg_done, which nothing
        waits for.  Same expressions per element: the bit-identity tests against one launch per operator cover it."""
        fi = [i for i, d in enumerate(fwd_list) if isinstance(d, L.FinalDesc) and d.kind == L.OP_FINAL_FWD]
        if len(fi) != 1 or fused.nsplit > 1 or not any(d is fused for d in bwd_descs):
            return fwd_list, bwd_descs
        f = fwd_list[fi[0]]
        same = f.B == fused.B and f.nseg == fused.nseg and f.w == fused.w and f.logits == fused.logits and all(
            f.seg[q] == fused.seg[q] and f.width[q] == fused.width[q] and f.ld[q] == fused.ld[q] and f.off[q] == fused.off[q]
            and f.tok_stride[q] == fused.tok_stride[q] and (not fused.dseg[q] or f.seg[q]) for q in range(f.nseg))
        if not same:
            return fwd_list, bwd_descs
        both = L.FinalDesc.from_buffer_copy(fused)
        both.kind, both.bias = L.OP_FINAL_FUSED, f.bias
        rest = L.FinalDesc.from_buffer_copy(fused)
        rest.dseg_done = 1
        return ([both if i == fi[0] else d for i, d in enumerate(fwd_list)], [rest if d is fused else d for d in bwd_descs])

    @staticmethod
    def _fuse_head(fwd_list, bwd_descs):
        """joint program, behind _fuse_final: the last dense Linear y = pre_add + x W^T + b whose only forward reader is the final logit
        (<= 32 inputs, <= 256 outputs: 2 K multiply-adds per sample in ea_criteo_kaggle_xlarge_best_1shot.json, alone in its level) and
        its input gradient dx (+)= dy W (alone in the level behind the logit) become part of NASREC_OP_FINAL_FUSED: the workgroup that
        sums a sample's logit computes the sample's row of both (csrc/final_bodies.h, same MFMA, same k order, same epilogue order:
        the bit-identity tests against one launch per operator cover it).  Two levels less.  Everything else — an activation, mask,
        LayerNorm or gating operand on the Linear, several K-segments, another forward reader of y, token-strided segments
        (last_n_blocks_out > 1), an operator in between that the move would overtake — keeps today's descriptors; a Linear whose dx
        product does not fit the pattern still gives its forward half."""
        fi = [i for i, d in enumerate(fwd_list) if isinstance(d, L.FinalDesc) and d.kind == L.OP_FINAL_FUSED]
        if len(fi) != 1:
            return fwd_list, bwd_descs
        fi = fi[0]
        both = fwd_list[fi]
        if both.head_x or any(both.tok_stride[q] for q in range(both.nseg)):
            return fwd_list, bwd_descs
        fn = [S.Node(d) for d in fwd_list]
        if any(n.reads is None for n in fn):
            return fwd_list, bwd_descs

        def bare(d, zmode):
            return (isinstance(d, L.GemmDesc) and d.nseg == 1 and d.zmode == zmode and d.splitk <= 1 and not d.defer_second_pass and d.act == L.ACT_NONE
                    and d.dims_in_use < 0 and not d.save_z and not d.save_act and d.mul_nseg == 0 and d.precision == 0 and d.cmode == L.CM_PLAIN
                    and d.amode == L.AM_KC and d.seg[0].A and not d.seg[0].Aaux and not d.seg[0].Baux and not d.seg[0].ones_col
                    and not 0 < d.seg[0].Mvalid < d.seg[0].M)
        for hi in range(fi - 1, -1, -1):
            h = fwd_list[hi]
            if not (bare(h, 0) and h.bmode == L.AM_KC and h.beta == 0):
                continue
            s = h.seg[0]
            hq = [q for q in range(both.nseg) if both.seg[q] == s.C and both.width[q] == s.N and both.ld[q] == s.ldc]
            if len(hq) != 1 or s.M != both.B or not (1 <= s.K <= L.FINAL_HEAD_K and 1 <= s.N <= L.FINAL_HEAD_N) or s.ldb > (1 << 20):
                continue
            hq = hq[0]
            y = S.Acc(s.C, s.M, s.N, s.ldc)
            others = [n for i, n in enumerate(fn) if i not in (hi, fi)]
            if any(S.overlap(a, y) for n in others for a in n.reads + n.writes):
                continue  # another forward reader (or writer) of y
            if any(S._depends(fn[i], fn[hi]) for i in range(hi + 1, fi)):
                continue  # the Linear cannot move behind an operator that overwrites one of its operands
            new = L.FinalDesc.from_buffer_copy(both)
            new.head_x, new.head_w, new.head_bias, new.head_pre, new.head_y = s.A, s.B, h.bias, h.pre_add, s.C
            new.head_K, new.head_N, new.head_ldx, new.head_ldw, new.head_ldy, new.head_seg = s.K, s.N, s.lda, s.ldb, s.ldc, hq
            jf = [new if i == fi else d for i, d in enumerate(fwd_list) if i != hi]
            jb = list(bwd_descs)
            # the input gradient: one problem dx = dy W on the same W, reading what this operator writes as dseg[hq]
            for xi, x in enumerate(bwd_descs):
                if not (bare(x, 1) and x.bmode == L.AM_RC and not x.bias and not x.pre_add and both.dseg[hq]):
                    continue
                t = x.seg[0]
                if not (t.A == both.dseg[hq] and t.lda == both.ld[hq] and t.B == s.B and t.ldb == s.ldb and (t.M, t.N, t.K) == (s.M, s.K, s.N) and t.C):
                    continue
                xn = S.Node(x)
                before = [S.Node(d) for d in fwd_list[fi + 1:] + bwd_descs[:xi]]  # what the product overtakes when it moves into the logit's operator
                if any(n.reads is None or S._depends(xn, n) for n in before):
                    break
                new.head_dx, new.head_lddx, new.head_dx_accumulate = t.C, t.ldc, int(t.accumulate != 0)
                jb = [d for i, d in enumerate(bwd_descs) if i != xi]
                break
            return jf, jb
        return fwd_list, bwd_descs

    def _stage_inputs(self, sp, cp, int_x, cat_x, y=None, lr=None, rows=None, launch=True, catch_up=False):
        """one launch: batch -> the plan's static buffers (+ this step's learning rate -> device scalar); host_embedding: the
        looked-up rows [B, Fs, 16] come with the batch.  launch=False: only patch the prebuilt staging descriptor (the caller launches it
        as the head of a program) — returns True when that is what happened, False when the inputs went another way and are staged.
        catch_up (train_step): a plan with decoupled weight decay launches its phase 0 over this batch's ids in front of the gather
        (launch=False: the caller's program carries it in front of the staging descriptor)"""
        dec0 = getattr(cp, "decay0", None) if catch_up else None  # (decoupled weight decay: the batch's rows pay before the gather)
        if self.host_embedding:
            if rows is None:
                raise L.EngineError("this engine holds no embedding table (place_embedding_on_cpu): pass the looked-up rows")
            cp.sparse0.t.copy_(rows.reshape(-1).to(torch.float32), non_blocking=True)
        ok = (int_x.is_cuda and cat_x.is_cuda and int_x.dtype == torch.float32 and cat_x.dtype == torch.int64
              and int_x.is_contiguous() and cat_x.is_contiguous()
              and (y is None or (y.is_cuda and y.dtype == torch.float32 and y.is_contiguous())))
        if not ok:  # host tensors / other dtypes: let torch convert and copy
            cp.int_x.copy_(int_x.reshape(cp.int_x.shape), non_blocking=True)
            cp.cat_x.copy_(cat_x.reshape(cp.cat_x.shape), non_blocking=True)
            if y is not None:
                cp.y.copy_(y.reshape(cp.y.shape), non_blocking=True)
            if lr is not None:
                self.lr_dev.fill_(float(lr))
            if dec0 is not None:
                dec0.idx = cp.cat_x.data_ptr()
                L.check(L.load().nasrec_launch(sp, C.addressof(dec0)))
            if not self.host_embedding:
                L.check(L.load().nasrec_launch(sp, C.addressof(cp.gather)))
            if getattr(cp, "ids_on_stage", False):  # (the staging launch would have carried it)
                L.check(L.load().nasrec_launch(sp, C.addressof(cp.tail.dedup_ids)))
            return False
        d = cp.stage  # prebuilt per plan: only the sources change from step to step
        d.int_src, d.cat_src = int_x.data_ptr(), cat_x.data_ptr()
        d.y_src = y.data_ptr() if y is not None else None
        if dec0 is not None:
            dec0.idx = cat_x.data_ptr()  # (the raw ids: the staging launch has not copied them yet)
        if lr is not None:
            d.lr, d.lr_dst = float(lr), self.lr_dev.data_ptr()
        else:
            d.lr_dst = None
        if not launch:
            return True
        if dec0 is not None:
            L.check(L.load().nasrec_launch(sp, C.addressof(dec0)))
        L.check(L.load().nasrec_launch(sp, C.addressof(d)))
        return False

    @_on_device
    def forward(self, int_x, cat_x, choice=None, graph=False, rows=None):
        """logits [B,1] for the given choice (fixed mode: the fixed choice)."""
        choice = choice if choice is not None else self.warm_choice
        if self._decay_dirty:  # (fused steps with decoupled weight decay left table rows owing)
            self.flush_decay_rows()
        B = int(int_x.shape[0])
        cp = self.compile(choice, B, train=False, graph=graph)
        sp = self._sp()
        self._stage_inputs(sp, cp, int_x, cat_x, rows=rows)
        if graph:
            cp.fwd.replay(sp)
        else:
            cp.fwd.run(sp)
        return cp.logits.view(B, 1)

    def prefers_graph(self, B: int) -> bool:
        """graph = None: replay the captured step, or launch its program?  A level-scheduled step (fixed sub-network, batch <= 256) is
        ~27 launches issued by ONE host call (nasrec_program_run: ~3 us each, the host stays far ahead of a 0.25 ms step), and every
        graph launch ends on a ~8.5 us bubble before the next command starts (rocprofv3 kernel trace, tools/launch_gaps.py: graph's last
        kernel -> next launch 8.4 - 8.7 us, 0.0 between eagerly launched kernels): 0.2575 ms replayed, 0.2515 ms launched.  Plans
        of 60+ launches (no level schedule; larger batches) keep the graph: there the host call is what bounds the step.  (A host that
        has more to do between steps — the training harness with its data pipe — is better off replaying: SuperNet.engine_train_step.)"""
        return not (self.level_schedule and self.cfg.fixed and B <= 256) or os.environ.get("NASREC_STEP_GRAPH", "auto") == "1"

    @_on_device
    def train_step(self, int_x, cat_x, y, lr: float, choice=None, clip: Optional[float] = 5.0, eps: float = 1e-2, graph: Optional[bool] = False,
                   staged: bool = False, weight_decay: float = 0.0, no_reg_param_name: Optional[str] = None, optim=None, ema: float = 0.0,
                   decoupled_wd: float = 0.0, cowclip=None):
        """zero_grad -> forward -> BCE -> backward -> clip_grad_norm_ -> Adagrad (train_utils.py:262-286).
        Returns the (device) loss tensor of this step.  `staged`: inputs are already in the plan's static buffers.  graph: True = replay
        the captured step, False = launch its program, None = whichever is faster for this plan (prefers_graph).
        weight_decay != 0: the step minimises BCE + get_l2_loss(model, weight_decay, no_reg_param_name) (train_utils.py:91-115,262-266):
        every regularised parameter and EVERY table row is decayed; wd_l2_sumsq then holds sum ||W||^2 of the pre-step weights.
        optim: an OptimSpec of kind adam / sgd replaces Adagrad (eps is then unused): torch.optim.Adam / SGD over the parameters the step
        reaches and EVERY table row, state in `moments` and `opt_steps` (ensure_moments_state); with sparse_rows the tables move in the
        batch's rows only (utils/optim.RowSparseAdam), and weight decay must leave them out.
        ema: the decay of a weight average kept beside the step (ensure_ema_state; csrc/weight_ema.hip): two more launches in the
        optimizer tail, exact only where the tables move in the batch's rows alone (OptimSpec.rows_only: Adagrad, row-sparse Adam,
        RMSprop, Adam with Adagrad on the tables; no regularised table) — refused otherwise.
        decoupled_wd: lambda of the decoupled weight decay p <- p (1 - lr lambda) in front of the update (utils/optim.
        DecoupledWeightDecay; csrc/decoupled_decay.hip) over the parameters get_l2_loss's rule selects (no_reg_param_name) and the
        step reaches: two more launches, the table rows outside the batch rest and owe — a raw read of a table needs
        flush_decay_rows() first.  Refused where the tables move outside the batch's rows, and, when it reaches the tables, beside a
        weight average or an L2 term on them.
        cowclip: (r, zeta) = CowClip (utils/optim.CowClip; csrc/cowclip.hip) on the batch's summed table rows, behind the global clip
        and in front of every optimizer statement: two more launches, whatever rule the tables take.  Refused on bf16 tables, beside
        an L2 term on the tables and in the persistent form; cowclip_stats() counts the rows it touched and clipped."""
        self._refuse_swapped("train_step")
        if decoupled_wd:
            if optim is not None and not optim.rows_only:
                raise L.EngineError("the fused decoupled weight decay lets the table rows outside the batch rest: dense Adam and "
                                    "momentum SGD move every row (DecoupledWeightDecay.apply() on the torch route is the dense form)")
            if P.regularised(self.shapes, no_reg_param_name)[1] and (ema or weight_decay):
                raise L.EngineError("a decoupled weight decay that reaches the embedding tables runs beside neither a fused weight "
                                    "EMA nor an L2 term on the tables (DecoupledWeightDecay.apply() on the torch route is the dense form)")
        if ema and ((optim is not None and not optim.rows_only)
                    or (weight_decay and P.regularised(self.shapes, no_reg_param_name)[1])):
            raise L.EngineError("the fused weight EMA averages the batch's table rows only: dense Adam, momentum SGD and a regularised "
                                "table move every row (WeightEMA.update() on the torch route is the dense form)")
        choice = choice if choice is not None else self.warm_choice
        if graph is None:
            graph = self.cfg.fixed and self.prefers_graph(int(int_x.shape[0]) if int_x is not None else int(self._last_plan[2].cat_x.shape[0]))
        if self.host_embedding:
            raise L.EngineError("the fused training step needs the embedding tables on the device (place_embedding_on_cpu keeps them "
                                "on the host): use the nn.Module path (forward / backward / torch optimizer)")
        if int_x is not None:
            B = int(int_x.shape[0])
        else:  # pre-staged inputs: the batch size is the one of the plan they were staged into
            assert staged and self._last_plan is not None, "train_step without inputs needs a previously compiled plan holding them"
            B = int(self._last_plan[2].cat_x.shape[0])
        cp = self.compile(choice, B, train=True, clip=clip, eps=eps, graph=graph, spec=OptimSpec.of(eps, weight_decay, no_reg_param_name, optim, ema, decoupled_wd),
                          cowclip=cowclip)
        sp = self._sp()
        dec0 = None
        if cp.tail.spec.dwd:
            self._decay_begin(cp, lr)
            dec0 = cp.decay0
        elif self._decay_dirty:  # (a step without the decay behind steps with it: its gather reads current rows)
            self.flush_decay_rows()
        if not staged:
            whole = not graph and getattr(cp, "fb", None) is not None and not self.host_embedding
            if self._stage_inputs(sp, cp, int_x, cat_x, y, lr, launch=not whole, catch_up=True):
                # a launched (not replayed) step: staging launch + joint program + optimizer as ONE host call
                if getattr(cp, "whole", None) is None:
                    cp.whole = Program(([dec0] if dec0 is not None else []) + [cp.stage] + list(cp.fb.descs) + list(cp.opt.descs))
                cp.whole.run(sp)
                return cp.loss
        else:
            self.lr_dev.fill_(float(lr))
            if dec0 is not None:
                dec0.idx = cp.cat_x.data_ptr()
                L.check(L.load().nasrec_launch(sp, C.addressof(dec0)))
            L.check(L.load().nasrec_launch(sp, C.addressof(cp.gather)))
            if getattr(cp, "ids_on_stage", False):
                L.check(L.load().nasrec_launch(sp, C.addressof(cp.tail.dedup_ids)))
        if graph:
            cp.step.replay(sp)
        else:
            if getattr(cp, "fb", None) is not None:
                cp.fb.run(sp)
            else:
                cp.fwd.run(sp)
                cp.bwd.run(sp)
            cp.opt.run(sp)
        return cp.loss

    def ensure_last_layer_state(self, kind: str):
        """Adam's exp_avg / exp_avg_sq or SGD's momentum_buffer of _final.{weight, bias} for the last-layer step (last_layer_step),
        allocated on first use, zero, and its two step counters ll_steps [weight, bias].  -> {state key: (weight array, bias array)}.
        (The whole-model moments of ensure_moments_state would hold two more copies of every table.)"""
        keys = ("exp_avg", "exp_avg_sq") if kind == "adam" else ("momentum_buffer",)
        st = self.__dict__.setdefault("ll_moments", {})
        with torch.cuda.stream(self.stream):
            for k in keys:
                if k not in st:
                    st[k] = (torch.zeros_like(self.params["_final.weight"]), torch.zeros_like(self.params["_final.bias"]))
            if getattr(self, "ll_steps", None) is None:
                self.ll_steps = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.stream.synchronize()
        return {k: st[k] for k in keys}

    def _last_layer_program(self, cp, clip, spec, graph):
        """(staging launch + forward + final-logit backward with BCE folded in, d features skipped + NASREC_OP_LAST_LAYER_STEP,
        the same without the staging launch) of a compiled training plan, built once per plan and optimizer (spec)"""
        key = (clip, spec, graph)
        progs = cp.__dict__.setdefault("last_layer", {})
        if key in progs:
            return progs[key]
        last = next(d for d in cp.bwd_final_only.descs if isinstance(d, L.FinalDesc))
        fin = L.FinalDesc.from_buffer_copy(last)
        fin.logits, fin.y, fin.loss, fin.dlogits_out = cp.logits.data_ptr(), cp.y.data_ptr(), cp.loss.data_ptr(), None
        fin.grad_scale = cp.bce.grad_scale
        K = int(self.params["_final.weight"].numel())
        if K + 1 > L.LAST_LAYER_MAX:
            raise L.EngineError("last-layer step: the final layer has %d inputs, the kernel takes at most %d" % (K, L.LAST_LAYER_MAX - 1))
        d = L.LastLayerStepDesc()
        d.kind, d.K, d.nsplit = L.OP_LAST_LAYER_STEP, K, max(1, int(fin.nsplit))
        d.partial = fin.dw if fin.nsplit > 1 else None
        d.dw, d.dbias = self.grads["_final.weight"].data_ptr(), self.grads["_final.bias"].data_ptr()
        d.w, d.bias = self.params["_final.weight"].data_ptr(), self.params["_final.bias"].data_ptr()
        d.max_norm = float(clip) if clip is not None else 0.0
        d.wd = spec.wd
        d.decay_w = int(bool(spec.wd) and not (spec.no_reg is not None and "_final.weight".startswith(spec.no_reg)))
        if not spec.moments:
            d.algo, d.eps = L.OPTIM_ADAGRAD, spec.eps
            d.s_w, d.s_b = self.state["_final.weight"].data_ptr(), self.state["_final.bias"].data_ptr()
        else:
            st = self.ensure_last_layer_state(spec.kind)
            self._optim_scalars(d, spec)
            first = st["exp_avg"] if spec.kind == "adam" else st["momentum_buffer"]
            d.s_w, d.s_b = first[0].data_ptr(), first[1].data_ptr()
            if spec.kind == "adam":
                d.v_w, d.v_b = st["exp_avg_sq"][0].data_ptr(), st["exp_avg_sq"][1].data_ptr()
            d.step = self.ll_steps.data_ptr()
        d.lr, d.norm_out = self.lr_dev.data_ptr(), self.clip_out.data_ptr()
        cp.ll_keep = getattr(cp, "ll_keep", []) + [fin, d]  # (descriptors are passed by address: they live as long as the plan)
        rest = Program(list(cp.fwd.descs) + [fin, d])
        whole = None
        if graph:
            rest.capture(self.stream.cuda_stream)
            self.stream.synchronize()
        else:
            whole = Program([cp.stage] + list(cp.fwd.descs) + [fin, d])
        progs[key] = (whole, rest)
        return progs[key]

    @_on_device
    def last_layer_step(self, int_x, cat_x, y, lr: float, choice=None, clip: Optional[float] = 5.0, eps: float = 1e-2,
                        weight_decay: float = 0.0, no_reg_param_name: Optional[str] = None, optim=None, graph: bool = False):
        """The training step of last-layer fine-tuning (SuperNet.set_mode_to_finelune_last_only): forward -> BCE -> d loss / d _final
        (nothing else) -> [+ 2 wd W] -> clip_grad_norm_ over _final -> Adagrad (state: self.state) / Adam / SGD (optim, state:
        ensure_last_layer_state) on _final.{weight, bias} alone.  Returns the (device) loss.  graph: replay a captured program (fixed
        sub-networks).  The plan is the one the autograd route runs (compile(choice, B, train=True))."""
        self._refuse_swapped("last_layer_step")
        if self._decay_dirty:
            self.flush_decay_rows()
        choice = choice if choice is not None else self.warm_choice
        if self.host_embedding:
            raise L.EngineError("the last-layer step needs the embedding tables on the device")
        self._refuse_bf16_tables("the last-layer step (its plan is the Adagrad training plan)")
        if optim is not None and optim.kind == "rmsprop":
            raise L.EngineError("the last-layer step has no RMSprop: the fine-tune keeps the torch route with it")
        if optim is not None and optim.adagrad_tables:
            raise L.EngineError("the last-layer step has no split optimizer: the fine-tune keeps the torch route with it")
        B = int(int_x.shape[0])
        cp = self.compile(choice, B, train=True)
        self.last_layer_plan = cp  # (its logits: SuperNet.engine_last_logits)
        whole, rest = self._last_layer_program(cp, clip, OptimSpec.of(eps, weight_decay, no_reg_param_name, optim), bool(graph))
        sp = self._sp()
        if self._stage_inputs(sp, cp, int_x, cat_x, y, lr, launch=whole is None):
            whole.run(sp)
            return cp.loss
        if graph:
            rest.replay(sp)
        else:
            rest.run(sp)
        return cp.loss

    def close(self):
        """Release what this engine holds outside torch's allocator now, not at the next garbage collection: captured graphs and the
        uncached arenas of its plans (hipExtMallocWithFlags memory, freed when the last view of it goes).  The engine is unusable after."""
        if self._decay_dirty:  # (the tables outlive the engine: their rows are left current)
            self.flush_decay_rows()
        self.stream.synchronize()
        for cp in list(self._plans.values()):
            for prog in [getattr(cp, n, None) for n in ("step", "fwd", "whole")] + [p for pr in getattr(cp, "last_layer", {}).values() for p in pr]:
                if prog is not None and prog.graph is not None:
                    L.load().nasrec_graph_destroy(prog.graph)
                    prog.graph = None
            ctx = getattr(cp, "ctx", None)
            if ctx is not None:
                ctx.closures, ctx.deferred, ctx.mha_reduce, ctx.keep = [], [], [], []
                ctx.sk_workspace = None
                ctx.arena = None
            cp.ctx = None
            cp.arena = None
            cp.__dict__.clear()
        self._plans.clear()
        self._pcache.clear()
        self._spare_arenas = []
        self._last_plan = None
        self.last_layer_plan = None
        self._uc_flat_arena = None
        self._sk_ws = None
        self.ema_flat = self.ema_tables = self.ema_stamps = self.ema_count = self._ema_counter = self.ema_decay = None
        self.decay_stamps = self.decay_level = self._decay_counter = None

    @_on_device
    def run_forward(self, cp, int_x, cat_x, rows=None):
        """forward program of an already compiled (training) plan; logits land in cp.logits"""
        if self._decay_dirty:
            self.flush_decay_rows()
        sp = self._sp()
        self._stage_inputs(sp, cp, int_x, cat_x, rows=rows)
        cp.fwd.run(sp)

    @_on_device
    def run_backward(self, cp, dlogits, final_only: bool = False):
        """backward program with an externally supplied d(loss)/d(logits) [B,1] (torch.autograd entry)"""
        cp.dlogits.copy_(dlogits.reshape(-1), non_blocking=True)
        (cp.bwd_final_only if final_only else cp.bwd_core).run(self._sp())

    @_on_device
    def forward_backward(self, int_x, cat_x, y, choice=None, grad_scale=None):
        """forward + BCE + backward only (gradients left in self.grads / plan.sparse0 gradient); used by the data-parallel
        wrapper and by the parity tests."""
        choice = choice if choice is not None else self.warm_choice
        if self._decay_dirty:
            self.flush_decay_rows()
        B = int(int_x.shape[0])
        cp = self.compile(choice, B, train=True, grad_scale=grad_scale)
        sp = self._sp()
        self._stage_inputs(sp, cp, int_x, cat_x, y)
        if getattr(cp, "fb", None) is not None:
            cp.fb.run(sp)
        else:
            cp.fwd.run(sp)
            cp.bwd.run(sp)
        return cp

    def check_indices(self):
        """raise IndexError if any embedding id seen so far was out of range (torch raises at lookup time)"""
        torch.cuda.synchronize(self.device)
        for t in self._persist_errs:
            e = t.view(torch.int32)[:3].tolist()
            if e[0] != 0:
                raise RuntimeError("persistent step: a workgroup of item %d waited more than 10 ms for item %d (results of that step are invalid)" % (e[1], e[2]))
        flags = self.oob.tolist()
        if flags[0] != 0:
            raise IndexError("index out of range in embedding lookup")
        if flags[1] != 0:
            raise RuntimeError("embedding-gradient merge: a hash partition overflowed (more than 16384 distinct ids hashed into one "
                               "partition of 4096 expected); the optimizer step that raised the flag must be discarded")


def _jsonable(o):
    if hasattr(o, "tolist"):
        return o.tolist()
    if hasattr(o, "item"):
        return o.item()
    raise TypeError(type(o))
