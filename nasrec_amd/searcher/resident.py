"""Resident search workers (`--resident_candidates 1`): one weight-sharing supernet per GPU, set up once, scores every candidate.

`finetune_and_eval_one_model` (the reference's way, eval_subnet_from_supernet.py:71-207) builds a supernet, warms it up on the full
path and loads the checkpoint for EVERY candidate, then re-reads the same first batches through the data pipe.  In last-layer mode
(`--finetune_whole_supernet 0`, the default) two candidates differ only in the pinned path, `_final.{weight, bias}` and the optimizer
state; with `--finetune_whole_supernet 1` every weight moves.  `ResidentCandidateEvaluator` keeps the set-up and restores only what
a candidate may change (a snapshot, device to device), keeps the first batches on the device, and trains the last layer through the
engine's fused step (SuperNet.engine_last_layer_step).  Each candidate gets a fresh torch optimizer and LR schedule, exactly as
`finetune_and_eval_one_model` builds them, and the path bookkeeping of a freshly built supernet, so a random candidate is drawn
from the global np.random stream with the same calls in the same order.
"""
import copy
import gc
from typing import Optional

import numpy as np
import torch

from ..utils.data_pipes import make_loaders
from ..utils.io_utils import load_model_checkpoint
from ..utils.train_utils import train_and_test_one_epoch, warmup_supernet_model
from .searcher_utils import build_supernet

# the choice bookkeeping a forward pass of a SuperNet / of its blocks writes (supernet.py: _resolve_choice, _get_choice)
_NET_KEYS = ("macro_last_choice", "_fixed_path_called", "_supernet_train_steps_counter", "choice", "_fixed_resolved")
_BLOCK_KEYS = ("micro_last_choice", "_fixed_path_called", "_supernet_train_steps_counter", "choice")


def _book(obj, keys):
    """{key: deep copy of obj's attribute} of the keys obj has (an absent key stays absent when restored)"""
    return {k: copy.deepcopy(obj.__dict__[k]) for k in keys if k in obj.__dict__}


class ResidentCandidateEvaluator:
    """One supernet on one GPU for a whole search.  evaluate(choice) -> the dict finetune_and_eval_one_model returns.

    fused_last_layer: train the last layer with engine_last_layer_step (False: the torch route, as finetune_and_eval_one_model).
    Batches: with bounded max_train_steps / max_eval_steps, the first ones are kept on the device when they take at most
    RESIDENT_BATCH_BYTES; otherwise every candidate streams them from make_loaders, as before."""

    RESIDENT_BATCH_BYTES = 2 << 30

    def __init__(self, args, checkpoint=None, gpu: Optional[int] = None, fused_last_layer: bool = True, resident_batches: bool = True):
        args = copy.copy(args)
        if gpu is not None:
            args.gpu = gpu
        if args.loss_function != "bce":
            raise NotImplementedError("Loss function {} is not implemented!".format(args.loss_function))
        if checkpoint is None:
            if getattr(args, "ckpt_path", None) is None:
                raise ValueError("a resident candidate evaluator needs the supernet checkpoint (a dict or --ckpt_path)")
            checkpoint = load_model_checkpoint(args.ckpt_path)
        self.args, self.fused_last_layer = args, bool(fused_last_layer)
        self.last_only = args.finetune_whole_supernet == 0
        model = build_supernet(args, getattr(args, "num_embeddings", None))
        train_loader, test_loader = make_loaders(args)
        model = model.to(args.gpu)
        with torch.no_grad():
            model = warmup_supernet_model(model, train_loader, args.gpu)
        model.load_state_dict(checkpoint["model_state_dict"], strict=True)
        self.model = model
        # the path bookkeeping of a supernet that has just been warmed up (what every fresh candidate starts from)
        self._net_book = _book(model, _NET_KEYS)
        self._block_book = [_book(b, _BLOCK_KEYS) for b in model._blocks]
        # what a candidate may change, kept on the device: _final (last-layer mode) or every parameter (the dense arena + the tables)
        names = ("_final.weight", "_final.bias") if self.last_only else None
        with torch.no_grad():
            self._snapshot = {n: p.detach().clone() for n, p in model.named_parameters() if names is None or n in names}
        torch.cuda.synchronize(args.gpu)
        self.train_loader = self.test_loader = None  # (streamed batches: every candidate gets loaders of its own, as before)
        self.resident = False
        if resident_batches and args.max_train_steps > 0 and args.max_eval_steps > 0:
            self._keep_batches(train_loader, test_loader)
        del train_loader, test_loader
        self.loss_fn = torch.nn.BCEWithLogitsLoss()

    def _keep_batches(self, train_loader, test_loader):
        a = self.args

        def first(loader, n):
            out, nbytes = [], 0
            it = iter(loader)
            try:
                for b in it:
                    b = tuple(t.to(a.gpu).clone() for t in b)  # (clone: a device-staging loader reuses its buffers)
                    nbytes += sum(t.numel() * t.element_size() for t in b)
                    if nbytes > self.RESIDENT_BATCH_BYTES:
                        return None
                    out.append(b)
                    if len(out) >= n:
                        break
            finally:
                close = getattr(it, "close", None)  # (a generator's reader threads and staging blocks end here, not at collection)
                if close is not None:
                    close()
            return out
        tr = first(train_loader, a.max_train_steps)
        te = first(test_loader, a.max_eval_steps) if tr is not None else None
        if tr is None or te is None:
            print("Resident batches exceed {} bytes: streaming them per candidate.".format(self.RESIDENT_BATCH_BYTES))
            return
        self.train_loader, self.test_loader, self.resident = tr, te, True

    def _loaders(self):
        if self.resident:
            return self.train_loader, self.test_loader
        return make_loaders(self.args)

    def _reset(self, choice):
        """the checkpoint's values of what a candidate changes; the path bookkeeping of a fresh warmed-up supernet; then the choice"""
        model = self.model
        with torch.no_grad():
            params = dict(model.named_parameters())
            for n, v in self._snapshot.items():
                params[n].data.copy_(v)
        for obj, keys, book in [(model, _NET_KEYS, self._net_book)] + [(b, _BLOCK_KEYS, bk) for b, bk in zip(model._blocks, self._block_book)]:
            for k in keys:
                obj.__dict__.pop(k, None)
            obj.__dict__.update(copy.deepcopy(book))
        if choice is not None:
            model.configure_choice(choice)
        model.configure_path_sampling_strategy("fixed-path")
        if self.last_only:
            model.set_mode_to_finelune_last_only()
        else:
            model.set_mode_to_normal_mode()

    def evaluate(self, choice=None):
        """score one candidate (None: a random one, drawn by the first forward as a fresh supernet draws it)"""
        from ..eval_subnet_from_supernet import make_optimizer_and_schedule
        a, model = self.args, self.model
        self._reset(choice)
        print("Finetune last only ..." if self.last_only else "Finetuning the whole supernet.")
        train_loader, test_loader = self._loaders()
        l2_loss_fn, optimizer, lr_scheduler = make_optimizer_and_schedule(model, a)
        lr_scheduler.step(epoch=-1)
        logs = train_and_test_one_epoch(model, 0, optimizer, lr_scheduler, train_loader, test_loader, self.loss_fn, l2_loss_fn,
                                        a.train_batch_size, a.gpu, max_train_steps=a.max_train_steps, max_eval_steps=a.max_eval_steps,
                                        test_interval=max(2, a.max_train_steps), test_only_at_last_step=(a.test_only_at_last_step == 1),
                                        grad_clip_value=5.0, last_layer_step=self.fused_last_layer and self.last_only)
        return {"choice": copy.deepcopy(model.choice), "test_acc": logs["test_Accuracy"], "test_auroc": logs["test_AUROC"],
                "test_loss": logs["test_loss"]}

    def close(self):
        """release the engine's plans, graphs and uncached arenas and the snapshot now (not at some later garbage collection)"""
        model = getattr(self, "model", None)
        if model is None:
            return
        eng = getattr(model, "_engine", None)
        if eng is not None:
            eng.close()
        self._snapshot = None
        self.train_loader = self.test_loader = None
        self.model = None
        del model, eng
        gc.collect()
        torch.cuda.empty_cache()


def evaluate_candidate(evaluator, tokenizer, choice, kwargs):
    """one search result ({choice, test_*, hash_token[, latency]}) from a resident evaluator — searcher_utils'
    _create_model_train_and_get_results with the set-up taken out: latency-aware search (beta != 0) still builds its fixed model"""
    results = evaluator.evaluate(choice)
    results["hash_token"] = tokenizer.hash_token(tokenizer.tokenize(results["choice"]))
    if kwargs.get("beta", 0.0) != 0.0:
        from .searcher_utils import fixed_model_latency
        results["latency"] = fixed_model_latency(evaluator.args, results["choice"], evaluator.args.gpu, kwargs)
    return results


def make_evaluator(args, gpu_id):
    """the evaluator of one resident search worker: the checkpoint from args.ckpt_path, read by the worker itself"""
    return ResidentCandidateEvaluator(args, None, gpu=gpu_id)


def worker_main(factory, args, gpu_id, tokenizer, kwargs, inbox, outbox):
    """process entry of a resident search worker: build one evaluator, then score (job_id, choice) messages until None.  A failure
    is reported as ("error", message) and ends the worker with exit code 1 (the parent raises; the worker is never restarted)."""
    import traceback
    ev = None
    try:
        if not getattr(args, "deterministic_workers", False):
            np.random.seed(None)
        ev = factory(args, gpu_id)
        while True:
            msg = inbox.get()
            if msg is None:
                break
            job_id, choice = msg
            outbox.put((job_id, evaluate_candidate(ev, tokenizer, choice, kwargs)))
    except BaseException:
        outbox.put(("error", "worker on device {}: {}".format(gpu_id, traceback.format_exc())))
        raise SystemExit(1)
    finally:
        if ev is not None and hasattr(ev, "close"):
            ev.close()
