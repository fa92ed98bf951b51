"""Random search and regularized evolution over sub-networks of a trained supernet (reference: nasrec/searcher/searcher.py).

Parallelism is the reference's: independent candidates, one process per GPU (`gpu_id = job_id`), no collective — on an 8-GPU
MI355X node `--num_parallel_workers 8` scores 8 candidates at a time.  Workers are spawned (never forked: a process that has
touched the GPU must not be duplicated) and never re-exec."""
import argparse
from copy import deepcopy

import numpy as np
import torch.multiprocessing as mp

from ..search_space import ops_config_lib
from .searcher_utils import create_model_train_and_get_results_helper, get_device_id
from .tokenizer import Tokenizer

_CRITERIA = ["test_loss", "test_acc", "test_auroc", "test_loss_penalty_lat"]


class _ResidentPool:
    """`--resident_candidates 1`: one long-lived spawned worker per GPU (gpu_id = job_id), each holding one
    ResidentCandidateEvaluator (searcher/resident.py) that reads the checkpoint from args.ckpt_path itself.  A wave hands job j to
    worker j and returns the results in _run_jobs' order.  A worker that fails or dies makes the wave raise; it is never restarted."""

    POLL_S = 1.0

    def __init__(self, factory, args, tokenizer, kwargs, on_cpu):
        # a wave that brings no result within this many seconds (args.resident_worker_timeout; None = no limit) ends the search: its
        # workers are stopped and the wave raises
        self.timeout_s = getattr(args, "resident_worker_timeout", None)
        from .resident import worker_main
        self._ctx = mp.get_context("spawn")
        self._main, self._factory, self._args, self._tokenizer, self._kwargs, self._on_cpu = worker_main, factory, args, tokenizer, kwargs, on_cpu
        self._outbox = self._ctx.Queue()
        self.workers = {}  # job_id -> (process, inbox)

    def _worker(self, job_id):
        if job_id not in self.workers:
            inbox = self._ctx.Queue()
            p = self._ctx.Process(target=self._main, args=(self._factory, deepcopy(self._args), get_device_id(job_id, self._on_cpu),
                                                         deepcopy(self._tokenizer), self._kwargs, inbox, self._outbox))
            p.start()
            self.workers[job_id] = (p, inbox)
        return self.workers[job_id]

    def run(self, choices):
        import queue
        import time
        for job_id, choice in enumerate(choices):
            self._worker(job_id)[1].put((job_id, choice))
        got = {}
        deadline = time.monotonic() + self.timeout_s if self.timeout_s else None
        while len(got) < len(choices):
            try:
                job_id, res = self._outbox.get(timeout=self.POLL_S)
            except queue.Empty:
                if deadline is not None and time.monotonic() > deadline:
                    self.close(wait_s=0)
                    raise RuntimeError("the search workers brought no result within %s s: stopped" % self.timeout_s)
                for j in range(len(choices)):
                    p = self.workers[j][0]
                    if j not in got and not p.is_alive():
                        raise RuntimeError("a search worker exited with code %s" % p.exitcode)
                continue
            if job_id == "error":
                raise RuntimeError("a search worker failed: %s" % res)
            got[job_id] = res
        return [got[j] for j in sorted(got, key=lambda j: "worker_{}".format(j))]  # (the order of _run_jobs' return_dict keys)

    def close(self, wait_s: float = 60):
        for p, inbox in self.workers.values():
            if p.is_alive():
                try:
                    inbox.put(None)
                except (OSError, ValueError):
                    pass
        for p, _ in self.workers.values():
            p.join(timeout=wait_s)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
        self.workers = {}


class Searcher(object):
    def __init__(self, eval_fn, args: argparse.Namespace, evaluator_factory=None):
        """evaluator_factory (`--resident_candidates 1`): (args, gpu_id) -> an evaluator with evaluate(choice) and close(), built once
        in each worker process; default: resident.make_evaluator"""
        self._eval_fn = eval_fn
        self._args = args
        self.all_results = []
        self._tokenizer = Tokenizer(num_blocks=args.num_blocks, ops_config=ops_config_lib[args.config])
        self._checkpoint = None
        self._resident = getattr(args, "resident_candidates", 0) == 1
        self._evaluator_factory = evaluator_factory
        self._pool = None

    def _open_pool(self, on_cpu, kwargs) -> bool:
        """start the resident pool if this search uses one and none is open; -> True when this call opened it"""
        if not self._resident or self._pool is not None:
            return False
        factory = self._evaluator_factory
        if factory is None:
            from .resident import make_evaluator
            factory = make_evaluator
        self._pool = _ResidentPool(factory, self._args, self._tokenizer, kwargs, on_cpu)
        return True

    def _close_pool(self):
        pool, self._pool = self._pool, None
        if pool is not None:
            pool.close()

    @staticmethod
    def _sort_results_with_criterion(results: np.ndarray, criterion: str = "test_loss", **kwargs) -> np.ndarray:
        """searcher.py:57-79 (latency-penalised objective: loss + beta * (latency / target - 1))"""
        objs = []
        for r in results:
            if criterion == "test_loss_penalty_lat":
                objs.append(r["test_loss"] + kwargs["beta"] * (r["latency"] / kwargs["target_latency"] - 1))
            else:
                objs.append(r[criterion])
        order = np.argsort(np.asarray(objs).flatten())
        return results[order[::-1]] if criterion in ("test_acc", "test_auroc") else results[order]

    def _sampler(self, population: np.ndarray, num_samples: int, criterion: str = "test_loss") -> np.ndarray:
        return population[np.random.choice(len(population), num_samples, replace=False)]

    @staticmethod
    def _defaults(kwargs):
        kwargs["beta"] = kwargs.get("beta", 0.0)
        kwargs["target_latency"] = kwargs.get("target_latency", -1)
        kwargs["latency_batch_size"] = kwargs.get("latency_batch_size", 512)
        if kwargs["target_latency"] == -1 and kwargs["beta"] != 0:
            kwargs["target_latency"] = 0.0
        return kwargs

    def _run_jobs(self, choices, on_cpu, ckpt_holder, kwargs):
        """one process per candidate of this wave (searcher.py:134-152 / 261-278) -> list of result dicts
        (`--resident_candidates 1`: the candidates go to the resident workers instead)"""
        if self._pool is not None:
            return self._pool.run(choices)
        ctx = mp.get_context("spawn")
        manager = self._manager
        return_dict = manager.dict()
        procs = []
        for job_id, choice in enumerate(choices):
            p = ctx.Process(target=create_model_train_and_get_results_helper,
                            args=(deepcopy(self._args), get_device_id(job_id, on_cpu), self._eval_fn, deepcopy(self._tokenizer), choice,
                                  return_dict, ckpt_holder, kwargs))
            p.start()
            procs.append(p)
        for p in procs:
            p.join()
            if p.exitcode != 0:
                raise RuntimeError("a search worker exited with code %s" % p.exitcode)
        return [return_dict[k] for k in sorted(return_dict.keys())]

    def random_search_from_supernet(self, budget: int = 200, criterion: str = "test_loss", top_k: int = 5, num_parallel_workers: int = 1,
                                    on_cpu: bool = False, sorted: bool = True, **kwargs) -> np.ndarray:
        """searcher.py:88-165"""
        assert num_parallel_workers >= 1, "Should have at least 1 worker!"
        assert top_k <= budget, "Should have 'top_k' smaller than 'budget'."
        if on_cpu:
            assert num_parallel_workers == 1, ValueError("Can only use 'num_parallel_workers=1' when on CPU.")
        assert criterion in _CRITERIA, NotImplementedError("Criterion {} is not supported!".format(criterion))
        kwargs = self._defaults(kwargs)
        self.all_results = []
        owner = self._open_pool(on_cpu, kwargs)
        try:
            ckpt_holder = None
            if not self._resident:
                self._manager = mp.Manager()
                ckpt_holder = self._manager.dict()
            idx = 0
            while idx < budget:
                print("Evaluating {} of {} random networks!".format(idx, budget))
                num_jobs = min(num_parallel_workers, budget - idx)
                self.all_results += self._run_jobs([None] * num_jobs, on_cpu, ckpt_holder, kwargs)
                idx += num_jobs
        finally:
            if owner:
                self._close_pool()
        self.all_results = np.asarray(self.all_results)
        if sorted:
            return self._sort_results_with_criterion(self.all_results, criterion, **kwargs)[:top_k]
        return self.all_results[:top_k]

    def regularized_evolution_from_supernet(self, n_generations: int = 50, n_childs: int = 16, init_population: int = 100, sample_size: int = 5,
                                            criterion: str = "test_loss", skip_random: bool = False, num_parallel_workers: int = 1,
                                            on_cpu: bool = False, top_k: int = 2, **kwargs) -> np.ndarray:
        """searcher.py:167-294: aging evolution — tournament of `sample_size`, the winner's mutated children join the population,
        the oldest `n_childs` members leave; the `top_k` best children of every generation form the returned history."""
        assert criterion in _CRITERIA, NotImplementedError("Criterion {} is not supported!".format(criterion))
        assert top_k <= sample_size, ValueError("You must maintain more than 'top_k' children to append 'top_k' archs to history.")
        assert sample_size < init_population, ValueError("Sample size must be no greater than the number of population ('init_population')!")
        assert num_parallel_workers >= 1, ValueError("Should have at least 1 worker!")
        if init_population < n_childs:
            print("WARNING: For the best effect, you should have more initial population than children!")
        if on_cpu:
            assert num_parallel_workers == 1, ValueError("Can only use 'num_parallel_workers=1' when on CPU.")
        kwargs = self._defaults(kwargs)
        owner = self._open_pool(on_cpu, kwargs)
        try:
            return self._evolve(n_generations, n_childs, init_population, sample_size, criterion, num_parallel_workers, on_cpu, top_k, kwargs)
        finally:
            if owner:
                self._close_pool()

    def _evolve(self, n_generations, n_childs, init_population, sample_size, criterion, num_parallel_workers, on_cpu, top_k, kwargs):
        population = np.asarray(self.random_search_from_supernet(budget=init_population, criterion=criterion, top_k=init_population,
                                                                 num_parallel_workers=num_parallel_workers, on_cpu=on_cpu, sorted=False, **kwargs))
        print("Done random sample!")
        history, visited = [], []
        ckpt_holder = self._manager.dict() if not self._resident else None
        for n_gen in range(n_generations):
            parent = self._sort_results_with_criterion(self._sampler(population, sample_size, criterion), criterion, **kwargs)[0]
            print("Parent Arch: {}".format(parent))
            # more mutations early, fewer late; one per child below 20 generations (searcher.py:243)
            num_mutations = (n_generations - n_gen) // (max(20, n_generations // 5)) + 1
            child_id = 0
            while child_id < n_childs:
                num_jobs = min(n_childs - child_id, num_parallel_workers)
                print("Generation {}, Child {}!".format(n_gen, child_id))
                wave = []
                for _ in range(num_jobs):
                    mutated = deepcopy(parent["choice"])
                    while True:
                        for _ in range(num_mutations):
                            mutated = self._tokenizer.mutate_spec(mutated)
                        h = self._tokenizer.hash_token(self._tokenizer.tokenize(mutated))
                        if h not in visited:
                            visited.append(h)
                            break
                    wave.append(mutated)
                for r in self._run_jobs(wave, on_cpu, ckpt_holder, kwargs):
                    population = np.append(population, r)
                child_id += num_parallel_workers
            best = self._sort_results_with_criterion(population[-n_childs:], criterion, **kwargs)
            history += [best[i] for i in range(top_k)]
            population = population[n_childs:]
        return np.asarray(history)
