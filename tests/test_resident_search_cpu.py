"""The resident search pool (`--resident_candidates 1`, searcher.py: _ResidentPool) without a GPU: spawned workers with a stand-in
evaluator.  Waves and result order are those of the one-process-per-candidate path, a worker that raises or dies makes the search
raise and is not restarted, no worker outlives the search, and the parser's default keeps the reference's path."""
import multiprocessing
import os

import numpy as np
import pytest

from nasrec_amd import eval_subnet_from_supernet as E
from nasrec_amd.searcher import searcher as S
from nasrec_amd.searcher import searcher_utils as SU


def _args(tmp_path, extra=()):
    a = E.build_parser().parse_args(["--dataset", "kdd", "--config", "autoctr", "--num_blocks", "3", "--use_layernorm", "1",
                                     "--resident_candidates", "1", "--logging_dir", str(tmp_path)] + list(extra))
    a.num_embeddings = [1000] * 10
    a.deterministic_workers = True
    a.starts_file = str(tmp_path / "starts.txt")
    return a


class StandIn:
    """evaluator of one worker: a candidate drawn (or taken) as a fresh CPU supernet would, scored by the worker's device id"""

    def __init__(self, args, gpu_id):
        self.args, self.gpu, self.n = args, gpu_id, 0
        with open(args.starts_file, "a") as f:
            f.write("%s %d\n" % (gpu_id, os.getpid()))

    def evaluate(self, choice):
        mode = getattr(self.args, "fail_mode", None)
        if mode == "raise":
            raise ValueError("stand-in failure")
        if mode == "exit":
            os._exit(3)
        if mode == "hang":
            import time
            time.sleep(600)
        model = SU.build_supernet(self.args, self.args.num_embeddings)
        if choice is not None:
            model.configure_choice(choice)
        model.configure_path_sampling_strategy("fixed-path")
        ch = model._resolve_choice(None)
        self.n += 1
        return {"choice": ch, "test_loss": [float(self.gpu) + 0.01 * self.n], "test_acc": [0.5], "test_auroc": [0.5], "gpu": self.gpu}

    def close(self):
        pass


def make_stand_in(args, gpu_id):
    return StandIn(args, gpu_id)


def test_parser_default_keeps_the_reference_path():
    assert E.build_parser().parse_args([]).resident_candidates == 0
    assert E.build_parser().parse_args(["--resident_candidates", "1"]).resident_candidates == 1
    a = E.build_parser().parse_args([])
    assert S.Searcher(E.finetune_and_eval_one_model, a)._resident is False


def test_pool_waves_and_result_order(tmp_path):
    a = _args(tmp_path)
    s = S.Searcher(E.finetune_and_eval_one_model, a, evaluator_factory=make_stand_in)
    out = s.random_search_from_supernet(budget=7, top_k=7, num_parallel_workers=3, sorted=False, on_cpu=False)
    assert [r["gpu"] for r in s.all_results] == [0, 1, 2, 0, 1, 2, 0]
    # every worker keeps its evaluator: its candidates count up
    assert [r["test_loss"][0] for r in s.all_results] == pytest.approx([0.01, 1.01, 2.01, 0.02, 1.02, 2.02, 0.03])
    assert len(out) == 7 and all(isinstance(r["hash_token"], str) for r in out)
    starts = open(a.starts_file).read().split("\n")[:-1]
    assert sorted(int(x.split()[0]) for x in starts) == [0, 1, 2]  # one long-lived worker per device
    assert multiprocessing.active_children() == []
    assert s._pool is None


def test_regularized_evolution_shares_one_pool(tmp_path):
    a = _args(tmp_path)
    np.random.seed(3)
    s = S.Searcher(E.finetune_and_eval_one_model, a, evaluator_factory=make_stand_in)
    hist = s.regularized_evolution_from_supernet(n_generations=2, n_childs=2, init_population=4, sample_size=3, top_k=2,
                                                 num_parallel_workers=2)
    assert len(hist) == 4
    starts = open(a.starts_file).read().split("\n")[:-1]
    assert len(starts) == 2  # the random phase and the generations ran on the same two workers
    assert multiprocessing.active_children() == []


@pytest.mark.parametrize("mode,needle", [("raise", "stand-in failure"), ("exit", "exited with code 3")])
def test_a_failing_worker_raises_and_is_not_restarted(tmp_path, mode, needle):
    a = _args(tmp_path)
    a.fail_mode = mode
    s = S.Searcher(E.finetune_and_eval_one_model, a, evaluator_factory=make_stand_in)
    with pytest.raises(RuntimeError, match=needle):
        s.random_search_from_supernet(budget=4, top_k=1, num_parallel_workers=1, sorted=False)
    assert len(open(a.starts_file).read().split("\n")[:-1]) == 1
    assert multiprocessing.active_children() == []
    assert s._pool is None


def test_a_hanging_worker_ends_the_search_at_the_deadline(tmp_path):
    import time
    a = _args(tmp_path)
    a.fail_mode = "hang"
    a.resident_worker_timeout = 5
    s = S.Searcher(E.finetune_and_eval_one_model, a, evaluator_factory=make_stand_in)
    t = time.monotonic()
    with pytest.raises(RuntimeError, match="no result within 5 s"):
        s.random_search_from_supernet(budget=2, top_k=1, num_parallel_workers=1, sorted=False)
    assert time.monotonic() - t < 60
    assert multiprocessing.active_children() == []
