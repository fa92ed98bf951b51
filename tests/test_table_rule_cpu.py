"""TableRule (nasrec_amd/optim_spec.py): the one record per table row rule agrees with what it replaced — the values of OptimSpec's seven
properties per rule as they were before the properties read the record, the table_algo the engine writes into the descriptor
(SupernetEngine._moments_descs), the code the data-parallel ranks compare (utils/dist.table_rule_code) — and names every rule once."""
import pytest
import torch

from nasrec_amd import _lib as L
from nasrec_amd import main_train as MT
from nasrec_amd.optim_spec import TABLE_RULES, OptimSpec, TableRule
from nasrec_amd.utils import dist as D
from test_optim_routing_cpu import _model


def _spec(name, **kw):
    m = _model()
    if kw.get("table_seed"):
        m._embedding.to(torch.bfloat16)
    opt = MT.build_optimizer(name, m, 0.05, **kw)
    return OptimSpec.for_step(opt) if name == "adagrad" else OptimSpec.from_optimizer(opt)


#  rule                    build_optimizer's arguments                                          rows_only rowwise rw_adam adagrad_t bf16   seed moments table_algo                        code
RULES = {
    "dense":                (("adam", {}),                                                      (False, False, False, False, False, 0, True), L.TABLE_ALGO_SAME, 0),
    "dense (sgd)":          (("sgd", {}),                                                       (False, False, False, False, False, 0, True), L.TABLE_ALGO_SAME, 0),
    "plain_adagrad":        (("adagrad", {}),                                                   (True, False, False, False, False, 0, False), None, 0),
    "row_sparse_adam":      (("row-sparse-adam", {}),                                           (True, False, False, False, False, 0, True), L.TABLE_ALGO_SAME, 1),
    "lazy_rmsprop":         (("rmsprop", {}),                                                   (True, False, False, False, False, 0, True), L.TABLE_ALGO_SAME, 0),
    "adagrad":              (("adam-adagrad-tables", {}),                                       (True, False, False, True, False, 0, True), L.TABLE_ALGO_ADAGRAD, 2),
    "rowwise_adagrad":      (("adam-adagrad-tables", dict(table_rowwise=True)),                 (True, True, False, True, False, 0, True), L.TABLE_ALGO_ROWWISE_ADAGRAD, 3),
    "rowwise_adagrad_bf16": (("adam-adagrad-tables", dict(table_rowwise=True, table_seed=3)),   (True, True, False, True, True, 3, True), L.TABLE_ALGO_ROWWISE_ADAGRAD_BF16, 4),
    "rowwise_adam":         (("rowwise-adam", {}),                                              (True, True, True, False, False, 0, True), L.TABLE_ALGO_ROWWISE_ADAM, 5),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_the_record_agrees_with_the_properties_it_replaced(rule):
    (name, kw), props, table_algo, code = RULES[rule]
    spec = _spec(name, **kw)
    assert spec is not None
    assert (spec.rows_only, spec.table_rowwise, spec.rowwise_adam, spec.adagrad_tables, spec.bf16_tables, spec.table_seed, spec.moments) == props
    assert all(type(v) is bool for v in props[:5]) and type(spec.table_seed) is int
    assert spec.table_rule is TABLE_RULES[rule.split(" ")[0]] and isinstance(spec.table_rule, TableRule)
    assert spec.table_rule.table_algo == table_algo  # (what _moments_descs writes; None: Adagrad has no such launch)
    assert D.table_rule_code(spec) == code == spec.table_rule.dp_code
    # the record's own fields against the properties
    r = spec.table_rule
    assert (r.rows_only, r.rowwise, r.bf16) == (spec.rows_only, spec.table_rowwise, spec.bf16_tables) and spec.kind in r.kinds
    assert r.state == ("table_row_state" if spec.adagrad_tables and spec.table_rowwise else "table_state" if spec.adagrad_tables or not spec.moments
                       else "moments")
    assert r.first_moment == ("exp_avg" in spec.state_keys or "momentum_buffer" in spec.state_keys) or r.state != "moments"


def test_the_rules_are_eight_and_no_two_answer_one_descriptor():
    """one rule per (dense rule, sparse_rows, table_algo) — what csrc/optim_moments.hip's resolve_row_form keys on; dense and lazy RMSprop
    share table_algo SAME and sparse_rows 0 and differ in the dense rule, as in the C ABI"""
    assert len(TABLE_RULES) == 8 and len({id(r) for r in TABLE_RULES.values()}) == 8
    keys = [(kind, name == "row_sparse_adam", r.table_algo) for name, r in TABLE_RULES.items() for kind in r.kinds]
    assert len(set(keys)) == len(keys)
    own = [r.table_algo for r in TABLE_RULES.values() if r.table_algo not in (None, L.TABLE_ALGO_SAME)]
    assert sorted(own) == [L.TABLE_ALGO_ADAGRAD, L.TABLE_ALGO_ROWWISE_ADAGRAD, L.TABLE_ALGO_ROWWISE_ADAGRAD_BF16, L.TABLE_ALGO_ROWWISE_ADAM]
    assert D.table_rule_code(None) == 0
    assert sorted(r.dp_code for r in TABLE_RULES.values()) == [0, 0, 0, 1, 2, 3, 4, 5]


#  specs no optimizer maps to: (kind, table_kind) -> the seven properties as they were, and whether _optim_scalars refuses the spec
ODD = {
    ("adam", "rowwise"):              ((False, False, False, True, False, 0, True), True),
    ("adam", "adagrad:5"):            ((False, False, False, True, False, 0, True), True),   # (only the bf16 rule takes a seed)
    ("adam", "rowwise_adam:7"):       ((False, False, False, True, False, 0, True), True),
    ("adam", "dense"):                ((False, False, False, True, False, 0, True), True),   # (a key of TABLE_RULES, no table_kind)
    ("adagrad", "adagrad"):           ((True, False, False, True, False, 0, False), True),
    ("sgd", "rowwise_adam"):          ((True, True, True, False, False, 0, True), True),
    ("adam", "rowwise_adagrad_bf16:"): ((True, True, False, True, True, 0, True), False),
}


@pytest.mark.parametrize("kind,table_kind", sorted(ODD))
def test_odd_specs_answer_as_before(kind, table_kind):
    from nasrec_amd.engine import SupernetEngine
    props, refused = ODD[(kind, table_kind)]
    spec = OptimSpec(kind, table_kind=table_kind)
    assert (spec.rows_only, spec.table_rowwise, spec.rowwise_adam, spec.adagrad_tables, spec.bf16_tables, spec.table_seed, spec.moments) == props
    if refused:
        with pytest.raises(L.EngineError, match="table_kind %r with %s" % (table_kind, kind)):
            SupernetEngine._optim_scalars(L.OptMomentsDesc(), spec)
    else:
        SupernetEngine._optim_scalars(L.OptMomentsDesc(), spec)
