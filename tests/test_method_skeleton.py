"""CPU: the skeleton the reference-named method classes share (src/methods/_em_dirichlet_base.py): the four rules that
spread one wall time over the reference's per-iteration records, the logger names, the argument defaults and the
evaluator's question whether a class reads its task rows in place."""
import pytest
import torch

from src.methods._em_dirichlet_base import MethodBase
from src.utils import CfgNode

ZERO_SHOT = [("em_dirichlet", "EM_DIRICHLET"), ("hard_em_dirichlet", "HARD_EM_DIRICHLET"), ("soft_kmeans", "SOFT_KMEANS"),
             ("hard_kmeans", "HARD_KMEANS"), ("kl_kmeans", "KL_KMEANS"), ("em_gaussian", "EM_GAUSSIAN"),
             ("em_gaussian_cov", "EM_GAUSSIAN_COV"), ("inductive_clip", "CLIP")]
FEW_SHOT = [("em_dirichlet", "EM_DIRICHLET"), ("hard_em_dirichlet", "HARD_EM_DIRICHLET"), ("paddle", "PADDLE"),
            ("tim", "TIM_GD"), ("tim", "ALPHA_TIM"), ("bdcspn", "BDCSPN"), ("laplacian_shot", "LAPLACIAN_SHOT")]
OWN_LOGGER = {"CLIP", "BDCSPN", "LAPLACIAN_SHOT"}       # every other class logs under the shared base module's name


def _cls(kind, module, name):
    return getattr(__import__(f"src.methods.{kind}.{module}", fromlist=[name]), name)


def _args(**extra):
    # no iter_mm: only the EM-Dirichlet YAMLs have one
    return CfgNode(iter=2, num_classes_test=20, n_class=20, n_query=75, T=30, use_softmax_feature=True, graph_matching=True,
                   lambd=1.0, norm_type="L2N", temp=30.0, loss_weights=[1.0, 1.0, 1.0], lr_tim=1e-4, lr_alpha_tim=1e-4,
                   entropies=["Shannon", "Alpha", "Alpha"], alpha_value=7.0, knn=3, lmd=0.7, batch_size=2, shots=1, **extra)


def test_timestamp_rules():
    """expected values by hand from the formulas of the reference files the classes mirror, total = 6 s, 3 iterations, 2 tasks"""
    spread = MethodBase.spread_time
    assert spread("cumulative", 6.0, 3, 2) == [1.0, 2.0, 3.0]            # total*(i+1)/iter/n_task
    assert spread("share", 6.0, 3, 2) == [1.0, 1.0, 1.0]                 # total/iter/n_task
    assert spread("twice", 6.0, 3, 2) == [2.0, 1.0, 2.0, 1.0, 2.0, 1.0]  # total/iter, then that over n_task
    assert spread("per_task", 6.0, 3, 2) == [3.0, 6.0]                   # total*(t+1)/n_task
    for rule in ("cumulative", "share", "twice"):
        assert spread(rule, 6.0, 0, 2) == []
    assert spread("per_task", 6.0, 0, 2) == [3.0, 6.0]
    with pytest.raises(ValueError, match="rule"):
        spread("evenly", 6.0, 3, 2)


@pytest.mark.parametrize("kind,module,name", [("zero_shot", m, n) for m, n in ZERO_SHOT] + [("few_shot", m, n) for m, n in FEW_SHOT])
def test_logger_names_and_argument_defaults(kind, module, name):
    cls = _cls(kind, module, name)
    em_dirichlet = name in ("EM_DIRICHLET", "HARD_EM_DIRICHLET")
    given = {"iter_mm": 100} if em_dirichlet else {}
    if kind == "few_shot" and name not in ("TIM_GD", "ALPHA_TIM"):
        given["k_eff"] = 4              # the few-shot lambd of the shared base reads it; only the TIM classes default it
    a = _args(**given)
    before = set(a)
    m = cls(model=None, device=torch.device("cpu"), log_file=None, args=a)
    want = f"src.methods.{kind}.{module}" if name in OWN_LOGGER else "src.methods._em_dirichlet_base"
    assert m.logger.logger.name.rsplit(".", 1)[0] == want
    added = {k: a[k] for k in set(a) - before}
    if name in ("TIM_GD", "ALPHA_TIM"):
        assert added == {"iter_mm": 0, "k_eff": 5}
    elif name in OWN_LOGGER or em_dirichlet:
        assert added == {}
    else:
        assert added == {"iter_mm": 0}
    assert (m.timestamps, m.criterions, m.test_acc) == ([], [], [])
    # a value the configuration has is kept
    a2 = _args(iter_mm=7, k_eff=3)
    cls(model=None, device=torch.device("cpu"), log_file=None, args=a2)
    assert (a2.iter_mm, a2.k_eff) == (7, 3)


def test_which_classes_read_task_rows_in_place():
    """what Evaluator_few_shot.evaluate_tasks asks before it chooses between run_tables and run_batch"""
    want = {"EM_DIRICHLET": (True, False), "HARD_EM_DIRICHLET": (True, False), "PADDLE": (True, True)}
    for module, name in FEW_SHOT:
        cls = _cls("few_shot", module, name)
        assert (cls.reads_rows_in_place(True), cls.reads_rows_in_place(False)) == want.get(name, (False, False)), name
        assert callable(cls.run_batch) and callable(cls.run_method)
