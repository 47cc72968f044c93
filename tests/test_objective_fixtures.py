"""CPU: the objective fixtures (tests/golden/objective/obj_*.npz, made by tests/golden/make_golden_objective.py from the reference)
pin the four terms' definitions to the reference's own `objective_function`, and the surface the option adds is there:
the three C symbols, the patience check of tclip_amd.objective, the evaluators' refusal for other methods."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import objective as ob
from tclip_amd import _capi

NEW_SYMBOLS = ("tclip_em_dirichlet_objective_workspace_bytes", "tclip_em_dirichlet_run_objective",
               "tclip_em_dirichlet_run_tasks_objective")


def test_the_fixtures_are_the_issues_table():
    assert sorted(f[:-4] for f in os.listdir(ob.OBJ_DIR) if f.endswith(".npz")) == sorted(ob.FIXTURES)
    for name, (kind, K, N, shots, iters) in ob.FIXTURES.items():
        g = ob.load(name)
        assert (str(g["kind"]), int(g["K"]), int(g["N"]), int(g["shots"]), int(g["iters"])) == (kind, K, N, shots, iters), name
        assert g["terms"].shape == g["abs_sums"].shape == (iters, N, 4) and g["terms"].dtype == np.float64
        assert g["ref_objective"].shape == g["fit_s_scale"].shape == (iters, N) and g["ref_objective"].dtype == np.float32
        assert g["u"].shape == (N, 75, K) and g["alpha"].shape == (N, K, K) and g["v"].shape == (N, K)
        assert int(g["lambd"]) == int(K / 5) * 75
        assert os.path.getsize(os.path.join(ob.OBJ_DIR, name + ".npz")) < 1 << 20
        few = kind.startswith("fs")
        assert ("x_s" in g.files) == few and bool((g["terms"][..., 1] != 0).all()) == few
        assert np.isfinite(g["terms"]).all() and (g["abs_sums"] >= np.abs(g["terms"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", sorted(ob.FIXTURES))
def test_composed_terms_are_the_references_objective(name):
    """The objective composed from the float64 terms against the reference's fp32 objective_function at the same state, within
    the a-priori bound of its fp32 sums: 2^-24 (Q K A_q / 2 + S K A_s / 2 + Q K A_ent + lambd K A_part)."""
    g = ob.load(name)
    K, Q, lambd = int(g["K"]), g["x_q"].shape[1], int(g["lambd"])
    S = g["x_s"].shape[1] if "x_s" in g.files else 0
    A = g["abs_sums"]
    bound = 2.0 ** -24 * (0.5 * Q * K * A[..., 0] + 0.5 * S * K * A[..., 1] + Q * K * A[..., 2] + lambd * K * A[..., 3])
    gap = np.abs(ob.compose(g["terms"], lambd) - g["ref_objective"].astype(np.float64))
    print(f"{name}: largest gap {gap.max():.3g}, largest share of the bound {(gap / bound).max():.3g}")
    assert (gap <= bound).all(), (gap / bound).max()
    # the bound is no licence: the composed value follows the reference's to 4e-5 relative at worst
    assert (gap <= 4e-5 * np.abs(g["ref_objective"])).all()


def test_capi_exposes_the_three_symbols():
    lib = _capi.lib()
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    res, args = _capi._SIGNATURES["tclip_em_dirichlet_run_objective"]
    stable = _capi._SIGNATURES["tclip_em_dirichlet_run_until_stable"][1]
    assert res is ctypes.c_int and len(args) == len(stable) + 1        # objective_terms after changes
    assert len(_capi._SIGNATURES["tclip_em_dirichlet_run_tasks_objective"][1]) == \
        len(_capi._SIGNATURES["tclip_em_dirichlet_run_tasks_until_stable"][1]) + 1


def test_workspace_query_and_argument_errors_need_no_device():
    """the query's relations to the two existing ones; a negative patience and a null objective_terms are TCLIP_ERR_ARG before
    any launch (so this runs without a GPU), the argument named in the error text"""
    lib = _capi.lib()
    query = lib.tclip_em_dirichlet_objective_workspace_bytes
    for shape in ((1, 4, 75, 10, 0), (3, 60, 75, 100, 0), (2, 3, 77, 37, 74), (10, 125, 75, 1000, 0)):
        p = _capi.Problem(*shape, 5, 120, 150, 0)
        plain, stable = lib.tclip_workspace_bytes(ctypes.byref(p)), lib.tclip_em_dirichlet_until_stable_workspace_bytes(ctypes.byref(p))
        rows = shape[0] * shape[1] * shape[2] * 16
        assert plain + rows <= query(ctypes.byref(p), 0) <= plain + rows + 256 * 16
        assert stable + rows <= query(ctypes.byref(p), 1) == query(ctypes.byref(p), 3) <= stable + rows + 256 * 16
        assert query(ctypes.byref(p), -1) == 0
        # no dependence on the support size beyond the plain workspace's own
        if shape[4]:
            q = _capi.Problem(*shape[:4], 2 * shape[4], 5, 120, 150, 0)
            assert query(ctypes.byref(q), 0) - lib.tclip_workspace_bytes(ctypes.byref(q)) == query(ctypes.byref(p), 0) - plain
    assert query(ctypes.byref(_capi.Problem(1, 4, 75, 1, 0, 5, 120, 150, 0)), 0) == 0          # n_class < 2
    assert query(None, 0) == 0
    p = _capi.Problem(1, 4, 75, 10, 0, 5, 120, 150, 0)
    P = ctypes.c_void_p(4096)          # never dereferenced: the checks fail first
    ARG = 1
    dense = lambda patience, terms: lib.tclip_em_dirichlet_run_objective(      # noqa: E731
        ctypes.byref(p), P, None, None, patience, P, P, P, P, P, P, P, P, terms, P, 1 << 40, None)
    src = _capi.TaskSource(4096, 4096, None, None, None)
    table = lambda patience, terms: lib.tclip_em_dirichlet_run_tasks_objective(      # noqa: E731
        ctypes.byref(p), ctypes.byref(src), None, patience, P, P, P, P, P, P, P, P, terms, P, 1 << 40, None)
    for call in (dense, table):
        assert call(-1, P) == ARG and b"patience" in lib.tclip_last_error()
        assert call(0, None) == ARG and b"objective_terms" in lib.tclip_last_error()
        assert call(2, None) == ARG and b"objective_terms" in lib.tclip_last_error()
    assert lib.tclip_em_dirichlet_run_objective(ctypes.byref(p), P, None, None, 2, P, P, P, P, P, P, None, P, P, P, 1 << 40, None) == ARG
    assert b"outer_iters" in lib.tclip_last_error()


@pytest.mark.parametrize("patience", [-1, 0, 1.5, "2", True])
def test_a_bad_patience_is_refused(patience):
    """before the tensors are looked at: they live on the CPU here"""
    from tclip_amd import objective
    x = torch.full((2, 75, 10), 0.1)
    with pytest.raises(ValueError, match="patience"):
        objective.run_em_dirichlet(x, patience=patience, iters=2, lambd=150)
    with pytest.raises(ValueError, match="patience"):
        objective.run_em_dirichlet_tasks(x.view(-1, 10), torch.arange(150).view(2, 75), patience=patience, iters=2, lambd=150)


def test_objective_composes_the_references_value():
    from tclip_amd import objective
    terms = np.array([[[2.0, 4.0, -1.0, -0.5], [0.0, 0.0, 0.0, 0.0]]])
    assert objective.objective(terms, 150).tolist() == [[-3.0 - 1.0 + 75.0, 0.0]]
    t = torch.from_numpy(terms)
    assert torch.equal(objective.objective(t, 150), torch.from_numpy(objective.objective(terms, 150))) and t.dtype == torch.float64


def _args(method, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=3, iter_mm=100, num_classes_test=10, n_class=10, n_query=75, k_eff=5, T=30, shots=2, use_softmax_feature=True,
                graph_matching=True, name_method=method, lambd=1.0, number_tasks=2, batch_size=1, used_test_set="test",
                dataset="synthetic", tunable=False)
    a.update(kw)
    return a


@pytest.mark.parametrize("method", ["SOFT_KMEANS", "PADDLE"])
def test_other_methods_refuse_the_option(method):
    """before any device work: the tables are CPU tensors, the device is one this machine may not have, nothing is drawn"""
    from src.eval_few_shot import Evaluator_few_shot
    from src.eval_zero_shot import Evaluator_zero_shot
    feats, labels = torch.full((40, 10), 0.1), torch.arange(10).repeat_interleave(4)
    if method == "PADDLE":
        ev = Evaluator_few_shot(device=torch.device("cuda:0"), args=_args(method, record_objective=True), log_file=None)
        call = lambda: ev.evaluate_tasks(None, feats, labels, feats, labels)      # noqa: E731
    else:
        ev = Evaluator_zero_shot(device=torch.device("cuda:0"), args=_args(method, record_objective=True), log_file=None)
        call = lambda: ev.evaluate_tasks(None, feats, labels)      # noqa: E731
    with pytest.raises(ValueError, match="record_objective"):
        call()


def test_the_option_is_absent_unless_given():
    from src._evaluator import arg_hidden, check_record_objective
    from src.methods.zero_shot.em_dirichlet import EM_DIRICHLET
    from tclip_amd import sharding
    a = _args("EM_DIRICHLET")
    assert check_record_objective(a) is False and "record_objective" not in a
    m = EM_DIRICHLET(model=None, device=torch.device("cpu"), log_file=None, args=a)
    assert m._record_objective() is False and "record_objective" not in a          # not written into args as a default
    assert sorted(sharding.method_parts(a, None, None, 0, 2, 75, torch.device("cpu"))) == ["acc", "criterions", "mm_iters", "preds"]
    a.record_objective = True
    assert check_record_objective(a) is True and m._record_objective() is True
    parts = sharding.method_parts(a, None, None, 0, 2, 75, torch.device("cpu"))
    assert sorted(parts) == ["acc", "criterions", "mm_iters", "objectives", "preds"]
    assert parts["objectives"].shape == (0, 2, 6) and parts["objectives"].dtype == torch.int32       # iter = 3 float64 values as words
    a.stop_patience = 2
    assert sorted(sharding.method_parts(a, None, None, 0, 2, 75, torch.device("cpu"))) == \
        ["acc", "criterions", "mm_iters", "objectives", "outer_iters", "preds"]
    with arg_hidden(a, "record_objective"):
        assert check_record_objective(a) is False
    assert a.record_objective is True
    a.name_method = "SOFT_KMEANS"
    a.record_objective = False                 # switched off explicitly: nothing to refuse
    assert check_record_objective(a) is False


def test_the_gather_carries_float64_rows_beside_the_old_records():
    """one rank: the objectives come back bit for bit, and every other record has the bytes it has without them"""
    from types import SimpleNamespace as NS
    from tclip_amd import sharding
    gen = torch.Generator().manual_seed(3)
    parts = {"preds": torch.randint(0, 10, (3, 8), generator=gen, dtype=torch.int32), "acc": torch.rand(3, 2, generator=gen),
             "criterions": torch.rand(3, 5, generator=gen), "mm_iters": torch.randint(0, 1000, (3, 5), generator=gen, dtype=torch.int32)}
    before = sharding.gather_packed(parts, 3, rank=0, world_size=1)
    obj = torch.rand(3, 2, 5, generator=gen, dtype=torch.float64) * -1e4
    a = NS(name_method="EM_DIRICHLET", iter=5, record_objective=True)
    m = NS(preds=parts["preds"], criterions_per_batch=parts["criterions"], mm_iters=parts["mm_iters"], objectives=obj.view(6, 5).numpy())
    logs = {"acc": parts["acc"].reshape(6, 1).numpy()}
    made = sharding.method_parts(a, m, logs, 3, 2, 4, torch.device("cpu"))
    assert sorted(made) == ["acc", "criterions", "mm_iters", "objectives", "preds"] and made["objectives"].shape == (3, 2, 10)
    after = sharding.gather_packed(made, 3, rank=0, world_size=1)
    back = sharding.objectives_of(after["objectives"])
    assert back.dtype == torch.float64 and back.shape == (3, 2, 5) and torch.equal(back, obj)
    for name in parts:
        assert before[name].dtype == after[name].dtype == parts[name].dtype and torch.equal(before[name], after[name]), name
