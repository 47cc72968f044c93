"""GPU: the penalised objective's four float64 terms per task and outer iteration (tclip_amd.objective; kernels
k_objective_rows / k_objective_task, csrc/tclip_objective.inc).  The run itself is only observed - every shared output has the
bits of the plain or of the until-stable entry -, the terms follow the reference's fixtures within bounds computed from the
fixtures (tests/helpers/objective.py), and a task's terms do not depend on what shares the call or on iters."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import objective as ob
from helpers import until_stable as us

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHARED = ("u", "v", "alpha", "preds", "criterions", "mm_iters")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else (t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t)


def _same(a, b):
    if a is None or b is None:
        return a is b
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def _call(mod, x_q, x_s, y_s, **kw):
    res = mod.run_em_dirichlet(_dev(x_q), _dev(x_s), _dev(y_s), **kw)
    torch.cuda.synchronize()
    return res


def _kw(g):
    return dict(iters=int(g["iters"]), iter_mm=int(g["iter_mm"]), lambd=int(g["lambd"]), hard=str(g["kind"]).endswith("hard"))


def _inputs(g):
    few = "x_s" in g.files
    return (torch.from_numpy(g["x_q"]), torch.from_numpy(g["x_s"]) if few else None,
            torch.from_numpy(g["y_s"]).squeeze(2) if few else None)


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_run(name):
    from tclip_amd import objective
    g = ob.load(name)
    return g, _call(objective, *_inputs(g), **_kw(g))


def _check_terms(name, g, terms):
    """device terms (N, iters, 4) against the fixture's (iters, N, 4) at every iteration, each figure printed before it is asserted"""
    got = terms.cpu().numpy().transpose(1, 0, 2)
    gap, bound = np.abs(got - g["terms"]), ob.fixture_bounds(g)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(bound > 0, gap / bound, 0.0)
    for i, term in enumerate(("fit_q", "fit_s", "ent", "part")):
        print(f"{name} {term}: largest gap {gap[..., i].max():.3g}, largest share of its bound {share[..., i].max():.3g}")
    assert np.isfinite(got).all()
    for i, term in enumerate(("fit_q", "fit_s", "ent", "part")):
        assert (gap[..., i] <= bound[..., i]).all(), (term, float(share[..., i].max()))
    if "x_s" not in g.files:
        assert not got[..., 1].any(), "fit_s is exactly 0 in zero-shot"


@pytest.mark.parametrize("name", sorted(ob.FIXTURES))
def test_reference_fixture_dense(name):
    from tclip_amd import engine
    g, res = _fixture_run(name)
    plain = _call(engine, *_inputs(g), **_kw(g))
    for key in SHARED:
        assert _same(getattr(res, key), getattr(plain, key)), key
    assert res.outer_iters is None and res.changes is None
    for key in ("u", "v", "alpha"):               # what the parity tests assert of the plain entry on the reference's fixtures
        assert np.array_equal(getattr(res, key).cpu().numpy(), g[key]), key
    assert np.array_equal(res.criterions[0].cpu().numpy(), g["criterions"])
    assert res.objective_terms.dtype == torch.float64 and tuple(res.objective_terms.shape) == (int(g["N"]), int(g["iters"]), 4)
    _check_terms(name, g, res.objective_terms)


@pytest.mark.parametrize("name", sorted(ob.FIXTURES))
def test_reference_fixture_tables(name):
    """the same through run_em_dirichlet_tasks: the tables are the stacked task rows, shuffled; few-shot with a column
    permutation per task"""
    from tclip_amd import objective
    g, dense = _fixture_run(name)
    x_q, x_s, y_s = _inputs(g)
    table_q, q_idx, table_s, s_idx, cols = ob.as_tables(x_q, x_s, seed=5, permute=x_s is not None)
    res = objective.run_em_dirichlet_tasks(_dev(table_q), q_idx, _dev(table_s), s_idx, y_s, cols, **_kw(g))
    torch.cuda.synchronize()
    for key in SHARED:
        assert _same(getattr(res, key), getattr(dense, key)), key
    _check_terms(name, g, res.objective_terms)
    if cols is None:       # the same rows in the same columns: the same sums in the same order
        assert _same(res.objective_terms, dense.objective_terms)


@pytest.mark.parametrize("name", sorted(ob.FIXTURES))
def test_the_objective_descends_where_the_references_does(name):
    """per task: where the fixture's own composed sequence never rises, the device's does not either, within the test-1 bounds
    of the two iterations compared"""
    g, res = _fixture_run(name)
    lambd = int(g["lambd"])
    ref = ob.compose(g["terms"], lambd)                                  # (iters, N)
    b = ob.fixture_bounds(g)
    tol = 0.5 * (b[..., 0] + b[..., 1]) + b[..., 2] + lambd * b[..., 3]
    got = ob.compose(res.objective_terms.cpu().numpy(), lambd).T
    falls = (np.diff(ref, axis=0) <= 0).all(0)                           # per task
    print(f"{name}: reference sequence non-increasing for tasks {np.flatnonzero(falls).tolist()} of {ref.shape[1]}")
    rise = np.diff(got, axis=0) - (tol[1:] + tol[:-1])
    assert (rise[:, falls] <= 0).all()


def test_some_fixture_sequence_descends():
    """the test above would show nothing if no task qualified"""
    n = sum(int((np.diff(ob.compose(ob.load(name)["terms"], int(ob.load(name)["lambd"])), axis=0) <= 0).all(0).sum()) for name in ob.FIXTURES)
    assert n >= 10


# ---- 2. observation only -------------------------------------------------------------------------------------------------------------
def _k10():
    g = ob.load("obj_zs_soft_K10_N4")              # the inputs of zs_soft_K10_N4: with patience 2 the batch runs 9 of 20 iterations
    return dict(x_q=torch.from_numpy(g["x_q"]), n_batches=1, iters=20, iter_mm=1000, lambd=150, stops=[us.STOPS["zs_soft_K10_N4"][1]])


def _k100():
    c = us.synthetic_case("two_groups")            # K = 100, four batches of 41 tasks in two stream groups
    return dict(x_q=c["x_q"], n_batches=4, iters=c["iters"], iter_mm=c["iter_mm"], lambd=c["lambd"], stops=c["stops"])


@pytest.mark.parametrize("case", [_k10, _k100], ids=["K10", "K100"])
def test_the_run_is_only_observed(case):
    from tclip_amd import engine, objective, until_stable
    c = case()
    kw = dict(n_batches=c["n_batches"], iters=c["iters"], iter_mm=c["iter_mm"], lambd=c["lambd"])
    plain, seen = _call(engine, c["x_q"], None, None, **kw), _call(objective, c["x_q"], None, None, **kw)
    for key in SHARED:
        assert _same(getattr(seen, key), getattr(plain, key)), key
    assert bool(seen.objective_terms[..., 0].all()) and bool(seen.objective_terms[..., 2:].all())
    stable = _call(until_stable, c["x_q"], None, None, patience=2, **kw)
    both = _call(objective, c["x_q"], None, None, patience=2, **kw)
    for key in SHARED + ("outer_iters", "changes"):
        assert _same(getattr(both, key), getattr(stable, key)), key
    assert both.outer_iters.tolist() == c["stops"] and min(c["stops"]) < c["iters"]
    N = c["x_q"].shape[0] // c["n_batches"]
    for b, s in enumerate(c["stops"]):
        sl = slice(b * N, (b + 1) * N)
        assert not both.objective_terms[sl, s:].any(), b                  # exactly 0 from outer_iters[b] on
        assert _same(both.objective_terms[sl, :s], seen.objective_terms[sl, :s]), b      # and the full run's before


@pytest.mark.parametrize("case", [_k10, _k100], ids=["K10", "K100"])
def test_prefix_consistency(case):
    from tclip_amd import objective
    c = case()
    T = c["x_q"].shape[0]
    x_q = c["x_q"][:min(T, 2 * (T // c["n_batches"]))] if c["n_batches"] > 1 else c["x_q"]
    kw = dict(n_batches=min(c["n_batches"], 2), iter_mm=c["iter_mm"], lambd=c["lambd"])
    full = _call(objective, x_q, None, None, iters=6, **kw)
    for s in (1, 3):
        short = _call(objective, x_q, None, None, iters=s, **kw)
        assert _same(full.objective_terms[:, :s], short.objective_terms), s


# ---- 3. company -------------------------------------------------------------------------------------------------------------------------
def test_terms_do_not_depend_on_what_shares_the_call():
    """B = 3 batches of N = 60 tasks at K = 100: 18 000 rows, two stream groups (n_groups_of); every batch alone gives the bits"""
    from tclip_amd import objective
    K, N, specs = 100, 60, [(11, 3), (12, 6), (13, None)]
    assert len(specs) * N * K // 8192 == 2
    x_q, _ = us.synthetic_batches(K, N, specs)
    kw = dict(iters=3, iter_mm=120, lambd=int(K / 5) * 75)
    together = _call(objective, x_q, None, None, n_batches=3, **kw)
    for b in range(3):
        sl = slice(b * N, (b + 1) * N)
        alone = _call(objective, x_q[sl], None, None, n_batches=1, **kw)
        assert _same(together.objective_terms[sl], alone.objective_terms), b
        for key in ("u", "v", "alpha", "preds"):
            assert _same(getattr(together, key)[sl], getattr(alone, key)), (b, key)
    again = _call(objective, x_q, None, None, n_batches=3, **kw)
    assert _same(again.objective_terms, together.objective_terms)


# ---- 4. shapes ----------------------------------------------------------------------------------------------------------------------------
MODES = {"zs_soft": (False, False), "zs_hard": (False, True), "fs_soft": (True, False), "fs_hard": (True, True)}


def _check_shape(mode, K, Q, T, seed):
    """the last iteration's terms against the float64 restatement from the returned fp32 alpha, u and the inputs.  Few-shot:
    S = K + 3 support rows with unbalanced labels; soft runs leave class K - 1 without a support row (cnt = 0).  Hard few-shot
    keeps one row per class: an empty cluster without support divides 0 by 0 in the M-step, in the reference too."""
    from tclip_amd import objective
    few, hard = MODES[mode]
    x_q, x_s, y_s = ob.make_tasks(T, Q, K, K + 3 if few else 0, seed, empty_class=few and not hard)
    if few and not hard:
        assert not (y_s == K - 1).any()
    lambd = int(K / 5) * Q
    res = _call(objective, x_q, x_s, y_s, iters=2, iter_mm=60, lambd=lambd, hard=hard)
    want, bound = ob.restate(x_q, x_s, y_s, res.alpha.cpu(), res.u.cpu())
    got = res.objective_terms[:, -1].cpu().numpy()
    gap = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(bound > 0, gap / bound, 0.0).max(0)
    print(f"{mode} K={K} Q={Q} T={T}: share of the bounds fit_q {share[0]:.3g} fit_s {share[1]:.3g} ent {share[2]:.3g} part {share[3]:.3g}")
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert (gap <= bound).all(), (mode, K, Q, T, share.tolist())
    assert bool(res.objective_terms[:, 0, 0].all())


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("K", [2, 3, 16, 17, 33, 130, 257])
def test_shapes(K, mode):
    for Q in (1, 2, 75, 77, 300):
        for T in (1, 5):
            _check_shape(mode, K, Q, T, seed=1000 * K + 10 * Q + T)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_shape_K1000(mode):
    _check_shape(mode, 1000, 75, 1, seed=77)


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from tclip_amd import _capi, engine
    lib = _capi.lib()
    T, Q, K, iters = 2, 75, 10, 3
    p = _capi.Problem(1, T, Q, K, 0, iters, 100, 150, 0)
    query = lib.tclip_em_dirichlet_objective_workspace_bytes
    plain, stable = lib.tclip_workspace_bytes(ctypes.byref(p)), lib.tclip_em_dirichlet_until_stable_workspace_bytes(ctypes.byref(p))
    n0, n2 = query(ctypes.byref(p), 0), query(ctypes.byref(p), 2)
    assert n0 >= plain + T * Q * 16 and n2 >= stable + T * Q * 16 and n2 > n0 and query(ctypes.byref(p), -1) == 0
    assert query(ctypes.byref(_capi.Problem(1, T, Q, 1, 0, iters, 100, 150, 0)), 0) == 0
    x_q = ob.make_tasks(T, Q, K, 0, seed=1)[0].to(DEV)
    mark = 7.0
    u, v, alpha = (torch.full(s, mark, device=DEV) for s in ((T, Q, K), (T, K), (T, K, K)))
    preds = torch.full((T, Q), 7, dtype=torch.int32, device=DEV)
    crit, mm = torch.full((1, iters), mark, device=DEV), torch.full((1, iters), 7, dtype=torch.int32, device=DEV)
    outer, changes = torch.full((1,), 7, dtype=torch.int32, device=DEV), torch.full((1, iters), 7, dtype=torch.int32, device=DEV)
    terms = torch.full((T, iters, 4), mark, dtype=torch.float64, device=DEV)
    ws = torch.empty(n2 + 256, dtype=torch.uint8, device=DEV)
    wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    ptr = engine._ptr

    def run(patience, terms_ptr):
        return lib.tclip_em_dirichlet_run_objective(ctypes.byref(p), ptr(x_q), None, None, patience, ptr(u), ptr(v), ptr(alpha),
                                                    ptr(preds), ptr(crit), ptr(mm), ptr(outer), ptr(changes), terms_ptr, wp, n2,
                                                    engine._stream())
    assert run(-1, ptr(terms)) == 1 and b"patience" in lib.tclip_last_error()
    assert run(0, None) == 1 and b"objective_terms" in lib.tclip_last_error()
    assert run(2, None) == 1 and b"objective_terms" in lib.tclip_last_error()
    assert lib.tclip_em_dirichlet_run_objective(ctypes.byref(p), ptr(x_q), None, None, 0, ptr(u), ptr(v), ptr(alpha), ptr(preds),
                                                ptr(crit), ptr(mm), None, None, ptr(terms), wp, n0 - 1, engine._stream()) == 2
    torch.cuda.synchronize()
    for t in (u, v, alpha, crit, terms):
        assert bool((t == mark).all())
    for t in (preds, mm, outer, changes):
        assert bool((t == 7).all())
    # and the same arguments, valid: patience 0 takes null outer_iters / changes and the smaller workspace
    assert lib.tclip_em_dirichlet_run_objective(ctypes.byref(p), ptr(x_q), None, None, 0, ptr(u), ptr(v), ptr(alpha), ptr(preds),
                                                ptr(crit), ptr(mm), None, None, ptr(terms), wp, n0, engine._stream()) == 0
    torch.cuda.synchronize()
    plain_res = engine.run_em_dirichlet(x_q, iters=iters, iter_mm=100, lambd=150)
    torch.cuda.synchronize()
    assert _same(u, plain_res.u) and _same(alpha, plain_res.alpha) and bool(terms[..., 0].all())


# ---- 6. classes and evaluators ------------------------------------------------------------------------------------------------------
def _eval_args(shots, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=6, iter_mm=120, num_classes_test=10, n_class=10, n_query=75, k_eff=5, T=30, shots=shots,
                use_softmax_feature=True, graph_matching=True, name_method="EM_DIRICHLET", number_tasks=6, batch_size=3,
                used_test_set="test", dataset="synthetic", tunable=False)
    a.update(kw)
    return a


def test_zero_shot_evaluator():
    from src.eval_zero_shot import Evaluator_zero_shot
    from tclip_amd import objective, synth
    K = 10
    feats, labels = synth.make_feature_table(K, 30, seed=3)
    ev = Evaluator_zero_shot(device=torch.device(DEV), args=_eval_args(0, record_objective=True), log_file=None)
    torch.manual_seed(11)
    np.random.seed(11)
    idx = ev.sample_indices(labels.numpy())
    B, N, Q = idx.shape
    assert (B, N) == (2, 3)
    ev.evaluate_tasks(None, feats, labels, indices=idx)
    x_q = feats[idx.reshape(-1)].view(B * N, Q, K)
    lambd = int(K / 5) * Q
    res = _call(objective, x_q, None, None, n_batches=B, iters=6, iter_mm=120, lambd=lambd)
    want = objective.objective(res.objective_terms, lambd).cpu().numpy().reshape(B, N, 6)
    assert ev.last_task_objectives.shape == (2, 3, 6) and ev.last_task_objectives.dtype == np.float64
    assert np.array_equal(ev.last_task_objectives, want)
    m = ev.last_method
    assert np.array_equal(m.objective_terms, res.objective_terms.cpu().numpy()) and m.objectives.shape == (B * N, 6)
    # without the option: the same accuracies and predictions, and no trace of the record
    ev0 = Evaluator_zero_shot(device=torch.device(DEV), args=_eval_args(0), log_file=None)
    ev0.evaluate_tasks(None, feats, labels, indices=idx)
    assert np.array_equal(ev0.last_task_accuracies, ev.last_task_accuracies)
    assert np.array_equal(ev0.last_task_predictions, ev.last_task_predictions)
    assert np.array_equal(ev0.last_batch_criterions, ev.last_batch_criterions)
    assert np.array_equal(ev0.last_batch_mm_iters, ev.last_batch_mm_iters)
    assert not hasattr(ev0, "last_task_objectives") and not hasattr(ev0.last_method, "objectives")


def test_few_shot_evaluator():
    """tables in place: the class reads its task rows through the index tensors"""
    from src.eval_few_shot import Evaluator_few_shot
    from tclip_amd import objective, synth
    K = 10
    feats_s, labels_s = synth.make_feature_table(K, 12, seed=4)
    feats_q, labels_q = synth.make_feature_table(K, 30, seed=5)
    ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(2, record_objective=True), log_file=None)
    torch.manual_seed(12)
    np.random.seed(12)
    indices = ev.sample_indices(labels_s.numpy(), labels_q.numpy())
    ev.evaluate_tasks(None, feats_s, labels_s, feats_q, labels_q, indices=indices)
    t = ev._tasks(feats_s, labels_s, feats_q, labels_q, indices)
    si, qi, _, _, rel = ev._block(t)
    assert rel is not None and ev.last_method.rows_in_place(ev.args) and (t.n_batches, t.N) == (2, 3)
    cols, y_s, y_q = rel
    tab_s, tab_q = t.tables()
    lambd = int(K / 5) * t.Q
    res = objective.run_em_dirichlet_tasks(tab_q, qi, tab_s, si, y_s, cols, n_batches=t.n_batches, iters=6, iter_mm=120, lambd=lambd)
    torch.cuda.synchronize()
    want = objective.objective(res.objective_terms, lambd).cpu().numpy().reshape(2, 3, 6)
    assert ev.last_task_objectives.shape == (2, 3, 6) and np.array_equal(ev.last_task_objectives, want)
    assert bool(res.objective_terms[..., 1].all())                       # few-shot: the support term is there
    ev0 = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(2), log_file=None)
    ev0.evaluate_tasks(None, feats_s, labels_s, feats_q, labels_q, indices=indices)
    assert np.array_equal(ev0.last_task_accuracies, ev.last_task_accuracies)
    assert np.array_equal(ev0.last_task_predictions, ev.last_task_predictions)
    assert not hasattr(ev0, "last_task_objectives")


def test_logs_gain_the_key_only_under_the_option():
    from src.methods.zero_shot.em_dirichlet import EM_DIRICHLET
    from src.utils import CfgNode
    from tclip_amd import synth
    K, N = 10, 3
    x_q, y_q = synth.make_query_tasks(N, K, seed=7)
    logs = {}
    for key, extra in (("plain", {}), ("record", dict(record_objective=True)), ("both", dict(record_objective=True, stop_patience=1))):
        args = CfgNode(iter=8, iter_mm=120, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, use_softmax_feature=True,
                       graph_matching=True, **extra)
        m = EM_DIRICHLET(model=None, device=torch.device(DEV), log_file=None, args=args)
        logs[key] = (m.run_task({"x_q": x_q.clone(), "y_q": y_q.clone()}), m)
    assert "objectives" not in logs["plain"][0] and not hasattr(logs["plain"][1], "objectives")
    rec, m = logs["record"]
    assert rec["objectives"].shape == (N, 8) and rec["objectives"].dtype == np.float64 and m.objective_terms.shape == (N, 8, 4)
    assert np.array_equal(rec["acc"], logs["plain"][0]["acc"]) and np.array_equal(rec["criterions"], logs["plain"][0]["criterions"])
    assert sorted(set(rec) - set(logs["plain"][0])) == ["objectives"]
    both, mb = logs["both"]
    s = int(mb.outer_iters[0])
    assert np.array_equal(both["objectives"][:, :s], rec["objectives"][:, :s]) and not both["objectives"][:, s:].any()
