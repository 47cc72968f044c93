"""GPU: EM-Dirichlet stopped per batch once its assignments stand still (tclip_amd.until_stable).  The contract is exactness:
a batch that stops after s outer iterations returns, bit for bit, what the plain entry returns for that batch alone with
iters = s, whatever shares the call with it.  The expected stop counts are pinned on the CPU (tests/test_until_stable.py): from
the reference's fixtures, and from oracle.ref_torch for the synthetic calls of several batches."""
import functools

import numpy as np
import pytest
import torch

from helpers import until_stable as us

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("u", "v", "alpha", "preds")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def _call(mod, x_q, x_s, y_s, **kw):
    res = getattr(mod, "run_em_dirichlet")(_dev(x_q), _dev(x_s), _dev(y_s), **kw)
    torch.cuda.synchronize()
    return res


def _check_batch(res, b, N, s, iters, plain):
    """batch b of `res` against the plain run of that batch alone with iters = s"""
    sl = slice(b * N, (b + 1) * N)
    for name in OUTPUTS:
        assert _same(getattr(res, name)[sl], getattr(plain, name)), (b, name)
    assert _same(res.criterions[b, :s], plain.criterions[0]), b
    assert _same(res.mm_iters[b, :s], plain.mm_iters[0]), b
    for name in ("criterions", "mm_iters", "changes"):
        assert not getattr(res, name)[b, s:].any(), (b, name)
    assert int(res.changes[b, 0]) == N * res.preds.shape[1] and s <= iters


# ---- 1. the reference's fixtures, one batch ------------------------------------------------------------------------------------
FIXTURES = [("zs_soft_K10_N4", 2), ("zs_soft_K37_N6", 2), ("zs_soft_K100_N4", 2), ("zs_hard_K37_N6", 2), ("fs_soft_K37_N3_s2", 2),
            ("fs_hard_K10_N4_s4", 2), ("zs_soft_K1000_N3", 2), ("zs_soft_K7_N4", 3), ("fs_hard_K100_N3_s4", 2)]
NEVER = ("zs_soft_K7_N4", "fs_hard_K100_N3_s4")


@pytest.mark.parametrize("name,patience", FIXTURES)
def test_reference_fixture(name, patience):
    from tclip_amd import engine, until_stable
    g = us.load(name)
    kind, K, iters = str(g["kind"]), int(g["K"]), int(g["iters"])
    few = kind.startswith("fs")
    kw = dict(iter_mm=int(g["iter_mm"]), lambd=int(K / 5) * 75, hard=kind.endswith("hard"))
    inputs = (g["x_q"], g["x_s"] if few else None, g["y_s"] if few else None)
    trace = us.changes_of(g["argmax"])
    s = us.stop_of(trace, patience)
    assert s == us.STOPS[name][patience - 1] and (s == iters) == (name in NEVER)
    res = _call(until_stable, *inputs, patience=patience, iters=iters, **kw)
    N, Q = res.preds.shape
    assert res.outer_iters.tolist() == [s]
    assert res.changes[0, :s].tolist() == trace[:s].tolist() and int(res.changes[0, 0]) == N * Q
    assert np.array_equal(res.preds.cpu().numpy(), g["argmax"][s - 1].astype(np.int32))
    assert np.array_equal(res.criterions[0, :s].cpu().numpy(), g["criterions"][:s])
    assert np.array_equal(res.mm_iters[0, :s].cpu().numpy(), g["mm_iters"][:s])
    _check_batch(res, 0, N, s, iters, _call(engine, *inputs, iters=s, **kw))
    if name in NEVER:
        for key in ("u", "v", "alpha"):
            assert np.array_equal(getattr(res, key).cpu().numpy(), g[key]), key


# ---- 2. several batches, several stream groups ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(name):
    from tclip_amd import until_stable
    c = us.synthetic_case(name)
    res = _call(until_stable, c["x_q"], c["x_s"], c["y_s"], patience=c["patience"], n_batches=len(c["specs"]), iters=c["iters"],
                iter_mm=c["iter_mm"], lambd=c["lambd"])
    return c, res


def _check_call(c, res):
    """every batch of the call against the plain run of that batch alone"""
    from tclip_amd import engine
    N, stops = c["N"], c["stops"]
    assert res.outer_iters.tolist() == stops
    assert len(set(stops)) >= 2 and min(stops) < c["iters"]
    for b, s in enumerate(stops):
        sl = slice(b * N, (b + 1) * N)
        plain = _call(engine, c["x_q"][sl], None if c["x_s"] is None else c["x_s"][sl], None if c["y_s"] is None else c["y_s"][sl],
                      iters=s, iter_mm=c["iter_mm"], lambd=c["lambd"])
        _check_batch(res, b, N, s, c["iters"], plain)
        quiet = res.changes[b, max(s - c["patience"], 0):s]
        assert (s == c["iters"] and bool(quiet.any())) or not quiet.any(), b


@pytest.mark.parametrize("name", ["two_groups", "one_group"])
def test_batches_stop_on_their_own(name):
    _check_call(*_synthetic(name))


def test_few_shot_rows_from_the_tables():
    """the same through run_em_dirichlet_tasks: few-shot, the rows read in place with a column permutation per task"""
    from tclip_amd import until_stable
    c = us.synthetic_case("few_shot")
    table_q, q_idx, table_s, s_idx, cols = us.as_tables(c["x_q"], c["x_s"], seed=5)
    kw = dict(patience=c["patience"], n_batches=len(c["specs"]), iters=c["iters"], iter_mm=c["iter_mm"], lambd=c["lambd"])
    res = until_stable.run_em_dirichlet_tasks(table_q.to(DEV), q_idx, table_s.to(DEV), s_idx, c["y_s"], cols, **kw)
    torch.cuda.synchronize()
    _check_call(c, res)
    dense = _call(until_stable, c["x_q"], c["x_s"], c["y_s"], **kw)
    for name in until_stable.UntilStableResult.__slots__:
        assert _same(getattr(res, name), getattr(dense, name)), name


# ---- 3. isolation, 4. determinism ----------------------------------------------------------------------------------------------
def test_a_stopped_batch_leaves_its_neighbour_alone():
    from tclip_amd import engine
    c, res = _synthetic("isolation")
    N, iters = c["N"], c["iters"]
    assert res.outer_iters.tolist() == c["stops"] and c["stops"][0] < iters == c["stops"][-1]
    full = _call(engine, c["x_q"][N:], None, None, iters=iters, iter_mm=c["iter_mm"], lambd=c["lambd"])
    _check_batch(res, 1, N, iters, iters, full)
    _check_call(c, res)


@pytest.mark.parametrize("name", ["two_groups", "one_group"])
def test_two_calls_return_equal_bits(name):
    from tclip_amd import until_stable
    c, first = _synthetic(name)
    again = _call(until_stable, c["x_q"], None, None, patience=c["patience"], n_batches=len(c["specs"]), iters=c["iters"],
                  iter_mm=c["iter_mm"], lambd=c["lambd"])
    for key in until_stable.UntilStableResult.__slots__:
        assert _same(getattr(first, key), getattr(again, key)), key


# ---- 5. classes and evaluators ---------------------------------------------------------------------------------------------------
def _eval_args(shots, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=12, iter_mm=120, num_classes_test=20, n_class=20, n_query=75, k_eff=5, T=30, shots=shots,
                use_softmax_feature=True, graph_matching=True, name_method="EM_DIRICHLET", number_tasks=6, batch_size=2,
                used_test_set="test", dataset="synthetic", tunable=False)
    a.update(kw)
    return a


def test_zero_shot_evaluator():
    from src.eval_zero_shot import Evaluator_zero_shot
    from tclip_amd import engine, synth, until_stable
    K = 20
    feats, labels = synth.make_feature_table(K, 30, seed=3)
    ev = Evaluator_zero_shot(device=torch.device(DEV), args=_eval_args(0, stop_patience=2), log_file=None)
    torch.manual_seed(11)
    np.random.seed(11)
    idx = ev.sample_indices(labels.numpy())
    B, N, Q = idx.shape
    ev.evaluate_tasks(None, feats, labels, indices=idx)
    x_q = feats[idx.reshape(-1)].view(B * N, Q, K)
    y_q = labels[idx.reshape(-1)].view(B * N, Q)
    kw = dict(n_batches=B, iters=12, iter_mm=120, lambd=int(K / 5) * Q)
    res = _call(until_stable, x_q, None, None, patience=2, **kw)
    outer = res.outer_iters.cpu().numpy()
    assert outer.min() < 12, "no batch of this case stops early: the test would show nothing"
    assert np.array_equal(ev.last_batch_outer_iters, outer) and ev.last_batch_outer_iters.shape == (B,)
    acc, _ = engine.clustering_accuracy(x_q.to(DEV), res.preds, y_q, graph_matching=True)
    assert np.array_equal(ev.last_task_accuracies, acc.numpy().reshape(B, N))
    m = ev.last_method
    assert np.array_equal(m.outer_iters, outer) and np.array_equal(m.assignment_changes, res.changes.cpu().numpy())
    assert np.array_equal(ev.last_batch_mm_iters, res.mm_iters.cpu().numpy())
    assert np.array_equal(ev.last_batch_criterions, res.criterions.cpu().numpy())
    assert len(m.timestamps) == 12 and np.asarray(m.criterions).shape == (12,)          # the logs keep their shapes
    # without the option: today's run
    ev0 = Evaluator_zero_shot(device=torch.device(DEV), args=_eval_args(0), log_file=None)
    ev0.evaluate_tasks(None, feats, labels, indices=idx)
    plain = _call(engine, x_q, None, None, **kw)
    acc0, _ = engine.clustering_accuracy(x_q.to(DEV), plain.preds, y_q, graph_matching=True)
    assert np.array_equal(ev0.last_task_accuracies, acc0.numpy().reshape(B, N))
    assert np.array_equal(ev0.last_batch_mm_iters, plain.mm_iters.cpu().numpy())
    assert not hasattr(ev0, "last_batch_outer_iters") and not hasattr(ev0.last_method, "outer_iters")


def test_few_shot_evaluator():
    """tables in place: the class reads its task rows through the index tensors"""
    from src.eval_few_shot import Evaluator_few_shot
    from tclip_amd import engine, synth, until_stable
    K = 20
    feats_s, labels_s = synth.make_feature_table(K, 12, seed=4)
    feats_q, labels_q = synth.make_feature_table(K, 30, seed=5)
    ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(2, stop_patience=1), log_file=None)
    torch.manual_seed(12)
    np.random.seed(12)
    indices = ev.sample_indices(labels_s.numpy(), labels_q.numpy())
    ev.evaluate_tasks(None, feats_s, labels_s, feats_q, labels_q, indices=indices)
    t = ev._tasks(feats_s, labels_s, feats_q, labels_q, indices)
    si, qi, _, _, rel = ev._block(t)
    assert rel is not None and ev.last_method.rows_in_place(ev.args)
    cols, y_s, y_q = rel
    tab_s, tab_q = t.tables()
    kw = dict(n_batches=t.n_batches, iters=12, iter_mm=120, lambd=int(K / 5) * t.Q)
    res = until_stable.run_em_dirichlet_tasks(tab_q, qi, tab_s, si, y_s, cols, patience=1, **kw)
    torch.cuda.synchronize()
    outer = res.outer_iters.cpu().numpy()
    assert outer.min() < 12, "no batch of this case stops early: the test would show nothing"
    assert np.array_equal(ev.last_batch_outer_iters, outer)
    acc = (res.preds.cpu().long() == y_q.cpu()).float().mean(1).numpy().reshape(t.n_batches, t.N)
    assert np.array_equal(ev.last_task_accuracies, acc)
    assert np.array_equal(ev.last_batch_mm_iters, res.mm_iters.cpu().numpy())
    # without the option: today's run
    ev0 = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(2), log_file=None)
    ev0.evaluate_tasks(None, feats_s, labels_s, feats_q, labels_q, indices=indices)
    plain = engine.run_em_dirichlet_tasks(tab_q, qi, tab_s, si, y_s, cols, **kw)
    acc0 = (plain.preds.cpu().long() == y_q.cpu()).float().mean(1).numpy().reshape(t.n_batches, t.N)
    assert np.array_equal(ev0.last_task_accuracies, acc0)
    assert np.array_equal(ev0.last_batch_mm_iters, plain.mm_iters.cpu().numpy())
    assert not hasattr(ev0, "last_batch_outer_iters")
