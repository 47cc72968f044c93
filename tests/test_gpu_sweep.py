"""GPU: the value sweeps of the four tunable few-shot methods (engine.sweep_*_tasks -> tclip_*_sweep_tasks).

The contract is equality of bits: slice p of every per-value output is what the single-value entry fed from the same tables
(run_*_tasks on probability features, run_*_visual_tasks on visual ones) returns for values[p]; LaplacianShot's unary term and
neighbour lists, which no value enters, are the single entry's.  Nothing here has a tolerance.

  - every method on both feature kinds at shapes that cross the wavefront (Q, K around 64), the 64-wide GEMM tile, several tasks
    and, for ALPHA_TIM, two batches in one call;
  - the ends of the reference's tuning grids (scripts/opt_parameters.sh) and one interior value; a repeated value, the list
    reversed, a list of one;
  - LaplacianShot with (value, task) pairs that freeze before the last update next to pairs that do not;
  - a random column permutation per task on probability features;
  - Evaluator_few_shot.evaluate_sweep against evaluate_tasks, and main_features' `sweep_values` against one run per value."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from helpers import visual_fs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (T, Q, K, shots, n_batches): one tiny task; odd sizes below a wavefront; K just past 64 with one shot; two batches
SHAPES = [(1, 3, 5, 1, 1), (3, 35, 37, 2, 1), (2, 75, 65, 1, 1), (2, 75, 100, 4, 2)]
KINDS = [0, 33, 512]                       # 0: probability features (rows of K elements, cols), else the embedding length
# the ends of the reference's grid and one value inside it
GRID = {"paddle": [0.0, 5.0, 100.0], "bdcspn": [1.0, 20.0, 60.0], "lshot": [1.0, 4.0, 9.0], "alpha_tim": [1.5, 3.5, 7.0]}


def same(a, b):
    """byte for byte, on the host: NaN payloads and the sign of zero count, whatever the dtype"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


_INPUTS = {}


def _inputs(T, Q, K, shots, dim):
    """(table_q, q_idx, table_s, s_idx, y_s, cols): seeded tables of 3 * shots + 2 rows per class, every class `shots` times in
    every support set in a shuffled order, random query rows with repeats, and on probability features a random column
    permutation per task.  Made once per shape and shared; nothing modifies them."""
    key = (T, Q, K, shots, dim)
    if key not in _INPUTS:
        from tclip_amd import synth
        seed = 5000 + 7 * T + 11 * Q + 13 * K + 17 * shots + dim
        per_class = 3 * shots + 2
        if dim:
            # embeddings of norm about 1: ALPHA_TIM's Alpha cross-entropy raises a probability to the power -alpha, and with
            # rows of norm 10 that probability underflows
            table_s, labels, table_q, _ = visual_fs.make_tables(K, dim, per_class, seed)
            table_s, table_q = table_s * 0.1, table_q * 0.1
        else:
            (table_s, labels), (table_q, _) = synth.make_feature_table(K, per_class, seed=seed), synth.make_feature_table(K, per_class, seed=seed + 1)
        gen = torch.Generator().manual_seed(seed)
        s_idx = torch.empty(T, K * shots, dtype=torch.int64)
        for t in range(T):
            rows = torch.cat([k * per_class + torch.randperm(per_class, generator=gen)[:shots] for k in range(K)])
            s_idx[t] = rows[torch.randperm(K * shots, generator=gen)]
        q_idx = torch.randint(0, K * per_class, (T, Q), generator=gen)
        y_s = torch.as_tensor(labels).long()[s_idx]
        cols = None if dim else torch.stack([torch.randperm(K, generator=gen) for _ in range(T)]).to(torch.int32)
        if cols is not None and K > 2:
            assert not torch.equal(cols[0], torch.arange(K - 1, -1, -1, dtype=torch.int32))      # not just the reversal
        _INPUTS[key] = (torch.as_tensor(table_q).float().to(DEV), q_idx, torch.as_tensor(table_s).float().to(DEV), s_idx, y_s, cols)
    return _INPUTS[key]


def _method(name):
    """(sweep, single on probability features, single on visual features, the swept keyword, outputs no value enters)"""
    from tclip_amd import engine
    return {"paddle": (engine.sweep_paddle_tasks, engine.run_paddle_tasks, engine.run_paddle_visual_tasks, "lambd", ()),
            "bdcspn": (engine.sweep_bdcspn_tasks, engine.run_bdcspn_tasks, engine.run_bdcspn_visual_tasks, "temp", ()),
            "lshot": (engine.sweep_laplacian_shot_tasks, engine.run_laplacian_shot_tasks, engine.run_laplacian_shot_visual_tasks,
                      "lmd", (0, 1)),
            "alpha_tim": (engine.sweep_alpha_tim_tasks, engine.run_alpha_tim_tasks, engine.run_alpha_tim_visual_tasks,
                          "alpha_value", ())}[name]


def _sweep(name, inp, K, dim, values, **kw):
    sweep = _method(name)[0]
    table_q, q_idx, table_s, s_idx, y_s, cols = inp
    return sweep(table_q, q_idx, table_s, s_idx, y_s, cols, values=values, n_class=K if dim else None, **kw)


def _single(name, inp, K, dim, value, **kw):
    _, prob, visual, attr, _ = _method(name)
    table_q, q_idx, table_s, s_idx, y_s, cols = inp
    if dim:
        return visual(table_q, q_idx, table_s, s_idx, y_s, n_class=K, **{attr: value}, **kw)
    return prob(table_q, q_idx, table_s, s_idx, y_s, cols, **{attr: value}, **kw)


def check_slices(name, inp, K, dim, values, what, **kw):
    """every slice of the sweep against the single-value call; returns the sweep's outputs"""
    once = _method(name)[4]
    out = _sweep(name, inp, K, dim, values, **kw)
    torch.cuda.synchronize()
    for p, v in enumerate(values):
        ref = _single(name, inp, K, dim, v, **kw)
        assert len(ref) == len(out)
        for i, (o, r) in enumerate(zip(out, ref)):
            got = o if i in once else o[p]
            assert got.shape == r.shape and (i in once or o.shape[0] == len(values)), (what, i, o.shape, r.shape)
            assert same(got, r), (what, "value", v, "output", i)
    return out


def _kw(name, Q, n_batches=1):
    if name == "paddle":
        return dict(iters=3)
    if name == "bdcspn":
        return dict()
    if name == "lshot":
        return dict(iters=20, knn=min(3, Q))
    return dict(iters=3, temp=15.0, lr=1e-3, loss_weights=[1.0, 0.7, 1.2], n_batches=n_batches)


# ---- 1. slice equality per method and feature kind ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim", KINDS)
@pytest.mark.parametrize("T,Q,K,shots,n_batches", SHAPES)
def test_paddle_slices_equal_single_calls(T, Q, K, shots, n_batches, dim):
    out = check_slices("paddle", _inputs(T, Q, K, shots, dim), K, dim, GRID["paddle"], (T, Q, K, shots, dim), **_kw("paddle", Q))
    P, D = 3, dim or K
    assert [tuple(o.shape) for o in out] == [(P, T, Q, K), (P, T, K), (P, T, K, D), (P, T, Q)]
    assert not torch.equal(out[0][0], out[0][2])                       # lambd does change the result


@pytest.mark.parametrize("norm_type", ["UN", "L2N", "CL2N"])
@pytest.mark.parametrize("dim", KINDS)
@pytest.mark.parametrize("T,Q,K,shots,n_batches", SHAPES)
def test_bdcspn_slices_equal_single_calls(T, Q, K, shots, n_batches, dim, norm_type):
    out = check_slices("bdcspn", _inputs(T, Q, K, shots, dim), K, dim, GRID["bdcspn"], (T, Q, K, shots, dim, norm_type),
                       norm_type=norm_type)
    P, D = 3, dim or K
    assert [tuple(o.shape) for o in out] == [(P, T, K, D), (P, T, Q, K), (P, T, Q)]
    assert not torch.equal(out[1][0], out[1][2])


@pytest.mark.parametrize("dim", KINDS)
@pytest.mark.parametrize("T,Q,K,shots,n_batches", SHAPES)
def test_laplacian_shot_slices_equal_single_calls(T, Q, K, shots, n_batches, dim):
    kw = _kw("lshot", Q)
    out = check_slices("lshot", _inputs(T, Q, K, shots, dim), K, dim, GRID["lshot"], (T, Q, K, shots, dim), **kw)
    assert [tuple(o.shape) for o in out] == [(T, Q, K), (T, Q, kw["knn"] - 1), (3, T, 20, Q), (3, T, 20)]


@pytest.mark.parametrize("dim", [0, 33])
@pytest.mark.parametrize("Q,knn", [(129, 7), (75, 75)])
def test_laplacian_shot_wide_graphs(Q, knn, dim):
    """more than two wavefront passes over the queries with knn = 7, and every other query a neighbour (knn = Q: the largest
    lists, 75 * 74 words of LDS)"""
    T, K, shots = 2, 37, 2
    out = check_slices("lshot", _inputs(T, Q, K, shots, dim), K, dim, GRID["lshot"], (Q, knn, dim), iters=20, knn=knn)
    assert out[1].shape == (T, Q, knn - 1)
    nbr = out[1].cpu()
    assert int(nbr.min()) >= 0 and int(nbr.max()) < Q and not bool((nbr == torch.arange(Q).view(1, Q, 1)).any())


@pytest.mark.parametrize("entropies", [("Shannon", "Alpha", "Alpha"), ("Alpha", "Alpha", "Alpha")])
@pytest.mark.parametrize("dim", KINDS)
@pytest.mark.parametrize("T,Q,K,shots,n_batches", SHAPES)
def test_alpha_tim_slices_equal_single_calls(T, Q, K, shots, n_batches, dim, entropies):
    kw = _kw("alpha_tim", Q, n_batches)
    out = check_slices("alpha_tim", _inputs(T, Q, K, shots, dim), K, dim, GRID["alpha_tim"], (T, Q, K, shots, dim, entropies),
                       entropies=entropies, **kw)
    P, D = 3, dim or K
    assert [tuple(o.shape) for o in out] == [(P, T, K, D), (P, T, Q, K), (P, T, Q), (P, n_batches, 3)]
    # (no "another alpha, another result" here: Adam's first steps are nearly sign steps, two alphas may give the same weights)
    assert all(bool(torch.isfinite(o.float()).all()) for o in out)
    if n_batches == 2:                      # a criterion is one batch's, within one value
        assert not torch.equal(out[3][0, 0], out[3][0, 1])


# ---- 2. the list of values ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["paddle", "bdcspn", "lshot", "alpha_tim"])
def test_repeated_reversed_and_single_values(name):
    T, Q, K, shots, dim = 3, 35, 37, 2, 0
    inp, kw = _inputs(T, Q, K, shots, dim), _kw(name, Q)
    once = _method(name)[4]
    a, b, c = GRID[name]
    values = [a, b, a, c]
    out = check_slices(name, inp, K, dim, values, name, **kw)
    per_value = [o for i, o in enumerate(out) if i not in once]
    assert all(same(o[0], o[2]) for o in per_value)                    # the repeated value: the same bits twice
    assert any(not torch.equal(o[0], o[3]) for o in per_value)         # and another value: other results
    rev = _sweep(name, inp, K, dim, values[::-1], **kw)
    for i, (o, r) in enumerate(zip(out, rev)):
        assert same(o, r) if i in once else same(o, r.flip(0)), (name, "reversed", i)
    one = _sweep(name, inp, K, dim, [b], **kw)
    ref = _single(name, inp, K, dim, b, **kw)
    for i, (o, r) in enumerate(zip(one, ref)):
        assert same(o if i in once else o[0], r) and (i in once or o.shape[0] == 1), (name, "one value", i)
    # an integer in the list is the float of the single call
    if name == "lshot":
        assert same(_sweep(name, inp, K, dim, [4], **kw)[3][0], _single(name, inp, K, dim, 4.0, **kw)[3])


# ---- 3. LaplacianShot: frozen and running (value, task) pairs in one call ---------------------------------------------------

def test_laplacian_shot_freezes_per_value_and_task():
    """The freeze rule stops a solve once its energy moves by less than 1e-6 of itself; the remaining entries repeat the last
    update.  Small lmd values settle within a few updates, large ones keep moving: both kinds of (value, task) pairs share this
    call, so the tail fill runs for some blocks of the grid and not for others."""
    T, Q, K, shots, dim = 3, 35, 37, 2, 0
    values = [0.05, 1.0, 9.0, 60.0]
    out = check_slices("lshot", _inputs(T, Q, K, shots, dim), K, dim, values, "freeze", iters=20, knn=3)
    energies, preds_iter = out[3].cpu(), out[2].cpu()
    frozen = energies[:, :, -1] == energies[:, :, -2]                  # [P, T]: the last entry is a copy of the one before it
    print("first repeated update per (value, task):",
          [[int((energies[p, t, 1:] == energies[p, t, :-1]).float().argmax()) + 1 if bool(frozen[p, t]) else None for t in range(T)]
           for p in range(len(values))])
    assert bool(frozen.any()) and bool((~frozen).any()), frozen
    for p, t in frozen.nonzero().tolist():
        assert torch.equal(preds_iter[p, t, -1], preds_iter[p, t, -2])


# ---- 4. the evaluator and the command line ------------------------------------------------------------------------------------

EVAL_VALUES = {"PADDLE": [0.0, 5.0, 100.0], "BDCSPN": [1.0, 20.0, 60.0], "LAPLACIAN_SHOT": [1.0, 4.0, 9.0], "ALPHA_TIM": [1.5, 3.5, 7.0]}
EVAL_CASES = [("PADDLE", False), ("PADDLE", True), ("BDCSPN", False), ("BDCSPN", True), ("LAPLACIAN_SHOT", False), ("ALPHA_TIM", False)]
_TABLES = {}


def _eval_args(method, K, visual, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=5, num_classes_test=K, n_class=K, n_query=15, k_eff=5, T=30.0, use_softmax_feature=not visual,
                name_method=method, lambd=5.0, temp=15.0, norm_type="L2N", knn=3, lmd=0.7, loss_weights=[1.0, 1.0, 1.0],
                lr_alpha_tim=1e-3, entropies=["Shannon", "Alpha", "Alpha"], alpha_value=3.0, number_tasks=4, batch_size=2, shots=2,
                used_test_set="val", dataset="synthetic", tunable=True)
    a.update(kw)
    return a


def _tables(visual):
    """tiny seeded tables (K = 10) and one draw of task indices, made once and shared"""
    if visual not in _TABLES:
        from src.eval_few_shot import Evaluator_few_shot
        from tclip_amd import synth
        K, seed = 10, 9100
        if visual:
            tabs = visual_fs.make_tables(K, 96, 12, seed, signal=0.3)
        else:
            tabs = synth.make_feature_table(K, 12, seed=seed) + synth.make_feature_table(K, 12, seed=seed + 1)
        random.seed(seed)
        torch.manual_seed(seed)
        np.random.seed(seed)
        ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args("PADDLE", K, visual), log_file=None)
        s_idx, q_idx = ev.sample_indices(np.asarray(tabs[1]), np.asarray(tabs[3]))
        assert s_idx.shape == (2, 2, K * 2) and q_idx.shape == (2, 2, 15)
        _TABLES[visual] = (K, tabs, (s_idx, q_idx))
    return _TABLES[visual]


@pytest.mark.parametrize("method,visual", EVAL_CASES)
def test_evaluate_sweep_equals_evaluate_tasks(method, visual, monkeypatch):
    from src import eval_few_shot
    from src.eval_few_shot import Evaluator_few_shot
    K, tabs, indices = _tables(visual)
    values, attr = EVAL_VALUES[method], Evaluator_few_shot._TUNED[method]
    ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(method, K, visual), log_file=None)
    accs, mean_time = ev.evaluate_sweep(None, *tabs, values=values, indices=indices)
    assert accs.shape == (3,) and mean_time > 0 and ev.args[attr] == _eval_args(method, K, visual)[attr]
    assert [getattr(m, attr) for m in ev.last_methods] == values
    want = []
    for p, v in enumerate(values):
        one = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(method, K, visual, **{attr: v}), log_file=None)
        acc, _ = one.evaluate_tasks(None, *tabs, indices=indices)
        want.append(acc)
        assert accs[p] == acc, (method, v, accs[p], acc)
        assert np.array_equal(one.last_method.preds.cpu().numpy().reshape(-1), ev.last_methods[p].preds.cpu().numpy().reshape(-1))
    assert 0 < min(want) and max(want) <= 1
    # a support set that misses a class: ordinary runs, value after value, with the same result
    if not visual:
        monkeypatch.setattr(eval_few_shot, "relabel_indices", lambda *a, **k: None)
        again, _ = ev.evaluate_sweep(None, *tabs, values=values, indices=indices)
        assert np.array_equal(again, accs)


@pytest.mark.parametrize("method,visual", [("LAPLACIAN_SHOT", True), ("ALPHA_TIM", True)])
def test_classes_still_refuse_visual_features(method, visual):
    from src.eval_few_shot import Evaluator_few_shot
    K, tabs, indices = _tables(visual)
    ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(method, K, visual), log_file=None)
    with pytest.raises(NotImplementedError, match="probability features"):
        ev.evaluate_sweep(None, *tabs, values=EVAL_VALUES[method], indices=indices)


@pytest.mark.parametrize("method,visual", EVAL_CASES)
def test_main_features_sweep_file_equals_separate_runs(method, visual, tmp_path):
    from tclip_amd import features
    sys.path.insert(0, PKG)
    import main_features
    K, tabs, _ = _tables(visual)
    name = {"PADDLE": "paddle", "BDCSPN": "bdcspn", "LAPLACIAN_SHOT": "laplacian_shot", "ALPHA_TIM": "alpha_tim"}[method]
    attr = {"PADDLE": "lambd", "BDCSPN": "temp", "LAPLACIAN_SHOT": "lmd", "ALPHA_TIM": "alpha_value"}[method]
    values = EVAL_VALUES[method]
    files = []
    for root in (tmp_path / "one_call", tmp_path / "separate"):
        d = root / "data" / "synthetic" / "saved_features"
        d.mkdir(parents=True)
        stem = "visual_RN50" if visual else "softmax_RN50_T30"
        features.save_features(str(d / f"train_{stem}.plk"), tabs[0], tabs[1])
        features.save_features(str(d / f"val_{stem}.plk"), tabs[2], tabs[3])
        common = ["--results-root", str(root), "--opts", "method", name, "use_softmax_feature", str(not visual), "shots", "2",
                  "number_tasks", "4", "batch_size", "2", "n_query", "15", "dataset", "synthetic", "seed", "3", "used_test_set", "val"]
        if method == "ALPHA_TIM":
            common += ["iter", "5"]
        if root.name == "one_call":
            accs, _, path = main_features.main(common + ["sweep_values", str(values)])
            assert len(accs) == 3
        else:
            for v in values:
                _, _, path = main_features.main(common + [attr, str(v)])
        files.append(path)
    word = "_visual" if visual else "_softmax"
    assert files[0].endswith(os.path.join("results_few_shot", "val", "synthetic", f"{method}{word}_s2.txt"))
    one_call, separate = open(files[0], "rb").read(), open(files[1], "rb").read()
    assert one_call == separate
    rows = one_call.decode().splitlines()
    assert rows[0] == "val_param\tacc" and [r.split("\t")[0] for r in rows[1:]] == [str(v) for v in values]
