"""GPU: TIM_GD and ALPHA_TIM reading their task rows from the feature tables in place, in every Adam step.

  - engine.run_tim_gd_tasks / run_alpha_tim[_visual]_tasks against the dense entries fed `table[idx][..., cols]`, every output
    compared byte for byte, at the shapes where the GEMMs and TimRows::row change path (the 64-wide tile edge, the depth-16 slice
    edge, the multiple-of-4 condition of the 128-bit loads, the S / S + Q seam);
  - the reference-made fixtures through the in-place entries (rows embedded in a larger shuffled table, on probability features
    with inverse-permuted columns): bit-equal to the dense entry on the fixture's own tensors, and what the dense fixture tests
    assert;
  - Evaluator_few_shot.evaluate_tasks: `in_place_loop`, the default route, materialise_tasks and batches_per_call agree, and no
    task tensor is built under the option;
  - the memory of one in-place TIM_GD call against its workspace query and against the dense call;
  - out-of-range indices and columns raise IndexError from the binding.
5 Adam steps unless a fixture says otherwise.  Nothing here skips: a missing fixture fails."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_names
from helpers import alpha_tim, tim_gd, visual_fs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = ("weights", "logits_q", "preds", "criterions")
ITERS = 5


def same(a, b):
    """byte for byte, on the host: NaN payloads and the sign of zero count, whatever the dtype"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def assert_same(tasks, dense, what):
    for name, a, b in zip(OUT, tasks, dense):
        assert torch.equal(a.cpu(), b.cpu()) and same(a, b), (name, what)


# ---- 1. in place equals dense --------------------------------------------------------------------------------------------

def _labels(T, S, K, gen):
    """every class present (no class mean is 0/0), the rest at random (unequal class counts), shuffled per task: not class-sorted"""
    assert S >= K
    out = []
    for _ in range(T):
        y = torch.cat([torch.arange(K), torch.randint(0, K, (S - K,), generator=gen)])
        out.append(y[torch.randperm(S, generator=gen)])
    return torch.stack(out)


def _inputs(D, K, S, Q, softmax, seed, T=3):
    """tables of about three times the rows used, shuffled support indices with repeats, a random per-task column permutation
    on probability features; (x_q, x_s): what the dense side is fed, `table[idx][..., cols]` by torch's own indexing"""
    gen = torch.Generator().manual_seed(seed)
    rows_s, rows_q = 3 * S + 2, 3 * Q
    table_s, table_q = torch.randn(rows_s, D, generator=gen), torch.randn(rows_q, D, generator=gen)
    if softmax:
        table_s, table_q = (table_s * 3).softmax(-1), (table_q * 3).softmax(-1)
    else:
        table_s, table_q = table_s * (2.0 / D ** 0.5), table_q * (2.0 / D ** 0.5)
    s_idx = torch.stack([torch.randperm(rows_s, generator=gen)[:S] for _ in range(T)])
    for t in range(T):
        for j in range(0, S - 1, 3):
            s_idx[t, j + 1] = s_idx[t, j]                              # repeated support indices
    q_idx = torch.randint(0, rows_q, (T, Q), generator=gen)
    cols = torch.stack([torch.randperm(D, generator=gen) for _ in range(T)]).to(torch.int32) if softmax else None
    table_s, table_q = table_s.to(DEV), table_q.to(DEV)
    x_s, x_q = table_s[s_idx.to(DEV)], table_q[q_idx.to(DEV)]
    if cols is not None:
        take = cols.long().to(DEV).unsqueeze(1)
        x_s, x_q = torch.gather(x_s, 2, take.expand(T, S, D)), torch.gather(x_q, 2, take.expand(T, Q, D))
    return table_q, q_idx, table_s, s_idx, _labels(T, S, K, gen), cols, x_q.contiguous(), x_s.contiguous()


SOFTMAX_SHAPES = [(K, shots, Q) for K in (5, 37, 68) for shots in (1, 3) for Q in (10, 75)]
# (D, K, S, Q); the last: R = 138, both GEMMs run interior tiles on the 128-bit path and partial edge tiles
VISUAL_SHAPES = [(1, 4, 4, 10), (5, 4, 8, 10), (33, 10, 20, 75), (64, 10, 10, 75), (130, 37, 37, 75), (128, 64, 128, 10)]
GD = dict(temp=15.0, lr=1e-3, loss_weights=[1.0, 0.7, 1.2])
ALPHA = dict(temp=15.0, lr=1e-3, alpha_value=3.0, loss_weights=[1.0, 0.7, 1.2])
ENTROPIES = (("Shannon", "Alpha", "Alpha"), ("Shannon", "Shannon", "Shannon"))


@pytest.mark.parametrize("K,shots,Q", SOFTMAX_SHAPES)
def test_tim_gd_in_place_equals_dense_probability_features(K, shots, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, cols, x_q, x_s = _inputs(K, K, K * shots, Q, True, K * 1000 + shots * 7 + Q)
    dense = engine.run_tim_gd(x_q, x_s, y_s.to(DEV), n_class=K, iters=ITERS, **GD)
    assert bool(torch.isfinite(dense[0]).all()) and bool((dense[3] > 0).all())
    for on_device in (False, True):                                    # index tensors from the host and from the device
        to = (lambda t: t.to(DEV)) if on_device else (lambda t: t)
        tasks = engine.run_tim_gd_tasks(table_q, to(q_idx), table_s, to(s_idx), y_s, to(cols), n_class=K, iters=ITERS, **GD)
        assert_same(tasks, dense, on_device)
    # without cols: the tables' own column order (at K = 68 the 128-bit path of the interior tiles)
    dense = engine.run_tim_gd(table_q[q_idx.to(DEV)], table_s[s_idx.to(DEV)], y_s.to(DEV), n_class=K, iters=ITERS, **GD)
    assert_same(engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, n_class=K, iters=ITERS, **GD), dense, "no cols")


@pytest.mark.parametrize("K,shots,Q", SOFTMAX_SHAPES)
def test_alpha_tim_in_place_equals_dense_probability_features(K, shots, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, cols, x_q, x_s = _inputs(K, K, K * shots, Q, True, K * 1000 + shots * 7 + Q + 1)
    for i, ent in enumerate(ENTROPIES):
        dense = engine.run_alpha_tim(x_q, x_s, y_s.to(DEV), iters=ITERS, entropies=ent, **ALPHA)
        assert bool(torch.isfinite(dense[0]).all())
        to = (lambda t: t.to(DEV)) if i else (lambda t: t)
        tasks = engine.run_alpha_tim_tasks(table_q, to(q_idx), table_s, to(s_idx), y_s, to(cols), iters=ITERS, entropies=ent, **ALPHA)
        assert_same(tasks, dense, ent)


def test_two_batches_in_one_call():
    """T = 4 in two batches: ALPHA_TIM's criterion is per batch, TIM_GD's per task"""
    from tclip_amd import engine
    K = 37
    table_q, q_idx, table_s, s_idx, y_s, cols, x_q, x_s = _inputs(K, K, 2 * K, 75, True, 4242, T=4)
    dense = engine.run_alpha_tim(x_q, x_s, y_s.to(DEV), iters=ITERS, n_batches=2, **ALPHA)
    tasks = engine.run_alpha_tim_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=ITERS, n_batches=2, **ALPHA)
    assert tasks[3].shape == (2, ITERS) and not torch.equal(tasks[3][0], tasks[3][1])
    assert_same(tasks, dense, "ALPHA_TIM")
    dense = engine.run_tim_gd(x_q, x_s, y_s.to(DEV), n_class=K, iters=ITERS, n_batches=2, **GD)
    tasks = engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, n_class=K, iters=ITERS, n_batches=2, **GD)
    assert tasks[3].shape == (ITERS, 4)
    assert_same(tasks, dense, "TIM_GD")
    with pytest.raises(ValueError, match="multiple of n_batches"):
        engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, n_class=K, iters=ITERS, n_batches=3, **GD)


@pytest.mark.parametrize("D,K,S,Q", VISUAL_SHAPES)
def test_tim_gd_in_place_equals_dense_visual_features(D, K, S, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, _, x_q, x_s = _inputs(D, K, S, Q, False, D * 1009 + K * 13 + S)
    dense = engine.run_tim_gd(x_q, x_s, y_s.to(DEV), n_class=K, iters=ITERS, **GD)
    assert dense[0].shape == (3, K, D) and bool(torch.isfinite(dense[0]).all())
    assert_same(engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx.to(DEV), y_s, n_class=K, iters=ITERS, **GD), dense, "aligned")
    if D % 4 == 0:
        # tables that are views at an odd offset: 4-byte aligned only, the interior tiles leave the 128-bit path
        odd_q, odd_s = (torch.empty(t.numel() + 1, device=DEV)[1:].view(t.shape).copy_(t) for t in (table_q, table_s))
        assert odd_q.data_ptr() % 16 == 4 and odd_s.data_ptr() % 16 == 4 and odd_q.is_contiguous()
        assert_same(engine.run_tim_gd_tasks(odd_q, q_idx, odd_s, s_idx, y_s, n_class=K, iters=ITERS, **GD), dense, "odd offset")
    with pytest.raises(ValueError, match="cols"):                       # no column permutation on visual features
        engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, torch.zeros(3, D, dtype=torch.int32), n_class=K, iters=ITERS, **GD)


@pytest.mark.parametrize("D,K,S,Q", [VISUAL_SHAPES[2], VISUAL_SHAPES[5]])
def test_alpha_tim_in_place_equals_dense_visual_features(D, K, S, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, _, x_q, x_s = _inputs(D, K, S, Q, False, D * 1009 + K * 13 + S + 1)
    for ent in ENTROPIES:
        dense = engine.run_alpha_tim_visual(x_q, x_s, y_s.to(DEV), n_class=K, iters=ITERS, entropies=ent, **ALPHA)
        tasks = engine.run_alpha_tim_visual_tasks(table_q, q_idx.to(DEV), table_s, s_idx, y_s, n_class=K, iters=ITERS, entropies=ent, **ALPHA)
        assert_same(tasks, dense, ent)


# ---- 2. the reference's fixtures through the in-place entries -------------------------------------------------------------

def _embed(x, gen, inverse_of=None):
    """(table, idx): the rows of x (T, R, W) at shuffled positions of a table three times as long (the other rows hold noise), so
    that table[idx] == x; with `inverse_of` (T, W) column permutations the columns are stored inverse-permuted, so that
    table[idx[t]][:, inverse_of[t]] == x[t]."""
    n, R, W = x.shape
    pos = torch.randperm(3 * n * R + 3, generator=gen)[:n * R].view(n, R)
    table = torch.randn(3 * n * R + 3, W, generator=gen)
    if inverse_of is not None:
        stored = torch.empty_like(x)
        stored.scatter_(2, inverse_of.long().unsqueeze(1).expand(n, R, W), x)          # stored[t, r, cols[t, d]] = x[t, r, d]
        x = stored
    table[pos.reshape(-1)] = x.reshape(n * R, W)
    return table, pos


def _embedded(g, permute):
    x_s, x_q = torch.from_numpy(g["x_s"]), torch.from_numpy(g["x_q"])
    gen = torch.Generator().manual_seed(int(g["K"]))
    cols = torch.stack([torch.randperm(x_q.shape[2], generator=gen) for _ in range(x_q.shape[0])]).to(torch.int32) if permute else None
    table_s, s_idx = _embed(x_s, gen, inverse_of=cols)
    table_q, q_idx = _embed(x_q, gen, inverse_of=cols)
    return dict(table_s=table_s.to(DEV), s_idx=s_idx, table_q=table_q.to(DEV), q_idx=q_idx, cols=cols)


ALPHA_FIX = ["fs_tim_K100_N3_s2", "fs_tim_K10_N3_s1_shannon", "fs_tim_K10_N4_s4", "fs_tim_K37_N2_s3_a2", "fs_tim_K37_N3_s2",
             "fs_tim_K397_N1_s1", "fs_tim_K5_N3_s2"]
ALPHA_BOUNDS = json.load(open(os.path.join(GOLDEN, "f4_tolerances.json")))["alpha_tim"]


def test_every_fixture_is_listed():
    assert sorted(ALPHA_FIX) == golden_names("fs_tim_") and sorted(tim_gd.PROB) == golden_names("fs_gd_tim_")
    assert sorted(tim_gd.VISUAL) == golden_names("fs_vis_gd_tim_") and sorted(alpha_tim.VISUAL) == golden_names("fs_vis_alpha_tim_")


@pytest.mark.parametrize("name", ALPHA_FIX)
def test_alpha_tim_probability_fixture_in_place(name):
    """what tests/test_alpha_tim.py::test_engine_matches_reference asserts, through ALPHA_TIM.run_tables"""
    from src.methods.few_shot.tim import ALPHA_TIM
    from src.utils import CfgNode
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K, prm = int(g["K"]), alpha_tim.params(g)
    a = CfgNode(iter=prm["iters"], num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, shots=int(g["shots"]),
                use_softmax_feature=True, temp=prm["temp"], loss_weights=prm["loss_weights"], lr_alpha_tim=prm["lr"],
                entropies=prm["entropies"], alpha_value=prm["alpha_value"])
    m = ALPHA_TIM(model=None, device=torch.device(DEV), log_file=None, args=a)
    y_s, y_q = torch.from_numpy(g["y_s"]).squeeze(2), torch.from_numpy(g["y_q"]).squeeze(2)
    m.run_tables(**_embedded(g, True), y_s=y_s.to(DEV), y_q=y_q.to(DEV))
    logs = m.get_logs()
    dense = engine.run_alpha_tim(torch.from_numpy(g["x_q"]).to(DEV), torch.from_numpy(g["x_s"]).to(DEV), y_s.to(DEV), **prm)
    assert_same((m.weights, m.logits_q, m.preds, torch.from_numpy(m.criterions_per_batch)), dense, name)
    b = ALPHA_BOUNDS[name]
    assert np.abs(m.weights.cpu().numpy() - g["weights"]).max() <= b["weights_abs"]
    assert np.abs(m.logits_q.cpu().numpy() - g["logits_q"]).max() <= b["logits_abs"]
    assert logs["criterions"].shape == g["criterions"].shape and logs["acc"].shape == g["acc"].shape
    assert np.abs(logs["criterions"] / g["criterions"] - 1).max() <= b["criterions_rel"]
    assert np.array_equal(m.preds.cpu().numpy(), g["logits_q"].argmax(2)), "predictions differ from the reference's"
    assert np.array_equal(logs["acc"], g["acc"]), "accuracies differ from the reference's"


@pytest.mark.parametrize("name", tim_gd.PROB + tim_gd.VISUAL)
def test_tim_gd_fixture_in_place(name):
    """what tests/test_gpu_tim_gd.py::test_fixture_drop_in asserts, through TIM_GD.run_tables"""
    from src.methods.few_shot.tim import TIM_GD
    from src.utils import CfgNode
    from tclip_amd import engine
    g = tim_gd.load_fixture(GOLDEN, name)
    K, prm, softmax = int(g["K"]), tim_gd.params(g), name in tim_gd.PROB
    a = CfgNode(iter=prm["iters"], num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, use_softmax_feature=softmax,
                temp=prm["temp"], loss_weights=prm["loss_weights"], lr_tim=prm["lr"], name_method="TIM-GD", shots=int(g["shots"]))
    m = TIM_GD(model=None, device=torch.device(DEV), log_file=None, args=a)
    N = g["x_q"].shape[0]
    y_s, y_q = torch.from_numpy(g["y_s"]).reshape(N, -1), torch.from_numpy(g["y_q"]).reshape(N, -1)
    m.run_tables(**_embedded(g, softmax), y_s=y_s.to(DEV), y_q=y_q.to(DEV))
    logs = m.get_logs()
    dense = engine.run_tim_gd(torch.from_numpy(g["x_q"]).to(DEV), torch.from_numpy(g["x_s"]).to(DEV), y_s.to(DEV), n_class=K, **prm)
    assert_same((m.weights, m.logits_q, m.preds, torch.from_numpy(m.criterions_per_task)), dense, name)
    assert logs["criterions"].shape == g["criterions"].shape and logs["acc"].shape == g["acc"].shape
    tim_gd.check_within_bounds(m.weights.cpu().numpy(), m.logits_q.cpu().numpy(), logs["criterions"], g)
    assert np.array_equal(m.preds.cpu().numpy(), g["logits_q"].argmax(2)), "predictions differ from the reference's"
    assert np.array_equal(logs["acc"], g["acc"]), "accuracies differ from the reference's"


@pytest.mark.parametrize("name", alpha_tim.VISUAL)
def test_alpha_tim_visual_fixture_in_place(name):
    """what tests/test_gpu_visual_alpha_tim.py::test_fixture asserts, through engine.run_alpha_tim_visual_tasks"""
    from tclip_amd import engine
    g = alpha_tim.load_fixture(GOLDEN, name)
    K, prm = int(g["K"]), alpha_tim.params(g)
    y_s = torch.from_numpy(g["y_s"]).reshape(g["x_s"].shape[0], -1)
    e = _embedded(g, False)
    out = engine.run_alpha_tim_visual_tasks(e["table_q"], e["q_idx"], e["table_s"], e["s_idx"], y_s, n_class=K, **prm)
    dense = engine.run_alpha_tim_visual(torch.from_numpy(g["x_q"]).to(DEV), torch.from_numpy(g["x_s"]).to(DEV), y_s.to(DEV), n_class=K, **prm)
    assert_same(out, dense, name)
    w, lq, preds, crit = out
    assert w.shape == g["weights"].shape and lq.shape == g["logits_q"].shape and crit.shape == (1, int(g["iters"]))
    assert float(np.abs(w.cpu().numpy() - g["weights"]).max()) <= float(g["weights_abs"])
    assert float(np.abs(lq.cpu().numpy() - g["logits_q"]).max()) <= float(g["logits_abs"])
    assert float(np.abs(crit[0].cpu().numpy() / g["criterions"] - 1).max()) <= float(g["criterions_rel"])
    assert np.array_equal(preds.cpu().numpy(), g["logits_q"].argmax(2)), "predictions differ from the reference's"
    acc = (preds.cpu().long() == torch.from_numpy(g["y_q"])).float().mean(1, keepdim=True).numpy()
    assert np.array_equal(acc, g["acc"]), "accuracies differ from the reference's"


# ---- 3. the evaluator's routes ----------------------------------------------------------------------------------------------

def _eval_args(method, K, visual, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=10, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=not visual,
                name_method=method, lambd=5.0, temp=15.0, norm_type="L2N", knn=3, lmd=0.7, loss_weights=[1.0, 0.3, 1.0],
                lr_tim=1e-3, lr_alpha_tim=1e-3, entropies=["Shannon", "Alpha", "Alpha"], alpha_value=3.0, number_tasks=6,
                batch_size=3, shots=2, used_test_set="test", dataset="synthetic", tunable=False)
    a.update(kw)
    return a


_TABLES = {}


def _tables(visual):
    """the seeded tables and one draw of task indices, made once and shared (never modified)"""
    if visual not in _TABLES:
        from src.eval_few_shot import Evaluator_few_shot
        from tclip_amd import synth
        K, seed = 10, 8200
        if visual:
            tabs = visual_fs.make_tables(K, 96, 40, seed, signal=0.3)
        else:
            tabs = synth.make_feature_table(K, 40, seed=seed) + synth.make_feature_table(K, 40, seed=seed + 1)
        random.seed(seed)
        torch.manual_seed(seed)
        np.random.seed(seed)
        ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args("TIM-GD", K, visual), log_file=None)
        s_idx, q_idx = ev.sample_indices(tabs[1].numpy(), tabs[3].numpy())
        assert s_idx.shape == (2, 3, K * 2) and q_idx.shape == (2, 3, 75)
        _TABLES[visual] = (K, tabs, (s_idx, q_idx))
    return _TABLES[visual]


def _evaluate(method, visual, **kw):
    from src.eval_few_shot import Evaluator_few_shot
    K, tabs, indices = _tables(visual)
    ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args(method, K, visual, **kw), log_file=None)
    acc, _ = ev.evaluate_tasks(None, *tabs, indices=indices)
    return ev, acc


@pytest.mark.parametrize("method,visual", [("TIM-GD", False), ("TIM-GD", True), ("ALPHA_TIM", False)])
def test_evaluator_in_place_loop_agrees_and_builds_nothing(method, visual, monkeypatch):
    from src import eval_few_shot
    from tclip_amd import engine
    cls = eval_few_shot._METHODS[method]
    ev, acc = _evaluate(method, visual)
    assert ev.last_task_accuracies.shape == (2, 3) and ev.last_task_predictions.shape == (2, 3, 75) and 0 < float(acc) <= 1
    seen = []
    run_tables = cls.run_tables

    def spy(self, **kw):
        seen.append((id(self), kw["q_idx"].shape[0], kw["cols"] is None))
        return run_tables(self, **kw)
    monkeypatch.setattr(cls, "run_tables", spy)
    for kw in (dict(materialise_tasks=True), dict(batches_per_call=1), dict(in_place_loop=False), dict(in_place_support=True),
               dict(in_place_loop=True, materialise_tasks=True)):
        other, acc2 = _evaluate(method, visual, **kw)
        assert np.array_equal(other.last_task_predictions, ev.last_task_predictions), kw
        assert np.array_equal(other.last_task_accuracies, ev.last_task_accuracies), kw
        assert acc2 == acc, kw
    assert seen == []                                                  # none of these goes through run_tables

    # a support set that misses a class: the old route, option or not
    if not visual:
        with monkeypatch.context() as mp:
            mp.setattr(eval_few_shot, "relabel_indices", lambda *a, **k: None)
            other, acc2 = _evaluate(method, visual, in_place_loop=True)
            assert np.array_equal(other.last_task_predictions, ev.last_task_predictions) and acc2 == acc and seen == []
            assert np.array_equal(other.last_task_accuracies, ev.last_task_accuracies)

    calls = []
    gather_task_rows = engine.gather_task_rows
    monkeypatch.setattr(engine, "gather_task_rows", lambda *a, **k: (calls.append(1), gather_task_rows(*a, **k))[1])
    monkeypatch.setattr(engine, "gather_rows", lambda *a, **k: calls.append(2))
    for kw, want in ((dict(), [(6, visual)]), (dict(batches_per_call=1), [(3, visual), (3, visual)])):
        del seen[:]
        other, acc2 = _evaluate(method, visual, in_place_loop=True, **kw)
        assert np.array_equal(other.last_task_predictions, ev.last_task_predictions), kw
        assert np.array_equal(other.last_task_accuracies, ev.last_task_accuracies), kw
        assert np.array_equal(other.last_batch_criterions, ev.last_batch_criterions), kw
        assert acc2 == acc and type(other.last_method) is cls
        assert [s[1:] for s in seen] == want and id(other.last_method) == seen[-1][0]
    assert calls == []                                                 # in_place_loop builds no task tensor
    _evaluate(method, visual)
    assert calls == [1, 1]                                             # the default route does build them


def test_alpha_tim_still_refuses_visual_features():
    with pytest.raises(NotImplementedError, match="probability features"):
        _evaluate("ALPHA_TIM", True, in_place_loop=True)
    with pytest.raises(NotImplementedError, match="probability features"):
        _evaluate("ALPHA_TIM", True)


# ---- 4. memory of one in-place call ---------------------------------------------------------------------------------------

def test_in_place_tim_gd_call_allocates_neither_x_s_nor_x_q():
    """both bounds follow from the layout: the in-place call holds its workspace, its outputs and (should the binding copy
    them) the index, label and cols tensors, 512 bytes of allocator rounding for each; the dense call with its inputs holds
    x_s [T,S,D] on top"""
    from tclip_amd import _capi, engine
    K, S, T_, Q = 100, 400, 20, 75
    gen = torch.Generator().manual_seed(11)
    rows = 2000
    table_s = (torch.randn(rows, K, generator=gen) * 3).softmax(-1).to(DEV)
    table_q = (torch.randn(rows, K, generator=gen) * 3).softmax(-1).to(DEV)
    s_idx = torch.randint(0, rows, (T_, S), generator=gen).to(DEV)
    q_idx = torch.randint(0, rows, (T_, Q), generator=gen).to(DEV)
    y_s = torch.arange(K).repeat(T_, S // K).to(DEV)
    cols = torch.stack([torch.randperm(K, generator=gen) for _ in range(T_)]).to(torch.int32).to(DEV)
    p = ctypes.byref(_capi.Problem(1, T_, Q, K, S, ITERS, 1, 0, 0))
    ws = _capi.lib().tclip_tim_gd_tasks_workspace_bytes(p, K)
    assert ws > 0 and ws == _capi.lib().tclip_tim_gd_workspace_bytes(p, K)
    x_s_bytes = T_ * S * K * 4
    outputs = 4 * (T_ * K * K + T_ * Q * K + T_ * Q + ITERS * T_)
    index_tensors = 8 * (T_ * S + T_ * Q) + 8 * T_ * S + 4 * T_ * K        # s_idx, q_idx, y_s, cols
    n_tensors = 1 + 4 + 4                                                   # the workspace, the outputs, the four above
    bound = ws + outputs + index_tensors + 512 * n_tensors

    def rise(call):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()            # no cached block of another test's: the allocator hands out what is asked for, rounded
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    prm = dict(n_class=K, iters=ITERS, **GD)
    in_place, out = rise(lambda: engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, **prm))
    dense, want = rise(lambda: engine.run_tim_gd(engine.gather_task_rows(table_q, q_idx, cols), engine.gather_task_rows(table_s, s_idx, cols),
                                                 y_s, **prm))
    print(f"peak rise in place {in_place} bytes (bound {bound}, workspace {ws}), dense with its inputs {dense}, x_s {x_s_bytes}")
    assert in_place <= bound
    assert dense >= in_place + x_s_bytes
    assert_same(out, want, "memory case")


# ---- 5. range checks of the binding ----------------------------------------------------------------------------------------

def test_out_of_range_indices_and_columns_raise_index_error():
    from tclip_amd import engine
    K, S, rows = 5, 10, 30
    tab = torch.rand(rows, K, device=DEV)
    q_idx, s_idx = torch.randint(0, rows, (2, 75)), torch.randint(0, rows, (2, S))
    y_s = torch.arange(K).repeat(2, 2)
    cols = torch.arange(K, dtype=torch.int32).repeat(2, 1)
    calls = (lambda q, s, c: engine.run_tim_gd_tasks(tab, q, tab, s, y_s, c, n_class=K, iters=2, **GD),
             lambda q, s, c: engine.run_alpha_tim_tasks(tab, q, tab, s, y_s, c, iters=2, **ALPHA),
             lambda q, s, c: engine.run_alpha_tim_visual_tasks(tab, q, tab, s, y_s, n_class=K, iters=2, **ALPHA))
    for bad_value in (rows, -1):
        s_bad, q_bad = s_idx.clone(), q_idx.clone()
        s_bad[0, 0] = bad_value
        q_bad[1, 74] = bad_value
        for call in calls:
            for to in (lambda t: t, lambda t: t.to(DEV)):
                with pytest.raises(IndexError):
                    call(q_idx, to(s_bad), cols)
                with pytest.raises(IndexError):
                    call(to(q_bad), s_idx, cols)
    for bad_value in (K, -1):
        c_bad = cols.clone()
        c_bad[1, 2] = bad_value
        for call in calls[:2]:
            for c in (c_bad, c_bad.to(DEV)):
                with pytest.raises(IndexError):
                    call(q_idx, s_idx, c)
    for bad in (-1, K):
        y_bad = y_s.clone()
        y_bad[1, 3] = bad
        with pytest.raises(ValueError, match="label"):
            engine.run_tim_gd_tasks(tab, q_idx, tab, s_idx, y_bad, n_class=K, iters=2, **GD)
        with pytest.raises(ValueError, match="label"):
            engine.run_alpha_tim_tasks(tab, q_idx, tab, s_idx, y_bad, iters=2, **ALPHA)
    with pytest.raises(ValueError, match="Entropies must be in"):
        engine.run_alpha_tim_tasks(tab, q_idx, tab, s_idx, y_s, iters=2, entropies=("Shannon", "Renyi", "Alpha"), **ALPHA)
    for w in calls[0](q_idx, s_idx, cols):                              # and the arguments above are fine otherwise
        assert bool(torch.isfinite(w.float()).all())
    torch.cuda.synchronize()
