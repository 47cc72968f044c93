"""GPU: BD-CSPN and LAPLACIAN_SHOT reading their task rows from the feature tables in place.

  - engine.run_bdcspn[_visual]_tasks / run_laplacian_shot[_visual]_tasks against the dense entries fed `table[idx][..., cols]`,
    every output compared byte for byte, at the row lengths and support sizes where the row kernels change path;
  - the reference-made BD-CSPN and LaplacianShot fixtures through the in-place entries (rows embedded in a larger shuffled
    table, on probability features with inverse-permuted columns), asserting what the dense fixture tests assert;
  - Evaluator_few_shot.evaluate_tasks: `in_place_support`, the default route, materialise_tasks and batches_per_call agree,
    and no task tensor is built under the option;
  - the memory of one in-place BD-CSPN call against its workspace formula and against the dense call;
  - out-of-range indices and columns raise IndexError from the binding.
Nothing here skips: a missing fixture fails."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_names
from helpers import visual_fs, visual_lshot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(a, b):
    """byte for byte, on the host: NaN payloads and the sign of zero count, whatever the dtype"""
    if isinstance(b, np.ndarray):
        b = torch.from_numpy(np.ascontiguousarray(b))
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- 1. in place equals dense --------------------------------------------------------------------------------------------

S_LIST = (1, 3, 8, 17, 65, 130)          # on and off multiples of 4 and 8, and past 64 for the outer sum
Q_LIST = (10, 75)
T = 3


def _labels(S, K, gen):
    """every class present when S allows it, the rest at random (unequal class counts), shuffled per task; with S < K the
    empty classes' prototypes are 0/0 in both entries and the comparison of bytes covers them"""
    out = []
    for _ in range(T):
        y = torch.cat([torch.arange(min(S, K)), torch.randint(0, K, (max(S - K, 0),), generator=gen)])
        out.append(y[torch.randperm(S, generator=gen)])
    return torch.stack(out)


def _inputs(D, K, S, Q, softmax, seed):
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
    return table_q, q_idx, table_s, s_idx, _labels(S, K, gen), cols, x_q.contiguous(), x_s.contiguous()


VISUAL_SHAPES = [(D, K, S_LIST[(i + j) % 6], Q_LIST[(i + j) % 2])
                 for i, D in enumerate((1, 5, 8, 31, 33, 64, 65, 257)) for j, K in enumerate((4, 10, 37))]
SOFTMAX_SHAPES = [(K, S, Q) for K in (5, 37, 65) for S in S_LIST for Q in Q_LIST]


def test_the_shapes_cover_both_sizes_of_the_shared_region():
    big_zs = [s for s in VISUAL_SHAPES if s[2] * s[0] > (s[2] + s[3]) * s[1]]
    big_logit = [s for s in VISUAL_SHAPES if s[2] * s[0] <= (s[2] + s[3]) * s[1]]
    assert any(s[:2] == (257, 4) for s in big_zs) and big_logit
    assert {s[2] for s in VISUAL_SHAPES} == set(S_LIST) and {s[3] for s in VISUAL_SHAPES} == set(Q_LIST)


@pytest.mark.parametrize("K,S,Q", SOFTMAX_SHAPES)
def test_bdcspn_in_place_equals_dense_probability_features(K, S, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, cols, x_q, x_s = _inputs(K, K, S, Q, True, K * 1000 + S * 7 + Q)
    for i, norm_type in enumerate(("UN", "L2N", "CL2N")):
        dense = engine.run_bdcspn(x_q, x_s, y_s.to(DEV), temp=15.0, norm_type=norm_type)
        on_device = i == 1                                             # index tensors from the host and from the device
        tasks = engine.run_bdcspn_tasks(table_q, q_idx.to(DEV) if on_device else q_idx, table_s, s_idx.to(DEV) if on_device else s_idx,
                                        y_s, cols.to(DEV) if on_device else cols, temp=15.0, norm_type=norm_type)
        for name, a, b in zip(("prototypes", "u", "preds"), tasks, dense):
            assert same(a, b), (name, norm_type)
    if S >= K:
        assert bool(torch.isfinite(dense[0]).all())


@pytest.mark.parametrize("D,K,S,Q", VISUAL_SHAPES)
def test_bdcspn_in_place_equals_dense_visual_features(D, K, S, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, _, x_q, x_s = _inputs(D, K, S, Q, False, D * 1009 + K * 13 + S)
    for norm_type in ("UN", "L2N", "CL2N"):
        dense = engine.run_bdcspn_visual(x_q, x_s, y_s.to(DEV), n_class=K, temp=15.0, norm_type=norm_type)
        tasks = engine.run_bdcspn_visual_tasks(table_q, q_idx, table_s, s_idx.to(DEV), y_s, n_class=K, temp=15.0, norm_type=norm_type)
        assert tasks[0].shape == (T, K, D)
        for name, a, b in zip(("prototypes", "u", "preds"), tasks, dense):
            assert same(a, b), (name, norm_type)


@pytest.mark.parametrize("Q", [17, 257])
@pytest.mark.parametrize("D,K,S", [(40, 24, 49), (520, 10, 21)])
def test_bdcspn_in_place_equals_dense_visual_features_off_75_queries(D, K, S, Q):
    """a last query group of k_vis_dist with a single working wavefront (17 query rows) and the second level of k_vis_mstats's
    cascade over the S + Q augmented rows (257), on one-chunk and two-chunk rows"""
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, _, x_q, x_s = _inputs(D, K, S, Q, False, (D * 1009 + K * 13 + S) * 7 + Q)
    assert x_q.shape == (T, Q, D)
    for norm_type in ("UN", "L2N", "CL2N"):
        dense = engine.run_bdcspn_visual(x_q, x_s, y_s.to(DEV), n_class=K, temp=15.0, norm_type=norm_type)
        tasks = engine.run_bdcspn_visual_tasks(table_q, q_idx.to(DEV), table_s, s_idx, y_s, n_class=K, temp=15.0, norm_type=norm_type)
        assert tasks[1].shape == (T, Q, K)
        for name, a, b in zip(("prototypes", "u", "preds"), tasks, dense):
            assert same(a, b), (name, norm_type)
    if S >= K:
        assert bool(torch.isfinite(dense[0]).all())


LSHOT_OUT = ("unary", "neighbours", "preds_iter", "energies")


@pytest.mark.parametrize("K,S,Q", SOFTMAX_SHAPES)
def test_laplacian_shot_in_place_equals_dense_probability_features(K, S, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, cols, x_q, x_s = _inputs(K, K, S, Q, True, K * 1000 + S * 7 + Q + 1)
    for i, norm_type in enumerate(("UN", "L2N")):
        prm = dict(iters=6, knn=3, lmd=0.7, norm_type=norm_type)
        dense = engine.run_laplacian_shot(x_q, x_s, y_s.to(DEV), **prm)
        on_device = i == 1
        tasks = engine.run_laplacian_shot_tasks(table_q, q_idx.to(DEV) if on_device else q_idx, table_s,
                                                s_idx.to(DEV) if on_device else s_idx, y_s, cols.to(DEV) if on_device else cols, **prm)
        for name, a, b in zip(LSHOT_OUT, tasks, dense):
            assert same(a, b), (name, norm_type)


@pytest.mark.parametrize("D,K,S,Q", VISUAL_SHAPES)
def test_laplacian_shot_in_place_equals_dense_visual_features(D, K, S, Q):
    from tclip_amd import engine
    table_q, q_idx, table_s, s_idx, y_s, _, x_q, x_s = _inputs(D, K, S, Q, False, D * 1009 + K * 13 + S + 1)
    for norm_type in ("UN", "L2N"):
        prm = dict(n_class=K, iters=6, knn=3, lmd=0.7, norm_type=norm_type)
        dense = engine.run_laplacian_shot_visual(x_q, x_s, y_s.to(DEV), **prm)
        tasks = engine.run_laplacian_shot_visual_tasks(table_q, q_idx.to(DEV), table_s, s_idx, y_s, **prm)
        for name, a, b in zip(LSHOT_OUT, tasks, dense):
            assert same(a, b), (name, norm_type)


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


def _embed_permuted(x_s, x_q, K):
    gen = torch.Generator().manual_seed(K)
    cols = torch.stack([torch.randperm(x_q.shape[2], generator=gen) for _ in range(x_q.shape[0])]).to(torch.int32)
    table_s, s_idx = _embed(x_s, gen, inverse_of=cols)
    table_q, q_idx = _embed(x_q, gen, inverse_of=cols)
    return dict(table_s=table_s.to(DEV), s_idx=s_idx, table_q=table_q.to(DEV), q_idx=q_idx, cols=cols)


BDCSPN_FIX = ["fs_bdcspn_K100_N2_s2_cl2n", "fs_bdcspn_K100_N3_s1", "fs_bdcspn_K10_N4_s1_cl2n", "fs_bdcspn_K10_N4_s4",
              "fs_bdcspn_K37_N3_s2", "fs_bdcspn_K37_N3_s3_un", "fs_bdcspn_K397_N1_s1", "fs_bdcspn_K5_N3_s2"]
VIS_BDCSPN_FIX = ["fs_vis_bdcspn_D512_K10_S4_N3", "fs_vis_bdcspn_D1024_K37_S2_N2", "fs_vis_bdcspn_D768_K100_S1_N1"]
LSHOT_FIX = ["fs_lshot_K100_N3_s2", "fs_lshot_K10_N3_s1_un", "fs_lshot_K10_N4_s4", "fs_lshot_K37_N2_s3_k7", "fs_lshot_K37_N3_s2",
             "fs_lshot_K397_N1_s1", "fs_lshot_K5_N3_s2"]
LSHOT_BOUNDS = json.load(open(os.path.join(GOLDEN, "f4_tolerances.json")))["laplacian_shot"]


def test_every_fixture_is_listed():
    assert sorted(BDCSPN_FIX) == golden_names("fs_bdcspn_") and sorted(VIS_BDCSPN_FIX) == golden_names("fs_vis_bdcspn_")
    assert sorted(LSHOT_FIX) == golden_names("fs_lshot_") and sorted(visual_lshot.VISUAL) == golden_names("fs_vis_lshot_")


@pytest.mark.parametrize("name", BDCSPN_FIX)
def test_bdcspn_probability_fixture_in_place(name):
    """what tests/test_bdcspn.py::test_engine_matches_reference asserts, through BDCSPN.run_tables"""
    from src.methods.few_shot.bdcspn import BDCSPN
    from src.utils import CfgNode
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K = int(g["K"])
    m = BDCSPN(model=None, device=torch.device(DEV), log_file=None, args=CfgNode(norm_type=str(g["norm_type"]), temp=float(g["temp"]), n_class=K))
    y_s, y_q = torch.from_numpy(g["y_s"]).squeeze(2), torch.from_numpy(g["y_q"]).squeeze(2)
    m.run_tables(**_embed_permuted(torch.from_numpy(g["x_s"]), torch.from_numpy(g["x_q"]), K), y_s=y_s.to(DEV), y_q=y_q.to(DEV))
    logs = m.get_logs()
    assert np.array_equal(m.prototypes.cpu().numpy(), g["prototypes"]), "rectified prototypes differ"
    want_u = (float(g["temp"]) * torch.from_numpy(g["logits"])).softmax(-1)
    assert torch.equal(m.u.cpu(), want_u), "responsibilities differ"
    assert np.array_equal(logs["acc"], g["acc"])
    assert logs["criterions"].shape == g["criterions"].shape and (logs["criterions"] == 0).all()


@pytest.mark.parametrize("name", VIS_BDCSPN_FIX)
def test_bdcspn_visual_fixture_in_place(name):
    """what tests/test_gpu_visual_few_shot.py asserts of the C entry and of the drop-in class, through BDCSPN.run_tables"""
    from src.methods.few_shot.bdcspn import BDCSPN
    from src.utils import CfgNode
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_s, y_s, x_q, y_q = visual_fs.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"]), int(g["seed"]),
                                              signal=float(g["signal"]))
    for k, a in (("x_s", x_s), ("x_q", x_q), ("y_s", y_s), ("y_q", y_q)):
        assert visual_fs.sha(a.numpy()) == str(g[k + "_sha1"]), k
    K = int(g["K"])
    a = CfgNode(iter=20, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=False, name_method="BDCSPN",
                lambd=0.0, temp=float(g["temp"]), norm_type=str(g["norm_type"]))
    gen = torch.Generator().manual_seed(K)
    table_s, s_idx = _embed(x_s, gen)
    table_q, q_idx = _embed(x_q, gen)
    m = BDCSPN(model=None, device=DEV, log_file=None, args=a)
    m.run_tables(table_s=table_s.to(DEV), s_idx=s_idx, table_q=table_q.to(DEV), q_idx=q_idx, cols=None, y_s=y_s.to(DEV), y_q=y_q.to(DEV))
    logs = m.get_logs()
    assert np.array_equal(m.preds.cpu().numpy(), g["preds"])
    assert np.array_equal((m.preds.long().cpu() == y_q).float().mean(1).numpy(), g["acc"])
    assert np.array_equal(logs["acc"][:, -1], g["acc"])
    assert same(m.prototypes, g["prototypes"])
    assert same(m.u, g["u"])
    assert ((g["u"] > 1e-6) & (g["u"] < 1 - 1e-6)).any() and any(0 < v < 1 for v in g["acc"])


@pytest.mark.parametrize("name", LSHOT_FIX)
def test_laplacian_shot_probability_fixture_in_place(name):
    """what tests/test_laplacian_shot.py::test_engine_matches_reference asserts, through LAPLACIAN_SHOT.run_tables"""
    from src.methods.few_shot.laplacian_shot import LAPLACIAN_SHOT
    from src.utils import CfgNode
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K, N = int(g["K"]), int(g["N"])
    a = CfgNode(iter=int(g["iters"]), num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, shots=int(g["shots"]),
                use_softmax_feature=True, knn=int(g["knn"]), lmd=float(g["lmd"]), norm_type=str(g["norm_type"]), temp=30, batch_size=N)
    m = LAPLACIAN_SHOT(model=None, device=torch.device(DEV), log_file=None, args=a)
    y_s, y_q = torch.from_numpy(g["y_s"]).squeeze(2), torch.from_numpy(g["y_q"]).squeeze(2)
    m.run_tables(**_embed_permuted(torch.from_numpy(g["x_s"]), torch.from_numpy(g["x_q"]), K), y_s=y_s.to(DEV), y_q=y_q.to(DEV))
    logs = m.get_logs()
    assert np.array_equal(np.sort(m.neighbours.cpu().numpy(), axis=2), g["neighbours"]), "kNN graph differs"
    b = LSHOT_BOUNDS[name]
    du = np.abs(m.unary.cpu().numpy() - g["unary"]) / np.maximum(np.abs(g["unary"]), 1e-30)
    assert du.max() <= b["unary_rel"], f"unary term differs by {du.max():.2e} relative (bound {b['unary_rel']:.1e})"
    assert np.array_equal(m.preds.cpu().numpy(), g["preds"]), "final assignment differs"
    assert logs["acc"].shape == g["acc"].shape and np.array_equal(logs["acc"], g["acc"]), "per-update accuracies differ"
    assert logs["ent_energy"].shape == g["ent_energy"].shape
    de = np.abs(np.asarray(logs["ent_energy"]) / g["ent_energy"] - 1).max()
    assert de <= b["energy_rel"], f"energies differ by {de:.2e} relative (bound {b['energy_rel']:.1e})"
    assert logs["criterions"] == [[0]] * N


@pytest.mark.parametrize("name", visual_lshot.VISUAL)
def test_laplacian_shot_visual_fixture_in_place(name):
    """what tests/test_gpu_visual_lshot.py::test_fixture asserts, through engine.run_laplacian_shot_visual_tasks"""
    from tclip_amd import engine
    g = visual_lshot.load_fixture(GOLDEN, name)
    K, iters, knn = int(g["K"]), int(g["iters"]), int(g["knn"])
    gen = torch.Generator().manual_seed(K)
    table_s, s_idx = _embed(torch.from_numpy(g["x_s"]), gen)
    table_q, q_idx = _embed(torch.from_numpy(g["x_q"]), gen)
    y_s = torch.from_numpy(g["y_s"]).reshape(s_idx.shape)
    unary, nbr, preds_iter, e = engine.run_laplacian_shot_visual_tasks(
        table_q.to(DEV), q_idx, table_s.to(DEV), s_idx, y_s, n_class=K, iters=iters, knn=knn, lmd=float(g["lmd"]), norm_type=str(g["norm_type"]))
    torch.cuda.synchronize()
    assert unary.shape == g["unary"].shape and nbr.shape == g["neighbours"].shape and preds_iter.shape == g["preds_iter"].shape
    du = float((np.abs(unary.cpu().numpy() - g["unary"]) / np.maximum(np.abs(g["unary"]), 1e-30)).max())
    de = float(np.abs(e.cpu().numpy() / g["ent_energy"] - 1).max())
    print(f"{name}: unary {du:.3e} relative (bound {float(g['unary_rel']):.3e}), energies {de:.3e} relative (bound {float(g['energy_rel']):.3e})")
    assert np.array_equal(np.sort(nbr.cpu().numpy(), axis=2), g["neighbours"]), "kNN graph differs"
    assert np.array_equal(preds_iter[:, -1].cpu().numpy(), g["preds_iter"][:, -1]), "final assignment differs"
    acc = (preds_iter.cpu().long() == torch.from_numpy(g["y_q"])[:, None, :]).float().mean(2).numpy()
    assert np.array_equal(acc, g["acc"]), "per-update accuracies differ"
    assert du <= float(g["unary_rel"]), f"unary term differs by {du:.2e} relative (bound {float(g['unary_rel']):.1e})"
    assert de <= float(g["energy_rel"]), f"energies differ by {de:.2e} relative (bound {float(g['energy_rel']):.1e})"


# ---- 3. the evaluator's routes ----------------------------------------------------------------------------------------------

def _eval_args(method, K, visual, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=10, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=not visual,
                name_method=method, lambd=5.0, temp=15.0, norm_type="L2N", knn=3, lmd=0.7, loss_weights=[1.0, 0.3, 1.0],
                lr_tim=1e-3, number_tasks=6, batch_size=3, shots=2, used_test_set="test", dataset="synthetic", tunable=False)
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
        ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args("BDCSPN", K, visual), log_file=None)
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


@pytest.mark.parametrize("method,visual", [("BDCSPN", False), ("BDCSPN", True), ("LAPLACIAN_SHOT", False)])
def test_evaluator_in_place_support_agrees_and_builds_nothing(method, visual, monkeypatch):
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
    for kw in (dict(materialise_tasks=True), dict(batches_per_call=1), dict(in_place_support=False),
               dict(in_place_support=True, materialise_tasks=True)):
        other, acc2 = _evaluate(method, visual, **kw)
        assert np.array_equal(other.last_task_predictions, ev.last_task_predictions), kw
        assert np.array_equal(other.last_task_accuracies, ev.last_task_accuracies), kw
        assert acc2 == acc, kw
    assert seen == []                                                  # none of these goes through run_tables

    # a support set that misses a class: the old route, option or not
    with monkeypatch.context() as mp:
        mp.setattr(eval_few_shot, "relabel_indices", lambda *a, **k: None)
        if not visual:
            other, acc2 = _evaluate(method, visual, in_place_support=True)
            assert np.array_equal(other.last_task_predictions, ev.last_task_predictions) and acc2 == acc and seen == []

    def forbidden(*a, **k):
        raise AssertionError("in_place_support builds no task tensor")
    monkeypatch.setattr(engine, "gather_rows", forbidden)
    monkeypatch.setattr(engine, "gather_task_rows", forbidden)
    for kw, calls in ((dict(), [(6, visual)]), (dict(batches_per_call=1), [(3, visual), (3, visual)])):
        del seen[:]
        other, acc2 = _evaluate(method, visual, in_place_support=True, **kw)
        assert np.array_equal(other.last_task_predictions, ev.last_task_predictions), kw
        assert np.array_equal(other.last_task_accuracies, ev.last_task_accuracies), kw
        assert acc2 == acc and type(other.last_method) is cls
        assert [s[1:] for s in seen] == calls and id(other.last_method) == seen[-1][0]
    with pytest.raises(AssertionError, match="builds no task tensor"):
        _evaluate(method, visual)                                      # the default route does build them


def test_evaluator_option_leaves_the_other_methods_on_the_builder_route(monkeypatch):
    from tclip_amd import engine
    ev, acc = _evaluate("TIM-GD", True)
    calls = []
    gather_task_rows = engine.gather_task_rows
    monkeypatch.setattr(engine, "gather_task_rows", lambda *a, **k: (calls.append(1), gather_task_rows(*a, **k))[1])
    other, acc2 = _evaluate("TIM-GD", True, in_place_support=True)
    assert len(calls) == 2
    assert np.array_equal(other.last_task_predictions, ev.last_task_predictions) and acc2 == acc
    assert np.array_equal(other.last_task_accuracies, ev.last_task_accuracies)


def test_laplacian_shot_still_refuses_visual_features():
    with pytest.raises(NotImplementedError, match="probability features"):
        _evaluate("LAPLACIAN_SHOT", True, in_place_support=True)
    with pytest.raises(NotImplementedError, match="probability features"):
        _evaluate("LAPLACIAN_SHOT", True)


# ---- 4. memory of one in-place call ---------------------------------------------------------------------------------------

def test_in_place_bdcspn_call_allocates_neither_x_s_nor_zs():
    from tclip_amd import _capi, engine
    K, S, T_, Q = 100, 1600, 50, 75
    gen = torch.Generator().manual_seed(11)
    rows = 4000
    table_s = (torch.randn(rows, K, generator=gen) * 3).softmax(-1).to(DEV)
    table_q = (torch.randn(rows, K, generator=gen) * 3).softmax(-1).to(DEV)
    s_idx = torch.randint(0, rows, (T_, S), generator=gen).to(DEV)
    q_idx = torch.randint(0, rows, (T_, Q), generator=gen).to(DEV)
    y_s = torch.arange(K).repeat(T_, S // K).to(DEV)
    cols = torch.stack([torch.randperm(K, generator=gen) for _ in range(T_)]).to(torch.int32).to(DEV)
    p = ctypes.byref(_capi.Problem(1, T_, Q, K, S, 1, 1, 0, 0))
    ws, ws_dense = _capi.lib().tclip_bdcspn_tasks_workspace_bytes(p), _capi.lib().tclip_bdcspn_workspace_bytes(p)
    x_s_bytes = T_ * S * K * 4
    assert ws > 0 and x_s_bytes == 32_000_000 and ws == ws_dense - x_s_bytes          # zs inside the logits' region
    outputs = 4 * (T_ * K * K + T_ * Q * K + T_ * Q)
    index_tensors = 8 * (T_ * S + T_ * Q) + 8 * T_ * S + 4 * T_ * K        # s_idx, q_idx, y_s, cols, should the call copy them
    bound = ws + outputs + index_tensors + (1 << 20)

    def rise(call):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    in_place, out = rise(lambda: engine.run_bdcspn_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, temp=15.0))
    dense, want = rise(lambda: engine.run_bdcspn(engine.gather_task_rows(table_q, q_idx, cols), engine.gather_task_rows(table_s, s_idx, cols),
                                                 y_s, temp=15.0))
    print(f"peak rise in place {in_place} bytes (bound {bound}, workspace {ws}), dense {dense} (workspace {ws_dense}), x_s {x_s_bytes}")
    assert in_place <= bound
    assert in_place <= dense - x_s_bytes
    for a, b in zip(out, want):
        assert same(a, b)


# ---- 5. range checks of the binding ----------------------------------------------------------------------------------------

def test_out_of_range_indices_and_columns_raise_index_error():
    from tclip_amd import engine
    K, S, rows = 5, 10, 30
    tab = torch.rand(rows, K, device=DEV)
    q_idx, s_idx = torch.randint(0, rows, (2, 75)), torch.randint(0, rows, (2, S))
    y_s = torch.arange(K).repeat(2, 2)
    cols = torch.arange(K, dtype=torch.int32).repeat(2, 1)
    calls = (lambda q, s, c: engine.run_bdcspn_tasks(tab, q, tab, s, y_s, c, temp=15.0),
             lambda q, s, c: engine.run_bdcspn_visual_tasks(tab, q, tab, s, y_s, n_class=K, temp=15.0),
             lambda q, s, c: engine.run_laplacian_shot_tasks(tab, q, tab, s, y_s, c, iters=2, knn=3, lmd=0.7),
             lambda q, s, c: engine.run_laplacian_shot_visual_tasks(tab, q, tab, s, y_s, n_class=K, iters=2, knn=3, lmd=0.7))
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
        for call in (calls[0], calls[2]):
            for c in (c_bad, c_bad.to(DEV)):
                with pytest.raises(IndexError):
                    call(q_idx, s_idx, c)
    for bad in (-1, K):
        y_bad = y_s.clone()
        y_bad[1, 3] = bad
        with pytest.raises(ValueError, match="label"):
            engine.run_bdcspn_tasks(tab, q_idx, tab, s_idx, y_bad, temp=15.0)
        with pytest.raises(ValueError, match="label"):
            engine.run_laplacian_shot_tasks(tab, q_idx, tab, s_idx, y_bad, iters=2, knn=3, lmd=0.7)
    with pytest.raises(ValueError, match="norm_type"):
        engine.run_laplacian_shot_tasks(tab, q_idx, tab, s_idx, y_s, iters=2, knn=3, lmd=0.7, norm_type="CL2N")
    with pytest.raises(ValueError, match="norm_type"):
        engine.run_bdcspn_tasks(tab, q_idx, tab, s_idx, y_s, temp=15.0, norm_type="L1N")
    torch.cuda.synchronize()
