"""GPU: few-shot tasks built on the device and PADDLE reading its support rows in place.

  - engine.gather_task_rows (tclip_gather_task_rows) against torch indexing, compared as 32-bit words;
  - engine.run_paddle_tasks / run_paddle_visual_tasks against the dense entries on the tensors gather_task_rows builds,
    every output bit for bit;
  - the reference-made PADDLE fixtures through the in-place entries: the fixture's rows embedded in a larger table at
    shuffled positions, on probability features with inverse-permuted columns;
  - Evaluator_few_shot.evaluate_tasks: the default route, materialise_tasks and batches_per_call agree;
  - the memory of one in-place call stays under what its workspace, outputs and index tensors add up to.
Nothing here skips: a missing fixture fails."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_names
from helpers import visual_fs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def words(t):
    """the 32-bit words of a float tensor or array, on the host: comparisons that see NaN payloads and the sign of zero"""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t, np.float32))
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(words(a), words(b))


# ---- 1. the task builder -------------------------------------------------------------------------------------------------

def _bit_table(rows, width, gen):
    """random 32-bit patterns read as floats - NaNs with every payload, infinities, denormals - with a few planted for sure"""
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, width), generator=gen, dtype=torch.int64).to(torch.int32)
    planted = torch.tensor([0x7fc00001, 0x7f800001, -0x400000 + 0x12345, 0x7f800000, -0x800000, -2 ** 31, 1], dtype=torch.int64)
    flat = t.view(-1)
    pos = torch.randperm(flat.numel(), generator=gen)[:planted.numel()]
    flat[pos] = planted[:pos.numel()].to(torch.int32)
    return t


def _cols(mode, T, width, gen):
    if mode == "none":
        return None
    if mode == "flip":
        return torch.arange(width - 1, -1, -1, dtype=torch.int32).repeat(T, 1)
    return torch.stack([torch.randperm(width, generator=gen) for _ in range(T)]).to(torch.int32)


@pytest.mark.parametrize("mode", ["none", "flip", "random"])
@pytest.mark.parametrize("width", [1, 5, 63, 64, 65, 1024])
def test_gather_task_rows_equals_torch_indexing(width, mode):
    from tclip_amd import engine
    T, rows = 3, 29
    gen = torch.Generator().manual_seed(width * 7 + len(mode))
    bits = _bit_table(rows, width, gen)
    table = bits.view(torch.float32).to(DEV)
    assert same(table, bits.view(torch.float32))                      # the upload itself keeps the words
    for R in (1, 7):
        idx = torch.randint(0, rows, (T, R), generator=gen)
        idx[:, R // 2] = idx[:, 0]                                    # repeated indices
        cols = _cols(mode, T, width, gen)
        want = bits[idx]                                              # (T, R, width) int32
        if cols is not None:
            want = torch.gather(want, 2, cols.long().unsqueeze(1).expand(T, R, width))
        for on_device in (False, True):
            got = engine.gather_task_rows(table, idx.to(DEV) if on_device else idx,
                                          cols.to(DEV) if on_device and cols is not None else cols)
            assert got.shape == (T, R, width) and got.dtype == torch.float32 and got.is_cuda
            assert torch.equal(words(got), want), (R, on_device)
        if cols is None:
            assert torch.equal(words(engine.gather_rows(table, idx.reshape(-1)).view(T, R, width)), want)


def test_gather_task_rows_unaligned_table_takes_the_scalar_path():
    """a 16-byte aligned row length in a table that starts 4 bytes off: the wide loads must not be used"""
    from tclip_amd import engine
    gen = torch.Generator().manual_seed(3)
    bits = _bit_table(11, 64, gen)
    store = torch.empty(11 * 64 + 1, dtype=torch.float32, device=DEV)
    table = store[1:].view(11, 64)
    table.copy_(bits.view(torch.float32))
    assert table.data_ptr() % 16 == 4 and table.is_contiguous()
    idx = torch.randint(0, 11, (2, 5), generator=gen)
    assert torch.equal(words(engine.gather_task_rows(table, idx)), bits[idx])


def test_gather_task_rows_rejects_bad_indices():
    from tclip_amd import engine
    table = torch.randn(20, 8, device=DEV)
    good = torch.randint(0, 20, (2, 3))
    cols = torch.arange(8, dtype=torch.int32).repeat(2, 1)
    for bad_value in (20, -1):
        bad = good.clone()
        bad[1, 2] = bad_value
        for idx in (bad, bad.to(DEV)):
            with pytest.raises(IndexError):
                engine.gather_task_rows(table, idx)
        bad_cols = cols.clone()
        bad_cols[0, 5] = 8 if bad_value > 0 else -1
        for c in (bad_cols, bad_cols.to(DEV)):
            with pytest.raises(IndexError):
                engine.gather_task_rows(table, good, c)
    with pytest.raises(IndexError):
        engine.gather_task_rows(table, good, cols[:1])                # one permutation per task
    # the C entry: an index outside the table leaves its row unwritten and reads nothing
    from tclip_amd import _capi
    idx = torch.tensor([3, 20, -1, 5], device=DEV)
    out = torch.full((4, 8), 7.0, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = _capi.lib().tclip_gather_task_rows(P(table), 20, 8, P(idx), 2, None, 4, P(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0], table[3]) and torch.equal(out[3], table[5]) and bool((out[1:3] == 7.0).all())


# ---- 2. PADDLE in place equals PADDLE on the materialised tensors ------------------------------------------------------------

def _labels(T, S, K, gen):
    """every class present when S allows it (the first min(S, K) labels are distinct), the rest drawn at random - unequal
    class counts -, in a shuffled order"""
    out = []
    for _ in range(T):
        y = torch.cat([torch.arange(min(S, K)), torch.randint(0, K, (max(S - K, 0),), generator=gen)])
        out.append(y[torch.randperm(S, generator=gen)])
    return torch.stack(out)


def _shuffled_repeated(T, S, rows, gen):
    """support indices in no order, a third of them repeating another position's row"""
    idx = torch.stack([torch.randperm(rows, generator=gen)[:S] for _ in range(T)])
    for t in range(T):
        for j in range(0, S - 1, 3):
            idx[t, j + 1] = idx[t, j]
    return idx


@pytest.mark.parametrize("lambd", [0.0, 12.5])
@pytest.mark.parametrize("mode", ["flip", "random"])
@pytest.mark.parametrize("shots", [1, 4])
@pytest.mark.parametrize("K", [2, 5, 37, 100])
def test_paddle_in_place_equals_dense_probability_features(K, shots, mode, lambd):
    from tclip_amd import engine
    T, Q, S, rows = 3, 75, K * shots, K * shots + 50
    gen = torch.Generator().manual_seed(K * 31 + shots * 7 + len(mode))
    table_s = (torch.randn(rows, K, generator=gen) * 3).softmax(-1).to(DEV)
    table_q = (torch.randn(rows, K, generator=gen) * 3).softmax(-1).to(DEV)
    s_idx, q_idx = _shuffled_repeated(T, S, rows, gen), torch.randint(0, rows, (T, Q), generator=gen)
    y_s = torch.stack([torch.arange(K).repeat_interleave(shots)[torch.randperm(S, generator=gen)] for _ in range(T)])
    cols = _cols(mode, T, K, gen)
    x_s, x_q = engine.gather_task_rows(table_s, s_idx, cols), engine.gather_task_rows(table_q, q_idx, cols)
    dense = engine.run_paddle(x_q, x_s, y_s.to(DEV), iters=7, lambd=lambd)
    tasks = engine.run_paddle_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=7, lambd=lambd)
    for name, a, b in zip("uvw", tasks, dense):
        assert a.shape == b.shape and same(a, b), name
    assert torch.equal(tasks[3], dense[3])
    assert bool(torch.isfinite(dense[2]).all())


@pytest.mark.parametrize("s_kind", ["K", "17", "67", "4K+3"])
@pytest.mark.parametrize("K,D", [(2, 1), (3, 37), (10, 512), (37, 1024)])
def test_paddle_in_place_equals_dense_visual_features(K, D, s_kind):
    """S not a multiple of 4 (the leftover rows of the 4-way path), S above 16 (cascade dumps), K*D with and without a
    remainder mod 32 (both column paths), unequal class counts.  Every class is present wherever S >= K; at K = 37, S = 17 it
    cannot be, the empty classes' prototypes are 0/0 in both entries and the comparison of words covers them."""
    from tclip_amd import engine
    S = {"K": K, "17": 17, "67": 67, "4K+3": 4 * K + 3}[s_kind]
    T, Q, rows = 2, 75, S + 40
    gen = torch.Generator().manual_seed(K * 1009 + D * 13 + S)
    table_s = (torch.randn(rows, D, generator=gen) * (2.0 / D ** 0.5)).to(DEV)
    table_q = (torch.randn(rows, D, generator=gen) * (2.0 / D ** 0.5)).to(DEV)
    s_idx, q_idx = _shuffled_repeated(T, S, rows, gen), torch.randint(0, rows, (T, Q), generator=gen)
    y_s = _labels(T, S, K, gen)
    if S >= K:
        counts = torch.zeros(T, K).scatter_add_(1, y_s, torch.ones(T, S))
        assert bool((counts > 0).all()) and (S % K == 0 or bool((counts.max(1).values > counts.min(1).values).all()))
    x_s, x_q = engine.gather_task_rows(table_s, s_idx), engine.gather_task_rows(table_q, q_idx)
    dense = engine.run_paddle_visual(x_q, x_s, y_s.to(DEV), n_class=K, iters=3, lambd=7.5)
    tasks = engine.run_paddle_visual_tasks(table_q, q_idx, table_s, s_idx.to(DEV), y_s, n_class=K, iters=3, lambd=7.5)
    for name, a, b in zip("uvw", tasks, dense):
        assert a.shape == b.shape and same(a, b), name
    assert tasks[2].shape == (T, K, D)
    assert torch.equal(tasks[3], dense[3])
    if S >= K:
        assert bool(torch.isfinite(dense[2]).all())


@pytest.mark.parametrize("Q", [17, 257])
@pytest.mark.parametrize("K,D", [(24, 40), (10, 520)])
def test_paddle_in_place_equals_dense_visual_features_off_75_queries(K, D, Q):
    """the query rows are gathered once into the workspace: one query group of k_vis_dist with a single working wavefront (17)
    and the second level of k_vis_mstats's cascade (257), with k_vis_mstats and k_vis_mstats_one (K = 24) and rows of two chunks
    (D = 520)"""
    from tclip_amd import engine
    T, S, rows = 2, 2 * K + 1, 300
    gen = torch.Generator().manual_seed((K * 1009 + D) * 13 + Q)
    table_s = (torch.randn(rows, D, generator=gen) * (2.0 / D ** 0.5)).to(DEV)
    table_q = (torch.randn(rows, D, generator=gen) * (2.0 / D ** 0.5)).to(DEV)
    s_idx, q_idx = _shuffled_repeated(T, S, rows, gen), torch.randint(0, rows, (T, Q), generator=gen)
    y_s = _labels(T, S, K, gen)
    x_s, x_q = engine.gather_task_rows(table_s, s_idx), engine.gather_task_rows(table_q, q_idx)
    dense = engine.run_paddle_visual(x_q, x_s, y_s.to(DEV), n_class=K, iters=3, lambd=7.5)
    tasks = engine.run_paddle_visual_tasks(table_q, q_idx.to(DEV), table_s, s_idx, y_s, n_class=K, iters=3, lambd=7.5)
    for name, a, b in zip("uvw", tasks, dense):
        assert a.shape == b.shape and same(a, b), name
    assert tasks[0].shape == (T, Q, K) and torch.equal(tasks[3], dense[3])
    assert bool(torch.isfinite(dense[2]).all())
    u = dense[0]
    assert bool(((u > 1e-6) & (u < 1 - 1e-6)).any())


def test_paddle_tasks_reject_bad_input():
    from tclip_amd import engine
    K, S, rows = 5, 10, 30
    tab = torch.rand(rows, K, device=DEV)
    q_idx, s_idx = torch.randint(0, rows, (2, 75)), torch.randint(0, rows, (2, S))
    y_s = torch.arange(K).repeat(2, 2)
    for bad in (-1, K):
        y_bad = y_s.clone()
        y_bad[1, 3] = bad
        with pytest.raises(ValueError, match="label"):
            engine.run_paddle_tasks(tab, q_idx, tab, s_idx, y_bad, iters=1, lambd=0.0)
        with pytest.raises(ValueError, match="label"):
            engine.run_paddle_visual_tasks(tab, q_idx, tab, s_idx, y_bad, n_class=K, iters=1, lambd=0.0)
    s_bad = s_idx.clone()
    s_bad[0, 0] = rows
    for idx in (s_bad, s_bad.to(DEV)):
        with pytest.raises(IndexError):
            engine.run_paddle_tasks(tab, q_idx, tab, idx, y_s, iters=1, lambd=0.0)
        with pytest.raises(IndexError):
            engine.run_paddle_visual_tasks(tab, q_idx, tab, idx, y_s, n_class=K, iters=1, lambd=0.0)
    with pytest.raises(IndexError):
        engine.run_paddle_tasks(tab, q_idx, tab, s_idx, y_s, torch.full((2, K), K, dtype=torch.int32), iters=1, lambd=0.0)
    with pytest.raises(ValueError):
        engine.run_paddle_visual_tasks(tab, q_idx, tab, s_idx, y_s, n_class=1025, iters=1, lambd=0.0)
    with pytest.raises(ValueError):
        engine.run_paddle_tasks(tab, q_idx, tab[:, :4].contiguous(), s_idx, y_s, iters=1, lambd=0.0)
    torch.cuda.synchronize()


# ---- 3. the reference's fixtures through the in-place entries -----------------------------------------------------------------

def _embed(x, gen, inverse_of=None):
    """(table, idx): the rows of x (T, R, W) at shuffled positions of a table twice as long (the other rows hold noise), so that
    table[idx] == x; with `inverse_of` (T, W) column permutations the columns are stored inverse-permuted, so that
    table[idx[t]][:, inverse_of[t]] == x[t]."""
    T, R, W = x.shape
    pos = torch.randperm(2 * T * R + 3, generator=gen)[:T * R].view(T, R)
    table = torch.randn(2 * T * R + 3, W, generator=gen)
    if inverse_of is not None:
        stored = torch.empty_like(x)
        stored.scatter_(2, inverse_of.long().unsqueeze(1).expand(T, R, W), x)          # stored[t, r, cols[t, d]] = x[t, r, d]
        x = stored
    table[pos.reshape(-1)] = x.reshape(T * R, W)
    return table, pos


PROB_FIX = ["fs_paddle_K100_N3_s1", "fs_paddle_K10_N4_s4", "fs_paddle_K37_N3_s2", "fs_paddle_K397_N1_s1", "fs_paddle_K5_N3_s2"]
VIS_FIX = ["fs_vis_paddle_D512_K10_S4_N3", "fs_vis_paddle_D1024_K37_S2_N2", "fs_vis_paddle_D768_K100_S1_N1"]
LEAN_FIX = "lean_fs_vis_paddle_D1024_K1000_S1_N1"


def test_every_paddle_fixture_is_listed():
    assert sorted(PROB_FIX) == golden_names("fs_paddle_")
    assert sorted(VIS_FIX) == golden_names("fs_vis_paddle_")
    assert os.path.exists(os.path.join(GOLDEN, LEAN_FIX + ".npz"))


@pytest.mark.parametrize("name", PROB_FIX)
def test_probability_fixture_in_place(name):
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K = int(g["K"])
    x_s, x_q = torch.from_numpy(g["x_s"]), torch.from_numpy(g["x_q"])
    y_s, y_q = torch.from_numpy(g["y_s"]).squeeze(2), torch.from_numpy(g["y_q"]).squeeze(2)
    T = x_q.shape[0]
    gen = torch.Generator().manual_seed(K)
    cols = torch.stack([torch.randperm(K, generator=gen) for _ in range(T)]).to(torch.int32)
    table_s, s_idx = _embed(x_s, gen, inverse_of=cols)
    table_q, q_idx = _embed(x_q, gen, inverse_of=cols)
    u, v, w, preds = engine.run_paddle_tasks(table_q.to(DEV), q_idx, table_s.to(DEV), s_idx, y_s, cols, iters=int(g["iters"]),
                                             lambd=float(g["lambd"]))
    assert same(w, g["alpha"]), "prototypes differ"
    assert same(u, g["u"]), "responsibilities differ"
    assert same(v, g["v"]), "v differs"
    assert np.array_equal(preds.cpu().numpy(), g["argmax"][-1].astype(np.int32))
    acc = (preds.long().cpu() == y_q).float().mean(1, keepdim=True)
    assert np.array_equal(acc.numpy(), g["acc"])


def _visual_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_s, y_s, x_q, y_q = visual_fs.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"]), int(g["seed"]),
                                              signal=float(g["signal"]))
    for k, a in (("x_s", x_s), ("x_q", x_q), ("y_s", y_s), ("y_q", y_q)):
        assert visual_fs.sha(a.numpy()) == str(g[k + "_sha1"]), k
    gen = torch.Generator().manual_seed(int(g["K"]))
    table_s, s_idx = _embed(x_s, gen)
    table_q, q_idx = _embed(x_q, gen)
    from tclip_amd import engine
    out = engine.run_paddle_visual_tasks(table_q.to(DEV), q_idx, table_s.to(DEV), s_idx, y_s, n_class=int(g["K"]),
                                         iters=int(g["iters"]), lambd=float(g["lambd"]))
    return g, y_q, out


@pytest.mark.parametrize("name", VIS_FIX)
def test_visual_fixture_in_place(name):
    g, y_q, (u, v, w, preds) = _visual_fixture(name)
    assert np.array_equal(preds.cpu().numpy(), g["preds"])
    assert np.array_equal((preds.long().cpu() == y_q).float().mean(1).numpy(), g["acc"])
    assert same(w, g["w"]) and same(u, g["u"]) and same(v, g["v"])


def test_lean_visual_fixture_in_place():
    g, y_q, (u, v, w, preds) = _visual_fixture(LEAN_FIX)
    assert np.array_equal(preds.cpu().numpy(), g["preds"])
    assert np.array_equal((preds.long().cpu() == y_q).float().mean(1).numpy(), g["acc"]) and 0 < float(g["acc"][0]) < 1
    for k, a in (("u", u), ("v", v), ("w", w)):
        assert visual_fs.sha(a.cpu().numpy()) == str(g[k + "_sha1"]), k


# ---- 4. the evaluator's routes ---------------------------------------------------------------------------------------------

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
        K, seed = 10, 8100
        if visual:
            tabs = visual_fs.make_tables(K, 96, 40, seed, signal=0.3)
        else:
            tabs = synth.make_feature_table(K, 40, seed=seed) + synth.make_feature_table(K, 40, seed=seed + 1)
        random.seed(seed)
        torch.manual_seed(seed)
        np.random.seed(seed)
        ev = Evaluator_few_shot(device=torch.device(DEV), args=_eval_args("PADDLE", K, visual), log_file=None)
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


@pytest.mark.parametrize("method,visual", [("PADDLE", False), ("PADDLE", True), ("BDCSPN", False), ("LAPLACIAN_SHOT", False),
                                           ("TIM-GD", True)])
def test_evaluator_routes_agree(method, visual, monkeypatch):
    from tclip_amd import engine
    ev, acc = _evaluate(method, visual)
    assert ev.last_task_accuracies.shape == (2, 3) and ev.last_task_predictions.shape == (2, 3, 75)
    assert 0 < float(acc) <= 1
    for kw in (dict(materialise_tasks=True), dict(batches_per_call=1), dict(batches_per_call=0), dict(batches_per_call=5)):
        other, acc2 = _evaluate(method, visual, **kw)
        assert np.array_equal(other.last_task_predictions, ev.last_task_predictions), kw
        assert np.array_equal(other.last_task_accuracies, ev.last_task_accuracies), kw
        assert acc2 == acc, kw
        assert type(other.last_method) is type(ev.last_method)
    # the default route builds its tensors with the fused builder (or none at all): gather_rows is the materialised route's
    def no_gather(*a, **k):
        raise AssertionError("the default route must not call engine.gather_rows")
    monkeypatch.setattr(engine, "gather_rows", no_gather)
    again, acc3 = _evaluate(method, visual)
    assert np.array_equal(again.last_task_predictions, ev.last_task_predictions) and acc3 == acc
    with pytest.raises(AssertionError, match="gather_rows"):
        _evaluate(method, visual, materialise_tasks=True)


@pytest.mark.parametrize("visual", [False, True])
def test_paddle_default_route_reads_the_tables_in_place(visual, monkeypatch):
    """neither builder runs: PADDLE goes through run_tables on both feature kinds, and with a method object per group"""
    from src.methods.few_shot.paddle import PADDLE
    from tclip_amd import engine
    want, acc = _evaluate("PADDLE", visual, materialise_tasks=True)

    def forbidden(*a, **k):
        raise AssertionError("PADDLE's default route builds no task tensor")
    monkeypatch.setattr(engine, "gather_rows", forbidden)
    monkeypatch.setattr(engine, "gather_task_rows", forbidden)
    seen = []
    run_tables = PADDLE.run_tables

    def spy(self, **kw):
        seen.append((id(self), kw["q_idx"].shape[0], kw["cols"] is None))
        return run_tables(self, **kw)
    monkeypatch.setattr(PADDLE, "run_tables", spy)
    ev, acc2 = _evaluate("PADDLE", visual, batches_per_call=1)
    assert np.array_equal(ev.last_task_predictions, want.last_task_predictions) and acc2 == acc
    assert [s[1:] for s in seen] == [(3, visual), (3, visual)] and seen[0][0] != seen[1][0]
    assert id(ev.last_method) == seen[-1][0]


def test_no_column_permutation_falls_back_to_the_materialised_route(monkeypatch):
    """relabel_indices returns None for a support set that misses a class: gather_rows + relabel_batch run, as they always did"""
    from src import eval_few_shot
    from tclip_amd import engine
    want, acc = _evaluate("BDCSPN", False)
    calls = []
    gather_rows = engine.gather_rows
    monkeypatch.setattr(engine, "gather_rows", lambda *a, **k: (calls.append(1), gather_rows(*a, **k))[1])
    monkeypatch.setattr(eval_few_shot, "relabel_indices", lambda *a, **k: None)

    def forbidden(*a, **k):
        raise AssertionError("no column permutation: the fused builder has nothing to apply")
    monkeypatch.setattr(engine, "gather_task_rows", forbidden)
    for method in ("BDCSPN", "PADDLE"):
        del calls[:]
        ev, acc2 = _evaluate(method, False)
        assert len(calls) == 2
        if method == "BDCSPN":
            assert np.array_equal(ev.last_task_predictions, want.last_task_predictions) and acc2 == acc


# ---- 5. memory of one in-place call ---------------------------------------------------------------------------------------

def test_in_place_call_allocates_no_support_tensor():
    from tclip_amd import _capi, engine
    K, D, S, T, Q, iters = 100, 512, 1600, 50, 75, 2
    gen = torch.Generator().manual_seed(9)
    rows = 4000
    table_s = torch.randn(rows, D, generator=gen).to(DEV)
    table_q = torch.randn(rows, D, generator=gen).to(DEV)
    s_idx = torch.randint(0, rows, (T, S), generator=gen).to(DEV)
    q_idx = torch.randint(0, rows, (T, Q), generator=gen).to(DEV)
    y_s = torch.arange(K).repeat(T, S // K).to(DEV)
    ws = _capi.lib().tclip_paddle_visual_tasks_workspace_bytes(ctypes.byref(_capi.Problem(1, T, Q, K, S, iters, 1, 0, 0)), D)
    assert ws > 0
    outputs = 4 * (T * Q * K + T * K + T * K * D + T * Q)
    index_tensors = 8 * (T * S + T * Q)                              # s_idx, q_idx, should the call copy them
    bound = ws + outputs + index_tensors + (1 << 20)
    avoided = T * S * D * 4
    assert avoided == 163_840_000 and bound < avoided / 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = engine.run_paddle_visual_tasks(table_q, q_idx, table_s, s_idx, y_s, n_class=K, iters=iters, lambd=1.0)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes, bound {bound}, workspace {ws}, avoided x_s {avoided}")
    assert rise <= bound
    assert bool(torch.isfinite(out[2]).all())
