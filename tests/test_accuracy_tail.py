"""CPU: the restatements of tests/helpers/accuracy_tail.py are pinned to the reference before any kernel is judged by them, and
every input condition of tests/test_gpu_accuracy_tail.py and tests/test_gpu_front_end.py is asserted here for every case, so
that a bad seed fails on the host.

  - prototypes_reference followed by the host matcher reproduces the accuracies the reference recorded, on every zero-shot
    method fixture (x_q, y_q, final u) and every visual k-means fixture (x_q, y_q, preds, text) - the latter through
    front_end_reference, the tail's scoring of the prototypes;
  - first_appearance is what ref_torch.clustering_accuracy builds;
  - the task-by-task and chunked evaluation of prototypes_reference has the bits of the formula in one piece;
  - prototype cases: the patterns give the cluster counts they are there for;
  - front-end cases: every float64 probability is at least 1e-32; the two scale orders differ in fp32 where they are to be
    told apart;
  - composition cases: fp32 and float64 prototypes lead to the same assignment (asserted inside compose_case)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_names
from helpers import accuracy_tail as at
from oracle import ref_torch

ZS = [n for n in golden_names("zs_") if "K1000" not in n]
VIS = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("vis_") and f.endswith(".npz"))


def _host_match(preds, ncl, ids, rows, y, K, graph=True):
    """tclip_match_clusters_host_strided, pinned to scipy by tests/test_capi_and_host.py"""
    from tclip_amd import _capi
    T, Q = preds.shape
    arrs = [np.ascontiguousarray(preds, np.int32), np.ascontiguousarray(ncl, np.int32), np.ascontiguousarray(ids, np.int32),
            np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(y, np.int64)]
    newp, acc = np.empty((T, Q), np.int32), np.empty(T, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _capi.lib().tclip_match_clusters_host_strided(T, Q, K, *[P(a) for a in arrs], int(graph), ids.shape[1], P(newp), P(acc))
    assert rc == 0, _capi.lib().tclip_last_error()
    return newp, acc


def test_fixtures_present():
    assert len(ZS) >= 30 and len(VIS) == 9


@pytest.mark.parametrize("name", ZS)
def test_prototypes_reference_reproduces_recorded_accuracy(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K = int(g["K"])
    x_q, y = torch.from_numpy(g["x_q"]), g["y_q"].squeeze(2)
    preds = torch.from_numpy(g["u"]).argmax(2).numpy()
    ncl, ids = at.first_appearance(preds, K)
    rows = at.prototypes_reference(preds, x_q, K, torch.float32)
    _, acc = _host_match(preds, ncl, ids, rows.numpy(), y, K)
    assert np.array_equal(acc, g["acc"][:, 0])
    _, acc_scipy = at.match_reference(preds, ncl, ids, rows, y, True)
    assert np.array_equal(acc_scipy, g["acc"][:, 0])


@pytest.mark.parametrize("name", VIS)
def test_visual_tail_restatement_reproduces_recorded_accuracy(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_q, y, preds, text, T = torch.from_numpy(g["x_q"]), g["y_q"], g["preds"], torch.from_numpy(g["text"]), float(g["T"])
    K, D = text.shape
    ncl, ids = at.first_appearance(preds, K)
    rows = at.prototypes_reference(preds, x_q, K, torch.float32)
    probs = at.front_end_reference(rows.reshape(-1, D), text, T, False, torch.float32).reshape(len(ncl), -1, K)
    for t in range(len(ncl)):
        probs[t, ncl[t]:] = 0.0                          # rows of no cluster (normalize(0) is NaN): never read
    _, acc = _host_match(preds, ncl, ids, probs.numpy(), y, K)
    assert np.array_equal(acc, g["acc"])
    _, acc_scipy = at.match_reference(preds, ncl, ids, probs, y, True)
    assert np.array_equal(acc_scipy, g["acc"])


@pytest.mark.parametrize("K,Q", [(5, 75), (7, 3), (100, 17), (7, 300), (65, 75)])
def test_first_appearance_is_what_the_oracle_builds(K, Q, monkeypatch):
    """ref_torch.clustering_accuracy hands scipy one cost row per cluster, in the order it found them: as many rows as
    n_clusters, row i the prototype of ids[i]"""
    import scipy.optimize
    preds, _ = at.make_preds(7, Q, K, seed=K * 1000 + Q)
    x_q = at.make_prob_rows(7, Q, K, seed=1)
    ncl, ids = at.first_appearance(preds, K)
    assert ids.shape == (7, min(Q, K)) and ids.dtype == np.int32 and ncl.dtype == np.int32
    dense = at.prototypes_reference_one_piece(preds, x_q, K, torch.float32)
    seen = []
    real = scipy.optimize.linear_sum_assignment
    monkeypatch.setattr(scipy.optimize, "linear_sum_assignment", lambda cost, maximize=False: (seen.append(cost.copy()), real(cost, maximize=maximize))[1])
    hot = ref_torch.one_hot_rows(torch.from_numpy(preds), K)
    ref_torch.clustering_accuracy(hot, x_q, torch.zeros(7, Q, dtype=torch.int64), K)
    assert len(seen) == 7
    for t in range(7):
        assert seen[t].shape == (ncl[t], K)
        assert (ids[t, ncl[t]:] == -1).all() and len(set(ids[t, :ncl[t]].tolist())) == ncl[t]
        assert np.array_equal(seen[t], -dense[t, ids[t, :ncl[t]].astype(np.int64)].numpy().astype(np.float64)), t


@pytest.mark.parametrize("shape,visual", [((65, 75, 7), False), ((100, 257, 7), False), ((72, 75, 17), False), ((7, 3, 7), False),
                                          ((5, 33, 75, 7), True), ((65, 513, 257, 7), True), ((7, 40, 300, 7), True),
                                          ((5, 1, 75, 7), True), ((130, 33, 75, 7), True)])
def test_task_by_task_and_chunked_equal_the_one_piece_formula(shape, visual):
    c = at.prototype_case(shape, visual)
    for dtype in (torch.float32, torch.float64):
        dense = at.prototypes_reference_one_piece(c["preds"], c["z"], c["K"], dtype)
        for limit in (1 << 29, 1 << 16):
            got = at.prototypes_reference(c["preds"], c["z"], c["K"], dtype, limit=limit)
            for t, n in enumerate(c["ncl"]):
                assert torch.equal(got[t, :n], dense[t, c["ids"][t, :n].astype(np.int64)]), (dtype, limit, t)
                assert not got[t, n:].any()
    assert len(at._column_chunks(c["K"], c["W"], c["preds"].shape[1], 4, 1 << 16)) > 1 or c["K"] * c["W"] < 4096


def test_shape_tables_hold_what_the_issue_lists():
    assert {s[0] for s in at.PROB_SHAPES if s[1] == 75 and s[2] == 7} >= set(at.PROB_K)
    assert {(k, q) for k in (7, 40, 100) for q in at.PROB_Q} <= {s[:2] for s in at.PROB_SHAPES}
    assert (1024, 1100) in {s[:2] for s in at.PROB_SHAPES} and {s[2] for s in at.PROB_SHAPES if s[0] == 72} == {1, 8, 9, 17}
    assert {s[1] for s in at.VIS_SHAPES if s[0] == 5 and s[2] == 75} == set(at.VIS_D)
    assert {s[0] for s in at.VIS_SHAPES if s[1] == 33} >= set(at.VIS_K) and (1000, 1024, 75) in {s[:3] for s in at.VIS_SHAPES}
    assert {s[2] for s in at.VIS_SHAPES if s[:2] == (7, 40)} == set(at.VIS_Q) and (65, 513, 257) in {s[:3] for s in at.VIS_SHAPES}
    # at least the six patterns wherever the reference's temporary allows it, and no temporary of 1 GB
    assert all(s[2] >= 7 for s in at.PROB_SHAPES if s[0] != 72 and s[:2] != (1024, 1100))
    assert all(s[3] >= 7 for s in at.VIS_SHAPES)
    for lists, visual in ((at.COMPOSE_PROB, False), (at.COMPOSE_VIS, True)):
        kq = [(s[0], s[2] if visual else s[1]) for s in lists]
        assert any(q < k for k, q in kq) and any(q > k for k, q in kq) and any(q != 75 for k, q in kq)
    assert {s[1] for s in at.FRONT_SHAPES if s[2] == 37 and s[0] == 65} >= set(at.FRONT_D)
    assert {s[2] for s in at.FRONT_SHAPES if s[1] == 512 and s[0] == 65 and s[3] == 30} >= set(at.FRONT_K)
    assert {s[0] for s in at.FRONT_SHAPES} == {1, 65}
    assert {(d, k, t) for (d, k) in ((512, 100), (1024, 1000), (1000, 397)) for t in (10, 30, 100)} <= {s[1:] for s in at.FRONT_SHAPES}


@pytest.mark.parametrize("shape", at.PROB_SHAPES, ids=at.prob_id)
def test_prototype_case_inputs_probability(shape):
    at.check_prototype_inputs(at.prototype_case(shape, False), shape)


@pytest.mark.parametrize("shape", at.VIS_SHAPES, ids=at.vis_id)
def test_prototype_case_inputs_visual(shape):
    at.check_prototype_inputs(at.prototype_case(shape, True), shape)


@pytest.mark.parametrize("kind", at.FRONT_KINDS)
@pytest.mark.parametrize("shape", at.FRONT_SHAPES, ids=at.front_id)
def test_front_end_case_inputs(shape, kind):
    c = at.front_case(shape, kind)                       # asserts min ref64 >= 1e-32 for both scale orders
    at.check_front_inputs(c, shape)
    assert abs(float(c["text"].norm(dim=-1).max()) - 1) < 1e-6


@pytest.mark.parametrize("shape", at.SWAP_CASES, ids=at.front_id)
def test_scale_orders_differ_where_they_are_told_apart(shape):
    c = at.front_case(shape, "sparse")
    assert shape[3] == 100
    before, after = c["ref32", False], c["ref32", True]
    assert int((before != after).sum()) > 0
    # and by more than a rounding of the softmax: the distance the GPU test compares is well above one fp32 ulp / sqrt(12)
    assert at.front_distance(before, after, c["ref64", False]) > 5e-7


@pytest.mark.parametrize("shape", at.COMPOSE_PROB, ids=at.prob_id)
def test_composition_case_inputs_probability(shape):
    c = at.compose_case(shape, False)                    # asserts that fp32 and float64 assign alike
    hot = ref_torch.one_hot_rows(torch.from_numpy(c["preds"]), c["K"])
    for graph in (True, False):
        acc, newp = ref_torch.clustering_accuracy(hot, c["x_q"], torch.from_numpy(c["y"]), c["K"], graph_matching=graph)
        acc64, newp64 = ref_torch.clustering_accuracy(hot, c["x_q"].double(), torch.from_numpy(c["y"]), c["K"], graph_matching=graph)
        assert torch.equal(newp, newp64) and torch.equal(acc, acc64)
        assert np.array_equal(newp.numpy(), c["want", graph][0]) and np.array_equal(acc[:, 0].numpy(), c["want", graph][1])
    assert 0.2 < c["want", True][1].mean() <= 1.0        # the relabelling is found again: the matcher has something to match


@pytest.mark.parametrize("shape", at.COMPOSE_VIS, ids=at.vis_id)
def test_composition_case_inputs_visual(shape):
    c = at.compose_case(shape, True)
    assert c["x_q"].shape == (shape[3], shape[2], shape[1])
    for graph in (True, False):
        newp, acc = c["want", graph]
        assert newp.min() >= 0 and newp.max() < c["K"] and ((acc >= 0) & (acc <= 1)).all()
