"""GPU: tclip_match_clusters (one wavefront per task, csrc/tclip_match.inc) equals the host entry
tclip_match_clusters_host_strided - pinned to scipy by tests/test_capi_and_host.py - bit for bit: array_equal on new_preds,
exact equality on acc, no tolerance.  Then the same through engine.clustering_accuracy[_visual](matching="device") and
through a drop-in class with args.device_matching."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tclip_amd import _capi, engine

pytestmark = pytest.mark.gpu

T_SHAPES = 13          # divides no tasks-per-block choice
SHAPES = [(5, 75), (10, 75), (37, 75), (100, 75), (200, 40), (64, 64), (1024, 75)]


def _first_appearance(preds, protos_full, K, c_stride=None):
    """n_clusters, cluster ids in first-appearance order (-1 padded) and their prototype rows, as tclip_cluster_prototypes
    leaves them: what tests/test_capi_and_host.py::_match builds"""
    T, Q = preds.shape
    cs = min(Q, K) if c_stride is None else c_stride
    ncl = np.zeros(T, np.int32)
    ids = -np.ones((T, cs), np.int32)
    pr = np.zeros((T, cs, K), np.float32)
    for t in range(T):
        order = []
        for c in preds[t]:
            if c not in order:
                order.append(int(c))
        ncl[t] = len(order)
        ids[t, :len(order)] = order
        pr[t, :len(order)] = protos_full[t, order]
    return ncl, ids, pr


def _host(preds, ncl, ids, pr, y, K, graph):
    T, Q = preds.shape
    newp = np.empty((T, Q), np.int32)
    acc = np.empty(T, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _capi.lib().tclip_match_clusters_host_strided(T, Q, K, P(preds), P(ncl), P(ids), P(pr), P(y), int(graph), ids.shape[1],
                                                       P(newp), P(acc))
    assert rc == 0, _capi.lib().tclip_last_error()
    return newp, acc


def _device(preds, ncl, ids, pr, y, K, graph):
    T, Q = preds.shape
    lib = _capi.lib()
    d = [torch.from_numpy(a).cuda() for a in (preds, ncl, ids, pr, y)]
    newp = torch.full((T, Q), -7, dtype=torch.int32, device="cuda")
    acc = torch.full((T,), -7.0, device="cuda")
    status = torch.full((T,), -7, dtype=torch.int32, device="cuda")
    assert lib.tclip_match_clusters_workspace_bytes(T, Q, K, ids.shape[1]) == 0
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.tclip_match_clusters(T, Q, K, *[P(t) for t in d], int(graph), ids.shape[1], P(newp), P(acc), P(status), None, 0,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.tclip_last_error()
    torch.cuda.synchronize()
    return newp.cpu().numpy(), acc.cpu().numpy(), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _shape_case(K, Q):
    """inputs of one shape and the host's answers for both graph_matching values, computed once"""
    rng = np.random.default_rng(1000 * K + Q)
    T = T_SHAPES
    preds = rng.integers(0, K, size=(T, Q)).astype(np.int32)
    preds[0, :] = 3 % K                                  # a single cluster
    preds[1, :] = np.arange(Q) % K                       # as many clusters as possible
    preds[5, :] = np.arange(Q)[::-1] % K                 # ... for the rank-one task too
    protos = rng.random((T, K, K)).astype(np.float32)
    protos[2] = 0.0                                      # all-zero prototypes: pure tie-breaking
    protos[3, :, : K // 2] = protos[3, :, K // 2: 2 * (K // 2)]   # exact ties between column halves
    protos[4, 1::2] = protos[4, 0:2 * (K // 2):2]       # duplicated prototype rows
    a, b = rng.random(K).astype(np.float32), rng.random(K).astype(np.float32)
    protos[5] = a[:, None] * b[None, :]                  # rank one: every cluster wants the same columns, long paths
    protos[6] = np.round(protos[6] * 4) / 4              # few distinct values: ties between assigned and unassigned columns
    y = rng.integers(0, K, size=(T, Q)).astype(np.int64)
    ncl, ids, pr = _first_appearance(preds, protos, K)
    assert ncl[0] == 1 and ncl[1] == min(Q, K)
    want = {g: _host(preds, ncl, ids, pr, y, K, g) for g in (1, 0)}
    return preds, ncl, ids, pr, y, want


@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("K,Q", SHAPES)
def test_device_matching_equals_host(K, Q, graph):
    preds, ncl, ids, pr, y, want = _shape_case(K, Q)
    newp, acc, status = _device(preds, ncl, ids, pr, y, K, graph)
    assert not status.any()
    for t in range(T_SHAPES):
        assert np.array_equal(newp[t], want[graph][0][t]), f"task {t}"
    assert np.array_equal(acc, want[graph][1])


@pytest.mark.parametrize("graph", [1, 0])
def test_c_stride_beyond_the_fullest_task(graph):
    """rows of cluster_ids / prototypes beyond a task's count (-1 ids, rows never read) up to the full min(Q, K)"""
    K, Q, T = 100, 75, 5
    rng = np.random.default_rng(7)
    preds = rng.integers(0, 9, size=(T, Q)).astype(np.int32) * 11      # at most 9 clusters, labels spread over 0..88
    protos = rng.random((T, K, K)).astype(np.float32)
    y = rng.integers(0, K, size=(T, Q)).astype(np.int64)
    ncl, ids, pr = _first_appearance(preds, protos, K)
    assert ids.shape[1] == 75 and ncl.max() <= 9 and (ids[:, 9:] == -1).all()
    pr[:, 9:] = np.nan                                                  # whatever lies beyond is not read
    newp, acc, status = _device(preds, ncl, ids, pr, y, K, graph)
    want_p, want_a = _host(preds, ncl, ids, pr, y, K, graph)
    used = int(ncl.max())                                               # the compact layout the host path of the engine copies
    tight_p, tight_a = _host(preds, ncl, np.ascontiguousarray(ids[:, :used]), np.ascontiguousarray(pr[:, :used]), y, K, graph)
    assert not status.any()
    assert np.array_equal(newp, want_p) and np.array_equal(acc, want_a)
    assert np.array_equal(newp, tight_p) and np.array_equal(acc, tight_a)


def test_failing_tasks_fail_alone():
    """a NaN prototype block (no feasible assignment) and a cluster id equal to K: argument checks per task, nothing faults"""
    K, Q, T = 10, 75, 4
    rng = np.random.default_rng(11)
    preds = rng.integers(0, K, size=(T, Q)).astype(np.int32)
    protos = rng.random((T, K, K)).astype(np.float32)
    y = rng.integers(0, K, size=(T, Q)).astype(np.int64)
    ncl, ids, pr = _first_appearance(preds, protos, K)
    pr[1] = np.nan
    ids[3, 0] = K
    newp, acc, status = _device(preds, ncl, ids, pr, y, K, 1)
    assert status[1] != 0 and status[3] != 0 and status[0] == 0 and status[2] == 0
    for t in (1, 3):
        assert np.isnan(acc[t]) and (newp[t] == -1).all()
    good = [0, 2]
    want_p, want_a = _host(*[np.ascontiguousarray(a[good]) for a in (preds, ncl, ids, pr, y)], K, 1)
    assert np.array_equal(newp[good], want_p) and np.array_equal(acc[good], want_a)
    with pytest.raises(RuntimeError, match=r"\[1, 3\]"):
        engine.match_status_ok(torch.from_numpy(acc))
    # the other per-task checks: a cluster count beyond c_stride, a prediction outside 0..K-1
    ncl2, preds2 = ncl.copy(), preds.copy()
    ncl2[0] = ids.shape[1] + 1
    preds2[2, Q - 1] = -1
    _, ids_ok, pr_ok = _first_appearance(preds, protos, K)
    newp, acc, status = _device(preds2, ncl2, ids_ok, pr_ok, y, K, 1)
    assert status[0] != 0 and status[2] != 0 and status[1] == 0 and status[3] == 0
    assert np.isnan(acc[[0, 2]]).all() and (newp[[0, 2]] == -1).all()
    want_p, want_a = _host(*[np.ascontiguousarray(a[[1, 3]]) for a in (preds, ncl, ids_ok, pr_ok, y)], K, 1)
    assert np.array_equal(newp[[1, 3]], want_p) and np.array_equal(acc[[1, 3]], want_a)


def _captured(fn):
    """runs fn once eagerly (code objects loaded, allocator warm), then inside a graph capture - where any synchronisation or
    copy to the host is an error - and returns the results of the replay"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()
    torch.cuda.synchronize()
    return out


def test_engine_device_matching_equals_host_and_does_not_synchronise():
    T, Q, K = 6, 75, 37
    gen = torch.Generator().manual_seed(3)
    x_q = torch.softmax(4 * torch.randn(T, Q, K, generator=gen), -1).cuda()
    preds = torch.randint(0, K, (T, Q), generator=gen, dtype=torch.int32).cuda()
    y_q = torch.randint(0, K, (T, Q), generator=gen)
    y_dev = y_q.cuda()
    for graph in (True, False):
        acc_h, new_h = engine.clustering_accuracy(x_q, preds, y_q, graph)
        acc_d, new_d = engine.clustering_accuracy(x_q, preds, y_q, graph, matching="device")       # y_q from the host
        assert acc_d.is_cuda and new_d.is_cuda and acc_d.dtype == torch.float32 and new_d.dtype == torch.int32
        assert not acc_h.is_cuda and not new_h.is_cuda
        assert torch.equal(new_d.cpu(), new_h) and torch.equal(acc_d.cpu(), acc_h)
        acc_g, new_g = _captured(lambda: engine.clustering_accuracy(x_q, preds, y_dev, graph, matching="device"))
        assert acc_g.is_cuda and new_g.is_cuda
        assert torch.equal(new_g.cpu(), new_h) and torch.equal(acc_g.cpu(), acc_h)


def test_engine_visual_device_matching_equals_host_and_does_not_synchronise():
    T, Q, D, K = 4, 75, 64, 10
    gen = torch.Generator().manual_seed(5)
    x_q = torch.randn(T, Q, D, generator=gen).cuda()
    text = torch.nn.functional.normalize(torch.randn(K, D, generator=gen), dim=1).cuda()
    preds = torch.randint(0, K, (T, Q), generator=gen, dtype=torch.int32).cuda()
    y_q = torch.randint(0, K, (T, Q), generator=gen)
    y_dev = y_q.cuda()
    acc_h, new_h = engine.clustering_accuracy_visual(x_q, preds, y_q, text, 30.0)
    acc_d, new_d = engine.clustering_accuracy_visual(x_q, preds, y_q, text, 30.0, matching="device")
    assert acc_d.is_cuda and new_d.is_cuda
    assert torch.equal(new_d.cpu(), new_h) and torch.equal(acc_d.cpu(), acc_h)
    acc_g, new_g = _captured(lambda: engine.clustering_accuracy_visual(x_q, preds, y_dev, text, 30.0, matching="device"))
    assert acc_g.is_cuda and new_g.is_cuda
    assert torch.equal(new_g.cpu(), new_h) and torch.equal(acc_g.cpu(), acc_h)


def test_drop_in_class_with_device_matching():
    from src.methods.zero_shot.soft_kmeans import SOFT_KMEANS
    from src.utils import CfgNode
    from tclip_amd import synth
    K, N = 10, 3
    x_q, y_q = synth.make_query_tasks(N, K, seed=4)
    logs, matched = {}, {}
    for flag in (False, True):
        args = CfgNode(iter=5, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, use_softmax_feature=True,
                       graph_matching=True)
        if flag:
            args.device_matching = True
        m = SOFT_KMEANS(model=None, device=torch.device("cuda:0"), log_file=None, args=args)
        logs[flag] = m.run_task({"x_q": x_q.clone(), "y_q": y_q.clone()})
        matched[flag] = m.matched_preds
    assert matched[True].is_cuda and not matched[False].is_cuda
    assert torch.equal(matched[True].cpu(), matched[False])
    assert logs[True]["acc"].dtype == logs[False]["acc"].dtype and logs[True]["acc"].shape == (N, 1)
    assert np.array_equal(logs[True]["acc"], logs[False]["acc"])
    # a NaN accuracy of the device path becomes the host path's RuntimeError in get_logs
    m.init_info_lists()
    m.test_acc = [torch.tensor([[0.5], [float("nan")], [1.0]]).cuda()]
    with pytest.raises(RuntimeError, match=r"\[1\]"):
        m.get_logs()
