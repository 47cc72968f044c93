"""GPU: EM_GAUSSIAN_COV on visual features (use_softmax_feature == False) at the engine level.

The loop from the reference's own u0 is pinned bit for bit to reference-made fixtures (tests/golden/make_golden_visual_cov.py);
at D = K, on simplex rows with u0 = x_q, to the probability-feature entry; and over a sweep of feature lengths, class counts,
query counts and task counts to the torch-CPU restatement of tests/helpers/visual_cov.py, which tests/test_visual_cov.py pins to
the same fixtures."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import visual, visual_cov

pytestmark = pytest.mark.gpu

FULL = ["full_vis_emgc_D512_K10_N3", "full_vis_emgc_D1024_K37_N2", "full_vis_emgc_D768_K100_N1", "full_vis_emgc_D5_K4_N2"]
LEAN = "lean_vis_emc_D1024_K1000_N1"
NAMES = ("u", "v", "w", "s", "preds")


@pytest.fixture(scope="module")
def log():
    """the reference host's logarithm on every host (helpers/visual_cov.py)"""
    return visual_cov.restated_log()


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(x_q, u0, iters, lambd):
    from tclip_amd import engine
    out = engine.run_em_gaussian_cov_visual(x_q.cuda(), u0.cuda(), iters=iters, lambd=lambd)
    return dict(zip(NAMES, (o.cpu() for o in out)))


def assert_same_bits(got, want, what):
    """prints the number of differing elements of every tensor before asserting that there is none"""
    bad = {}
    for k in NAMES:
        a, b = got[k].numpy(), want[k].numpy()
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        bad[k] = int((a.view(np.int32) != b.view(np.int32)).sum())
    print(what, "differing elements:", bad)
    assert not any(bad.values()), (what, bad)


@pytest.mark.parametrize("name", FULL)
def test_loop_parity_from_reference_u0(name):
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_q = torch.from_numpy(g["x_q"])
    got = run(x_q, torch.from_numpy(g["u0"]), int(g["iters"]), int(g["lambd"]))
    for k in NAMES:
        if k in g:
            assert torch.equal(got[k], torch.from_numpy(g[k])), k
        else:                     # the fixture would pass 1 MiB with w and s in it
            assert sha(got[k].numpy()) == str(g[k + "_sha1"]), k
    acc, _ = engine.clustering_accuracy_visual(x_q.cuda(), got["preds"].cuda(), torch.from_numpy(g["y_q"]), torch.from_numpy(g["text"]),
                                               float(g["T"]))
    assert np.array_equal(acc.numpy(), g["acc"])


def test_lean_case_digests():
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, LEAN + ".npz"))
    x_q, y_q, text = visual.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["seed"]))
    assert sha(x_q.numpy()) == str(g["x_q_sha1"])
    got = run(x_q, torch.from_numpy(g["u0"]), int(g["iters"]), int(g["lambd"]))
    for k in ("u", "v", "w", "s"):
        assert sha(got[k].numpy()) == str(g[k + "_sha1"]), k
    assert np.array_equal(got["preds"].numpy(), g["preds"])
    acc, _ = engine.clustering_accuracy_visual(x_q.cuda(), got["preds"].cuda(), y_q, text, float(g["T"]))
    assert np.array_equal(acc.numpy(), g["acc"])


@pytest.mark.parametrize("K", [10, 100])
def test_equals_the_probability_entry_at_D_equal_K(K):
    """simplex rows, u0 = x_q: the op sequence of tclip_em_gaussian_cov_run with the row length equal to the class count"""
    from tclip_amd import engine
    gen = torch.Generator().manual_seed(40 + K)
    x_q = (4 * torch.randn(3, 75, K, generator=gen)).softmax(-1)
    lambd = int(K / 5) * 75
    want = dict(zip(NAMES, (o.cpu() for o in engine.run_em_gaussian_cov(x_q.cuda(), iters=20, lambd=lambd))))
    assert_same_bits(run(x_q, x_q, 20, lambd), want, f"D = K = {K}")


# (D, K, Q, T): every D at which the row sums change their path (D < 8, the leftover vectors and the tail, one or several
# 256-element chunks of the LDS tiles, the cascade hand-overs at 512 and 1024) with K = 5; one, exactly one, and more than one
# 64-class tile with a partial last one; query counts below, not a multiple of and above the 16 wavefronts of a block; one and
# several tasks
SWEEP = [(d, 5, 75, 2) for d in (1, 5, 7, 8, 9, 31, 33, 64, 511, 512, 513, 1000, 1024)]
SWEEP += [(96, k, 75, 2) for k in (2, 64, 65, 130)]
SWEEP += [(40, 7, q, 2) for q in (1, 3, 75)]
SWEEP += [(40, 7, 75, 1), (40, 7, 75, 5)]
_seen = set()
SWEEP = [c for c in SWEEP if not (c in _seen or _seen.add(c))]


@pytest.mark.parametrize("D,K,Q,T", SWEEP)
def test_three_iterations_match_torch(D, K, Q, T, log):
    gen = torch.Generator().manual_seed(((D * 1031 + K) * 131 + Q) * 7 + T)
    x_q = torch.randn(T, Q, D, generator=gen) * 3
    u0 = (torch.randn(T, Q, K, generator=gen) * 8).softmax(-1)
    lambd = int(K / 5) * Q
    want = dict(zip(NAMES, visual_cov.run(x_q, u0, 3, lambd, log=log)))
    assert all(torch.isfinite(want[k]).all() for k in ("u", "v", "w", "s"))
    assert_same_bits(run(x_q, u0, 3, lambd), want, f"D={D} K={K} Q={Q} T={T}")


def test_dead_clusters_keep_their_initial_rows(log):
    """two u0 columns exactly zero: those clusters are empty from the first iteration on, and their rows of w and s are the
    ones w_init / s_init wrote"""
    T, Q, K, D, dead = 2, 75, 9, 70, [2, 7]
    gen = torch.Generator().manual_seed(77)
    x_q = torch.randn(T, Q, D, generator=gen) * 3
    u0 = torch.zeros(T, Q, K)
    keep = [k for k in range(K) if k not in dead]
    u0[:, :, keep] = (torch.randn(T, Q, len(keep), generator=gen) * 8).softmax(-1)
    lambd = int(K / 5) * Q
    w0, s0 = visual_cov.init(x_q, u0)
    got = run(x_q, u0, 3, lambd)
    assert (got["u"][:, :, dead].sum(1) <= visual_cov.EPS).all()
    assert torch.equal(got["w"][:, dead].view(torch.int32), w0[:, dead].view(torch.int32))
    assert torch.equal(got["s"][:, dead].view(torch.int32), s0[:, dead].view(torch.int32))
    assert not torch.equal(got["w"][:, keep], w0[:, keep])
    assert_same_bits(got, dict(zip(NAMES, visual_cov.run(x_q, u0, 3, lambd, log=log))), "dead clusters")


def test_runs_inside_a_graph_capture():
    """no host synchronisation: the call is captured (after one eager call: code objects loaded, allocator warm, the LDS limit
    of the logits kernel raised) and the replay gives the eager call's bits"""
    from tclip_amd import engine
    T, Q, K, D = 3, 75, 12, 300            # D > 256: the restaged LDS tiles, 65 KB of dynamic LDS
    gen = torch.Generator().manual_seed(5)
    x_q = (torch.randn(T, Q, D, generator=gen) * 3).cuda()
    u0 = (torch.randn(T, Q, K, generator=gen) * 8).softmax(-1).cuda()
    fn = lambda: engine.run_em_gaussian_cov_visual(x_q, u0, iters=3, lambd=150)      # noqa: E731
    eager = [o.clone() for o in fn()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
