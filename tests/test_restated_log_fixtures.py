"""The four log-using torch restatements (EM_GAUSSIAN, EM_GAUSSIAN_COV, KL_KMEANS, PADDLE) with the host-independent logarithm
of tests/helpers/restated.py in place of torch.log, against the fixtures the reference itself produced: every stored array bit
for bit.  That pins the swapped logarithm to the reference on any host, before tests/test_gpu_prob_method_shapes.py relies on it
at shapes no fixture holds.  What remains host-dependent is torch's sum order (AVX-512 kernels, at most 8 threads) and MKL's sgemm
in KL_KMEANS's centroids."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_names
from helpers.restated import restated_bmm, restated_log
from oracle import ref_torch

EMG, EMGC, KLK, PADDLE = (golden_names(p) for p in ("zs_emg_", "zs_emgc_", "zs_klk_", "fs_paddle_"))


@pytest.fixture(scope="module")
def log():
    return restated_log()


def load(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    if str(g["torch_version"]) != torch.__version__:
        pytest.skip("fixtures were made with another torch build")            # as the test_oracle_reproduces_reference tests
    return g, int(g["K"]), torch.from_numpy(g["x_q"])


def zero_shot_acc(t, g, K):
    acc, _ = ref_torch.clustering_accuracy(t["u"], torch.from_numpy(g["x_q"]), torch.from_numpy(g["y_q"]).squeeze(2), K)
    return acc.numpy()


def same_bits(t, g, pairs):
    """pairs: (restatement's key, fixture's key); the counts of differing elements are printed before any is asserted"""
    bad = {}
    for a, b in pairs:
        got, want = t[a].numpy(), g[b]
        assert got.shape == want.shape and got.dtype == want.dtype, (a, got.shape, got.dtype, want.shape, want.dtype)
        bad[a] = int((got.view(np.int32) != want.view(np.int32)).sum())
    print("differing elements:", bad)
    assert not any(bad.values()), bad


def test_fixtures_present():
    assert len(EMG) >= 5 and len(EMGC) >= 6 and len(KLK) >= 6 and len(PADDLE) >= 5


@pytest.mark.parametrize("name", EMG)
def test_em_gaussian(name, log):
    g, K, x_q = load(name)
    t = ref_torch.run_em_gaussian(x_q, n_class=K, iters=int(g["iters"]), temperature=30,
                                  lambd=int(K / 5) * 75, log=log)
    same_bits(t, g, [("w", "alpha"), ("u", "u"), ("v", "v")])
    assert np.array_equal(t["argmax"].numpy().astype(np.int16), g["argmax"])
    assert (t["criterions"] == 0).all() and (g["criterions"] == 0).all()
    assert np.array_equal(zero_shot_acc(t, g, K), g["acc"])


@pytest.mark.parametrize("name", EMGC)
def test_em_gaussian_cov(name, log):
    g, K, x_q = load(name)
    t = ref_torch.run_em_gaussian_cov(x_q, n_class=K, iters=int(g["iters"]), lambd=int(K / 5) * 75, log=log)
    same_bits(t, g, [("w", "alpha"), ("s", "s"), ("u", "u"), ("v", "v")])
    assert np.array_equal(t["argmax"].numpy().astype(np.int16), g["argmax"])
    assert (t["criterions"] == 0).all() and (g["criterions"] == 0).all()
    assert np.array_equal(zero_shot_acc(t, g, K), g["acc"])


@pytest.mark.parametrize("name", KLK)
def test_kl_kmeans(name, log):
    g, K, x_q = load(name)
    t = ref_torch.run_kl_kmeans(x_q, n_class=K, iters=int(g["iters"]), log=log, bmm=restated_bmm())
    same_bits(t, g, [("w", "alpha"), ("u", "u")])
    assert np.array_equal(t["labels"].numpy().astype(np.int16), g["argmax"])
    assert np.array_equal(t["criterions"].numpy(), g["criterions"][::2])          # the reference logs each twice
    assert np.array_equal(zero_shot_acc(t, g, K), g["acc"])


@pytest.mark.parametrize("name", PADDLE)
def test_paddle(name, log):
    g, K, x_q = load(name)
    t = ref_torch.run_paddle(x_q, torch.from_numpy(g["x_s"]), torch.from_numpy(g["y_s"]), n_class=K, iters=int(g["iters"]),
                             lambd=float(g["lambd"]), log=log)
    same_bits(t, g, [("w", "alpha"), ("u", "u"), ("v", "v")])
    assert np.array_equal(t["argmax"].numpy().astype(np.int16), g["argmax"])
    assert np.array_equal(t["criterions"].numpy(), g["criterions"]) and (g["criterions"] == 0).all()
    acc = (t["u"].argmax(2) == torch.from_numpy(g["y_q"]).squeeze(2)).float().mean(1, keepdim=True)
    assert np.array_equal(acc.numpy(), g["acc"])
