"""GPU: zero-shot SOFT_KMEANS, HARD_KMEANS, EM_GAUSSIAN and CLIP on visual features (use_softmax_feature == False).

The loop from the reference's own u0 is pinned bit for bit to reference-made fixtures (tests/golden/make_golden_visual.py) and,
one iteration at a time, to a torch-CPU restatement of the reference's op sequence over a sweep of feature lengths D and class
counts K (tests/helpers/visual.py).  The text-prompt initialisation is a GEMM, pinned to an fp64 evaluation within a bound."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG
from helpers import visual

pytestmark = pytest.mark.gpu

VIS = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("vis_") and f.endswith(".npz"))


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(method, x_q, u0, iters, T, lambd=0):
    from tclip_amd import engine
    x_q, u0 = x_q.cuda(), u0.cuda()
    if method == "soft_kmeans":
        u, w, preds = engine.run_soft_kmeans_visual(x_q, u0, iters=iters, temperature=T)
        return dict(u=u, w=w, preds=preds)
    if method == "hard_kmeans":
        u, w, preds, crit = engine.run_hard_kmeans_visual(x_q, u0, iters=iters)
        return dict(u=u, w=w, preds=preds, crit=crit)
    u, v, w, preds = engine.run_em_gaussian_visual(x_q, u0, iters=iters, temperature=T, lambd=lambd)
    return dict(u=u, v=v, w=w, preds=preds)


def test_fixtures_present():
    assert len(VIS) == 9 and {n.split("_")[1] for n in VIS} == {"skm", "hkm", "emg"}


@pytest.mark.parametrize("name", VIS)
def test_loop_parity_from_reference_u0(name):
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    method = str(g["method"])
    x_q = torch.from_numpy(g["x_q"])
    got = run(method, x_q, torch.from_numpy(g["u0"]), int(g["iters"]), float(g["T"]), int(g["lambd"]))
    assert np.array_equal(got["u"].cpu().numpy().view(np.uint32), g["u"].view(np.uint32))
    assert np.array_equal(got["w"].cpu().numpy().view(np.uint32), g["w"].view(np.uint32))
    assert np.array_equal(got["preds"].cpu().numpy(), g["preds"])
    if method == "em_gaussian":
        assert np.array_equal(got["v"].cpu().numpy().view(np.uint32), g["v"].view(np.uint32))
    if method == "hard_kmeans":       # the reference logs every criterion twice; a Frobenius norm: pinned as test_hard_kmeans.py pins it
        np.testing.assert_allclose(np.repeat(got["crit"].cpu().numpy()[0], 2), g["criterions"], rtol=5e-6, atol=0)
    acc, _ = engine.clustering_accuracy_visual(x_q.cuda(), got["preds"], torch.from_numpy(g["y_q"]), torch.from_numpy(g["text"]),
                                               float(g["T"]))
    assert np.array_equal(acc.numpy(), g["acc"])


def test_lean_case_digests():
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, "lean_vis_skm_D1024_K1000_N1.npz"))
    x_q, y_q, text = visual.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["seed"]))
    assert sha(x_q.numpy()) == str(g["x_q_sha1"])
    got = run("soft_kmeans", x_q, torch.from_numpy(g["u0"]), int(g["iters"]), float(g["T"]))
    assert sha(got["u"].cpu().numpy()) == str(g["u_sha1"])
    assert sha(got["w"].cpu().numpy()) == str(g["w_sha1"])
    acc, _ = engine.clustering_accuracy_visual(x_q.cuda(), got["preds"], y_q, text, float(g["T"]))
    assert np.array_equal(acc.numpy(), g["acc"])


# (D, K): every D of the sweep (the cascade hand-over at 512 and 1024 eight-float steps, D < 8, odd D whose K*D columns end
# in torch's 4-way row sums) with a small and a mid-size class count, the large class counts with a few D
SWEEP = [(d, k) for d in (1, 7, 8, 33, 255, 511, 512, 513, 640, 768, 1000, 1023, 1024) for k in (2, 10, 63, 64, 65)]
SWEEP += [(d, 397) for d in (33, 511, 512, 1023)] + [(d, 1000) for d in (7, 513, 1024)]
# What this sweep's inputs say about u: with rows of randn * 3 the squared distances differ by hundreds once D is large, and the
# reference's u after one iteration has an entry strictly between 1e-6 and 1 - 1e-6 only at D <= 8, at K >= 397 and at the six
# shapes below.  At the other 44 shapes - (33, 63), (33, 65), D = 255 but for K = 10, D = 512 but for K = 63, D = 640 but for
# K = 65, and every K <= 65 at D = 511, 513, 768, 1000, 1023, 1024 - u is zeros and ones: there the comparison pins w and the
# arg max, not the logits' last places (tests/test_gpu_visual_method_shapes.py scales the rows so that it does).
U_HAS_AN_INTERIOR_ENTRY = {(33, 2), (33, 10), (33, 64), (255, 10), (512, 63), (640, 65)}


@pytest.mark.parametrize("D,K", SWEEP)
def test_one_iteration_matches_torch(D, K):
    gen = torch.Generator().manual_seed(D * 1009 + K)
    N = 2 if K < 397 else 1
    x_q = torch.randn(N, 75, D, generator=gen) * 3
    u0 = (torch.randn(N, 75, K, generator=gen) * 8).softmax(-1)
    for method in ("soft_kmeans", "hard_kmeans", "em_gaussian") if K < 397 or D == 1024 else ("soft_kmeans",):
        lambd = int(K / 5) * 75
        ru, rw, rv = visual.reference_step(method, x_q, u0.clone(), T=30.0, lambd=lambd)
        if method != "hard_kmeans" and (D <= 8 or K >= 397 or (D, K) in U_HAS_AN_INTERIOR_ENTRY):
            assert bool(((ru > 1e-6) & (ru < 1 - 1e-6)).any()), method
        got = run(method, x_q, u0, 1, 30.0, lambd)
        assert np.array_equal(got["w"].cpu().numpy().view(np.uint32), rw.numpy().view(np.uint32)), method
        assert np.array_equal(got["u"].cpu().numpy().view(np.uint32), ru.numpy().view(np.uint32)), method
        if rv is not None:      # v = log(...) + 1 of the host's torch, whose SLEEF variant follows the host CPU's vector ISA: a few
            # ulp (the fixtures, made on the reference's side, pin v bit for bit; u and w above do not depend on the host's log)
            np.testing.assert_allclose(got["v"].cpu().numpy(), rv.numpy(), rtol=1e-6, atol=5e-7)


@pytest.mark.parametrize("name", ["vis_skm_D512_K10_N3", "vis_hkm_D1024_K37_N2", "vis_emg_D768_K100_N1"])
def test_end_to_end_from_embeddings_and_text(name):
    """GEMM init, so no reference bits: u0 within 2e-6 of an fp64 evaluation (fp32 GEMM noise on probabilities), then the
    loop's predictions and accuracies equal the reference's."""
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_q, text, T = torch.from_numpy(g["x_q"]), torch.from_numpy(g["text"]), float(g["T"])
    u0 = engine.visual_init(x_q.cuda(), text.cuda(), T).cpu()
    x64 = x_q.double()
    ref64 = (T * ((x64 / x64.norm(dim=-1, keepdim=True)) @ text.double().T)).softmax(-1)
    assert (u0.double() - ref64).abs().max() < 2e-6
    assert (u0.double() - torch.from_numpy(g["u0"]).double()).abs().max() < 2e-6
    got = run(str(g["method"]), x_q, u0, int(g["iters"]), T, int(g["lambd"]))
    assert np.array_equal(got["preds"].cpu().numpy(), g["preds"])
    acc, _ = engine.clustering_accuracy_visual(x_q.cuda(), got["preds"], torch.from_numpy(g["y_q"]), text, T)
    assert np.array_equal(acc.numpy(), g["acc"])


def _args(method, K, text, **kw):
    from src.utils import CfgNode
    iters = 10 if method == "HARD_KMEANS" else 20
    a = CfgNode(iter=iters, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=False,
                graph_matching=True, name_method=method, text_features=text)
    a.update(kw)
    return a


@pytest.mark.parametrize("name", ["vis_skm_D512_K10_N3", "vis_hkm_D512_K10_N3", "vis_emg_D512_K10_N3"])
def test_drop_in_run_task(name):
    from src.methods.zero_shot.em_gaussian import EM_GAUSSIAN
    from src.methods.zero_shot.hard_kmeans import HARD_KMEANS
    from src.methods.zero_shot.soft_kmeans import SOFT_KMEANS
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    cls = {"soft_kmeans": SOFT_KMEANS, "hard_kmeans": HARD_KMEANS, "em_gaussian": EM_GAUSSIAN}[str(g["method"])]
    m = cls(model=None, device="cuda", log_file=None, args=_args(cls.__name__, int(g["K"]), torch.from_numpy(g["text"])))
    logs = m.run_task({"x_q": torch.from_numpy(g["x_q"]), "y_q": torch.from_numpy(g["y_q"]).unsqueeze(2)})
    assert set(logs) == {"timestamps", "criterions", "acc"}
    assert logs["acc"].shape == (int(g["N"]), 1)
    assert np.array_equal(logs["acc"][:, -1], g["acc"])
    assert len(logs["criterions"]) == len(g["criterions"])


EVAL = ["SOFT_KMEANS", "HARD_KMEANS", "EM_GAUSSIAN", "CLIP"]


@pytest.mark.parametrize("method", EVAL)
def test_evaluator_on_visual_table(method, tmp_path):
    from src.eval_zero_shot import Evaluator_zero_shot
    g = np.load(os.path.join(GOLDEN, f"eval_zs_vis_{method.lower()}_D512_K10.npz"))
    K, D = int(g["K"]), int(g["D"])
    feats, labels, text = visual.make_table(K, D, int(g["rows_per_class"]), int(g["seed"]))
    np.save(tmp_path / "text.npy", text.numpy())
    a = _args(method, K, str(tmp_path / "text.npy"), number_tasks=int(g["number_tasks"]), batch_size=int(g["batch_size"]),
              used_test_set="test", dataset="synthetic", shots=0, iter=int(g["iters"]), lambd=5.0, iter_mm=0)
    ev = Evaluator_zero_shot(device=torch.device("cuda", 0), args=a, log_file=None)
    acc, _ = ev.evaluate_tasks(None, feats, labels, indices=torch.from_numpy(g["query_idx"]))
    assert np.array_equal(ev.last_task_accuracies.astype(np.float32), g["task_accuracy"])
    assert abs(float(acc) - float(g["mean_accuracy"])) < 1e-7


def test_main_features_visual_plk(tmp_path):
    """main_features on a visual .plk with --text-features: the reference's mean accuracy and its result file, under the
    _visual name"""
    from tclip_amd import features
    sys.path.insert(0, PKG)
    import main_features
    g = np.load(os.path.join(GOLDEN, "eval_zs_vis_soft_kmeans_D512_K10.npz"))
    feats, labels, text = visual.make_table(int(g["K"]), int(g["D"]), int(g["rows_per_class"]), int(g["seed"]))
    plk = str(tmp_path / "test_visual_RN50.plk")
    features.save_features(plk, feats, labels)
    torch.save(text, str(tmp_path / "text.pt"))
    acc, t, path = main_features.main(["--query", plk, "--results-root", str(tmp_path), "--text-features", str(tmp_path / "text.pt"),
                                       "--opts", "method", "soft_kmeans", "use_softmax_feature", "False", "number_tasks", "20",
                                       "batch_size", "10", "dataset", "synthetic", "seed", str(int(g["seed"]))])
    assert abs(float(acc) - float(g["mean_accuracy"])) < 1e-7
    assert path.endswith(os.path.join("results_zero_shot", "test", "synthetic", "SOFT_KMEANS_visual_0shot.txt"))
    assert open(path).read().splitlines()[-1].split("\t")[:4] == ["0", "75", "20", str(round(100 * float(g["mean_accuracy"]), 1))]
