"""CPU: the host side of few-shot PADDLE and BDCSPN on visual features - the new C entries in the library and the header, the
fixtures' input digests, the option combination, and the few-shot methods that still refuse visual features."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT, golden_names
from helpers import visual_fs

ENTRIES = ("tclip_paddle_visual_workspace_bytes", "tclip_paddle_visual_run", "tclip_bdcspn_visual_workspace_bytes",
           "tclip_bdcspn_visual_run")
METHOD_LEVEL = ["fs_vis_paddle_D512_K10_S4_N3", "fs_vis_paddle_D1024_K37_S2_N2", "fs_vis_paddle_D768_K100_S1_N1",
                "fs_vis_bdcspn_D512_K10_S4_N3", "fs_vis_bdcspn_D1024_K37_S2_N2", "fs_vis_bdcspn_D768_K100_S1_N1",
                "lean_fs_vis_paddle_D1024_K1000_S1_N1", "lean_fs_vis_bdcspn_D1024_K1000_S1_N1"]
EVAL_LEVEL = ["eval_fs_vis_paddle_D512_K10", "eval_fs_vis_bdcspn_D512_K10"]


def test_entries_in_header_binding_and_sources():
    from tclip_amd import _capi
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _capi.EXPORTS
    assert "#define TCLIP_ABI_VERSION 5" in header
    sys.path.insert(0, PKG)
    import build
    assert "tclip_visual_fs.inc" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "tclip_visual_fs.inc"))


def test_entries_exported_by_the_library():
    from tclip_amd import _capi
    assert os.path.exists(_capi.LIB_PATH), "libtclip.so is missing: run build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= exported


@pytest.mark.parametrize("name", METHOD_LEVEL)
def test_fixture_inputs_regenerate(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_s, y_s, x_q, y_q = visual_fs.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"]), int(g["seed"]),
                                              signal=float(g["signal"]))
    assert x_s.shape == (int(g["N"]), int(g["K"]) * int(g["shots"]), int(g["D"])) and x_q.shape[1] == 75
    assert torch.equal(y_s[0], torch.arange(int(g["K"])).repeat_interleave(int(g["shots"])))      # class order, labels unchanged
    for k, a in (("x_s", x_s), ("x_q", x_q), ("y_s", y_s), ("y_q", y_q)):
        assert visual_fs.sha(a.numpy()) == str(g[k + "_sha1"]), k
    assert any(0.0 < a < 1.0 for a in g["acc"])
    assert np.array_equal((torch.from_numpy(g["preds"]).long() == y_q).float().mean(1).numpy(), g["acc"])
    if not name.startswith("lean_"):
        assert ((g["u"] > 1e-6) & (g["u"] < 1 - 1e-6)).any()
        assert np.array_equal(g["u"].argmax(2), g["preds"])


def test_fixtures_cover_the_norm_types_and_a_nonzero_lambd():
    load = lambda n: np.load(os.path.join(GOLDEN, n + ".npz"))
    assert {str(load(n)["norm_type"]) for n in METHOD_LEVEL if "bdcspn" in n} == {"L2N", "CL2N", "UN"}
    assert any(float(load(n)["lambd"]) != 0 for n in METHOD_LEVEL if "paddle" in n)


def test_fixture_names_and_sizes():
    for n in METHOD_LEVEL + EVAL_LEVEL:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 1 << 20
        assert not n.startswith("vis_")                  # that prefix belongs to the zero-shot k-means fixtures
    for prefix in ("", "fs_", "fs_paddle_", "fs_bdcspn_", "zs_"):
        assert not any("vis" in n for n in golden_names(prefix) if prefix != "fs_" or "fs_vis_" not in n)
    assert not set(METHOD_LEVEL) & set(golden_names())


@pytest.mark.parametrize("name", EVAL_LEVEL)
def test_evaluator_fixture_indices(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K, shots, rows = int(g["K"]), int(g["shots"]), int(g["rows_per_class"])
    nb = int(g["number_tasks"]) // int(g["batch_size"])
    assert g["support_idx"].shape == (nb, int(g["batch_size"]), K * shots) and g["query_idx"].shape == (nb, int(g["batch_size"]), 75)
    assert g["support_idx"].max() < K * rows and g["query_idx"].max() < K * rows
    assert g["task_accuracy"].shape == (nb, int(g["batch_size"])) and 0 < float(g["mean_accuracy"]) < 1


@pytest.mark.parametrize("method", ["paddle", "bdcspn"])
def test_option_combination(method):
    sys.path.insert(0, PKG)
    import main_features
    ns, cfg = main_features.parse_args(["--opts", "method", method, "use_softmax_feature", "False", "shots", "4"])
    assert cfg.use_softmax_feature is False and cfg.shots == 4 and cfg.name_method == method.upper() and cfg.tunable is True
    assert getattr(cfg, "text_features", None) is None
    from tclip_amd import reporting
    assert reporting.saved_feature_path(cfg, "train", "/r").endswith("data/synthetic/saved_features/train_visual_RN50.plk")


@pytest.mark.parametrize("module,cls", [("tim", "ALPHA_TIM"), ("laplacian_shot", "LAPLACIAN_SHOT")])
def test_alpha_tim_and_laplacian_shot_still_refuse_visual_features(module, cls):
    from src.utils import CfgNode
    mod = __import__(f"src.methods.few_shot.{module}", fromlist=[cls])
    a = CfgNode(iter=5, num_classes_test=4, n_class=4, n_query=75, k_eff=5, T=30, use_softmax_feature=False, temp=15,
                loss_weights=[1.0, 1.0, 1.0], lr_alpha_tim=1e-4, entropies=["Shannon", "Alpha", "Alpha"], alpha_value=7.0,
                knn=3, lmd=0.7, norm_type="L2N", lambd=0.0, batch_size=1, shots=2)
    m = getattr(mod, cls)(model=None, device="cuda", log_file=None, args=a)
    with pytest.raises(NotImplementedError, match="use_softmax_feature"):
        m.run_method(support=torch.randn(1, 8, 16), query=torch.randn(1, 75, 16), y_s=torch.zeros(1, 8, dtype=torch.long),
                     y_q=torch.zeros(1, 75, dtype=torch.long))


def test_restated_steps_run_on_the_host():
    """the torch restatements the GPU sweep compares against: shapes, and PADDLE's w_update at u = one-hot of the labels"""
    x_s, y_s, x_q = visual_fs.random_tasks(2, 5, 33, 2, seed=1)
    u, v, w = visual_fs.paddle_step(x_s, x_q, y_s, 5, 2.0)
    assert u.shape == (2, 75, 5) and v.shape == (2, 5) and w.shape == (2, 5, 33)
    assert torch.allclose(u.sum(-1), torch.ones(2, 75), atol=1e-5)
    p, u, preds = visual_fs.bdcspn_pass(x_s, x_q, y_s, 5, 10.0, "CL2N")
    assert p.shape == (2, 5, 33) and u.shape == (2, 75, 5) and preds.shape == (2, 75)
    sums, counts = visual_fs.support_sums(x_s, y_s, 5)
    assert torch.equal(counts, torch.full((2, 5), 2.0)) and sums.shape == (2, 5, 33)
