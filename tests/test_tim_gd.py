"""CPU: the host side of TIM_GD (reference: src/methods/few_shot/tim.py:90-189) - the class behind the reference's module
name, the command line's `method tim`, the evaluator's registration, the C entries, the fixtures' schema and the bounds they
carry, and the torch restatement (tests/helpers/tim_gd.py) the GPU sweep compares against."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT
from helpers import tim_gd

NAMES = tim_gd.PROB + tim_gd.VISUAL


def _args(**kw):
    from src.utils import CfgNode
    base = dict(iter=5, num_classes_test=4, n_class=4, n_query=75, k_eff=5, T=30, use_softmax_feature=True, temp=15,
                loss_weights=[1.0, 0.3, 1.0], lr_tim=1e-4, batch_size=1, shots=2)
    base.update(kw)
    return CfgNode(**base)


def test_module_provides_the_reference_classes():
    from src.methods.few_shot.tim import ALPHA_TIM, BASE, TIM_GD
    assert issubclass(TIM_GD, BASE) and issubclass(ALPHA_TIM, BASE)
    a = _args(lr_tim="2e-4")
    m = TIM_GD(model=None, device="cuda", log_file=None, args=a)
    assert m.lr == 2e-4 and m.temp == 15 and m.iter == 5
    assert m.loss_weights == [1.0, 0.3, 1.0] and m.loss_weights is not a.loss_weights        # copied, as tim.py:29
    assert not hasattr(m, "entropies") and not hasattr(m, "alpha_value")


def test_entries_in_header_and_binding():
    from tclip_amd import _capi
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    for name in ("tclip_tim_gd_workspace_bytes", "tclip_tim_gd_run"):
        assert name + "(" in header and name in _capi.EXPORTS
        assert header.index(name) < header.index("#define TCLIP_ABI_VERSION 5")              # in the "later" list of the comment
    assert "#define TCLIP_ABI_VERSION 5" in header


def test_workspace_query_checks_its_arguments():
    """no GPU is touched: the query validates the problem and sizes the T*K*D regions by dim"""
    import ctypes
    from tclip_amd import _capi
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 40, 30, 1, 0, 0)
    small, large = lib.tclip_tim_gd_workspace_bytes(ctypes.byref(p), 10), lib.tclip_tim_gd_workspace_bytes(ctypes.byref(p), 512)
    assert small == lib.tclip_alpha_tim_workspace_bytes(ctypes.byref(p))                      # dim == n_class: ALPHA_TIM's layout
    assert large >= 4 * (2 * 10 * 512 * 4) > small                                            # sup, dW, M, V are T*K*D floats
    for dim, word in ((0, b"dim"), (1025, b"dim")):
        assert lib.tclip_tim_gd_workspace_bytes(ctypes.byref(p), dim) == 0 and word in lib.tclip_last_error()
    for bad, word in ((_capi.Problem(1, 2, 75, 10, 40, 0, 1, 0, 0), b"iters"), (_capi.Problem(1, 2, 75, 10, 0, 30, 1, 0, 0), b"n_support")):
        assert lib.tclip_tim_gd_workspace_bytes(ctypes.byref(bad), 10) == 0 and word in lib.tclip_last_error()
    lw = (ctypes.c_float * 3)(1.0, 0.3, 1.0)
    assert lib.tclip_tim_gd_run(ctypes.byref(p), 10, 1e-4, 15.0, lw, *([None] * 8), 0, None) == 1      # null pointers: TCLIP_ERR_ARG


@pytest.mark.parametrize("visual", [False, True])
def test_command_line_method_tim(visual):
    sys.path.insert(0, PKG)
    import main_features
    opts = ["--opts", "method", "tim", "shots", "4"] + (["use_softmax_feature", "False"] if visual else [])
    ns, cfg = main_features.parse_args(opts)
    assert cfg.name_method == "TIM-GD" and cfg.lr_tim == 1e-4 and cfg.iter == 2000 and cfg.tunable is False
    assert cfg.temp == 15 and cfg.loss_weights == [1.0, 0.3, 1.0] and cfg.shots == 4
    from tclip_amd import reporting
    want = "train_visual_RN50.plk" if visual else "train_softmax_RN50_T30.plk"
    assert reporting.saved_feature_path(cfg, "train", "/r").endswith("data/synthetic/saved_features/" + want)
    assert reporting.saved_feature_path(cfg, "test", "/r").endswith(("test_visual_RN50.plk" if visual else "test_softmax_RN50_T30.plk"))


@pytest.mark.parametrize("spelling", ["TIM-GD", "TIM_GD"])
def test_evaluator_builds_tim_gd(spelling):
    from src.eval_few_shot import Evaluator_few_shot
    from src.methods.few_shot.tim import TIM_GD
    a = _args(name_method=spelling)
    ev = Evaluator_few_shot(device="cuda", args=a, log_file=None)
    assert type(ev.get_method_builder(model=None, device="cuda", args=a, log_file=None)) is TIM_GD
    assert spelling not in ev._TUNED                       # the reference's set_value_opt_param has no branch for it


def test_per_task_criterions_travel_in_the_gather():
    """sharding.method_parts ships TIM-GD's criterions as one (iter, N) block per batch, in batch order"""
    from types import SimpleNamespace
    from tclip_amd import sharding
    iters, nb, N, Q = 3, 2, 4, 75
    crit = np.arange(iters * nb * N, dtype=np.float32).reshape(iters, nb * N)
    m = SimpleNamespace(preds=torch.zeros(nb * N, Q, dtype=torch.int32), criterions_per_task=crit)
    a = SimpleNamespace(name_method="TIM-GD", iter=iters)
    parts = sharding.method_parts(a, m, {"acc": np.zeros((nb * N, 1), np.float32)}, nb, N, Q, torch.device("cpu"))
    assert parts["criterions"].shape == (nb, iters, N)
    assert np.array_equal(parts["criterions"][1].numpy(), crit[:, N:])
    empty = sharding.method_parts(a, None, None, 0, N, Q, torch.device("cpu"))
    assert empty["criterions"].shape == (0, iters, N)
    got = sharding.gather_packed(parts, nb)
    assert np.array_equal(got["criterions"].numpy(), parts["criterions"].numpy())


@pytest.mark.parametrize("name", NAMES)
def test_fixture_schema_and_margin(name):
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20
    g = tim_gd.load_fixture(GOLDEN, name)
    K, N, S, it = int(g["K"]), int(g["N"]), int(g["K"]) * int(g["shots"]), int(g["iters"])
    D = int(g["D"]) if "D" in g else K
    assert g["x_s"].shape == (N, S, D) and g["x_q"].shape == (N, 75, D)
    assert g["y_s"].shape == (N, S, 1) and g["y_q"].shape == (N, 75, 1)
    assert g["weights"].shape == (N, K, D) and g["weights"].dtype == np.float32
    assert g["logits_q"].shape == g["logits_q64"].shape == (N, 75, K) and g["logits_q64"].dtype == np.float64
    assert g["criterions"].shape == g["criterions64"].shape == (it, N) and g["acc"].shape == (N, 1)
    w64 = g["weights64"] if "weights64" in g else g["weights"].astype(np.float64) + g["weights64_minus_weights"]
    # the three bounds are the generator's formulas on the stored arrays (weights64 of a visual file is stored as a difference
    # rounded to fp32: that changes the gap by far less than 1e-9)
    assert float(g["weights_abs"]) == pytest.approx(max(1e-6, 2 * np.abs(g["weights"] - w64).max()), rel=1e-4)
    assert float(g["logits_abs"]) == max(2e-5, 2 * np.abs(g["logits_q"] - g["logits_q64"]).max())
    assert float(g["criterions_rel"]) == pytest.approx(max(1e-5, 2 * np.abs(g["criterions"].astype(np.float64) / g["criterions64"] - 1).max()), rel=1e-3)
    # every query's top-2 margin of the fp64 logits exceeds 4 * logits_abs: predictions within the bound cannot differ
    top2 = np.sort(g["logits_q64"], axis=2)[:, :, -2:]
    margin = (top2[:, :, 1] - top2[:, :, 0]).min()
    assert margin == float(g["min_logit_margin"]) and margin > 4 * float(g["logits_abs"])
    assert np.array_equal(g["logits_q"].argmax(2), g["logits_q64"].argmax(2))
    assert np.array_equal((g["logits_q"].argmax(2) == g["y_q"][:, :, 0]).astype(np.float32).mean(1, keepdims=True), g["acc"])


def test_fixtures_cover_both_loss_weight_settings():
    lw = {tuple(np.load(os.path.join(GOLDEN, n + ".npz"))["loss_weights"]) for n in tim_gd.PROB}
    assert {(1.0, 0.3, 1.0), (1.0, 1.0, 1.0)} <= lw


@pytest.mark.parametrize("name", tim_gd.PROB + tim_gd.VISUAL[:1])
def test_restatement_reproduces_reference(name):
    g = tim_gd.load_fixture(GOLDEN, name)
    if str(g["torch_version"]) != torch.__version__:
        pytest.skip("fixtures were made with another torch build")
    t = tim_gd.run_tim_gd(torch.from_numpy(g["x_q"]), torch.from_numpy(g["x_s"]), torch.from_numpy(g["y_s"]),
                          n_class=int(g["K"]), **tim_gd.params(g))
    tim_gd.check_within_bounds(t["weights"].numpy(), t["logits_q"].numpy(), t["criterions"].numpy(), g)
    assert np.array_equal(t["argmax"].numpy(), g["logits_q"].argmax(2))


def test_restatement_in_double_follows_the_fp64_trajectory():
    g = tim_gd.load_fixture(GOLDEN, tim_gd.PROB[0])
    if str(g["torch_version"]) != torch.__version__:
        pytest.skip("fixtures were made with another torch build")
    t = tim_gd.run_tim_gd(torch.from_numpy(g["x_q"]), torch.from_numpy(g["x_s"]), torch.from_numpy(g["y_s"]),
                          n_class=int(g["K"]), dtype=torch.float64, **tim_gd.params(g))
    assert t["weights"].dtype == torch.float64
    assert np.abs(t["logits_q"].numpy() - g["logits_q64"]).max() <= 1e-9
    assert np.abs(t["weights"].numpy() - g["weights64"]).max() <= 1e-11
