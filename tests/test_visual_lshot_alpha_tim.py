"""CPU: the host side of ALPHA_TIM and LAPLACIAN_SHOT on visual features at the engine level - the four C entries in the header,
the binding and the library, the signatures of engine.run_*_visual, the fixtures' input digests and the conditions each
fixture's generator stored with it (tests/golden/make_golden_visual_lshot.py, make_golden_visual_alpha_tim.py)."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden_names
from helpers import visual_fs

ENTRIES = ("tclip_alpha_tim_visual_workspace_bytes", "tclip_alpha_tim_visual_run", "tclip_laplacian_shot_visual_workspace_bytes",
           "tclip_laplacian_shot_visual_run")
LSHOT = ["fs_vis_lshot_D512_K10_S4_N3", "fs_vis_lshot_D1024_K37_S2_N2", "fs_vis_lshot_D768_K100_S1_N1_un"]
ALPHA_TIM = ["fs_vis_alpha_tim_D512_K10_S4_N3", "fs_vis_alpha_tim_D1024_K37_S2_N2", "fs_vis_alpha_tim_D768_K100_S1_N1"]


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_entries_in_header_and_binding():
    from tclip_amd import _capi
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    later = header[header.index("later, without a new number"):header.index("#define TCLIP_ABI_VERSION")]
    for name in ENTRIES:
        assert name + "(" in header and name in later and name in _capi.EXPORTS
    assert "#define TCLIP_ABI_VERSION 5" in header


def test_entries_exported_by_the_library():
    from tclip_amd import _capi
    assert os.path.exists(_capi.LIB_PATH), "libtclip.so is missing: run build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= exported


def test_engine_signatures():
    from tclip_amd import engine

    def names(fn):
        p = inspect.signature(fn).parameters
        return ([n for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD], {n for n, v in p.items() if v.kind is v.KEYWORD_ONLY},
                {n: v.default for n, v in p.items() if v.default is not v.empty})
    pos, kw, default = names(engine.run_alpha_tim_visual)
    assert pos == ["x_q", "x_s", "y_s"]
    assert kw == {"n_class", "iters", "temp", "lr", "alpha_value", "loss_weights", "entropies", "n_batches"}
    assert default["n_batches"] == 1 and "n_class" not in default
    pos, kw, default = names(engine.run_laplacian_shot_visual)
    assert pos == ["x_q", "x_s", "y_s"] and kw == {"n_class", "iters", "knn", "lmd", "norm_type"}
    assert default == {"norm_type": "L2N"}


def test_engine_refuses_before_any_launch():
    """what the two calls refuse on the host, before a device is needed"""
    from tclip_amd import engine
    x = torch.zeros(1, 75, 16)
    with pytest.raises(ValueError, match="norm_type"):
        engine.run_laplacian_shot_visual(x, x[:, :4], torch.zeros(1, 4, dtype=torch.long), n_class=4, iters=3, knn=3, lmd=0.7,
                                         norm_type="CL2N")
    with pytest.raises(ValueError, match="Entropies"):
        engine.run_alpha_tim_visual(x, x[:, :4], torch.zeros(1, 4, dtype=torch.long), n_class=4, iters=3, temp=15, lr=1e-4,
                                    alpha_value=7.0, entropies=("Shannon", "Renyi", "Alpha"))
    with pytest.raises(RuntimeError, match="GPU"):
        engine.run_laplacian_shot_visual(x, x[:, :4], torch.zeros(1, 4, dtype=torch.long), n_class=4, iters=3, knn=3, lmd=0.7)


@pytest.mark.parametrize("name", LSHOT + ALPHA_TIM)
def test_fixture_inputs_regenerate(name):
    g = _load(name)
    N, K, D, shots = int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"])
    x_s, y_s, x_q, y_q = visual_fs.make_tasks(N, K, D, shots, int(g["seed"]), signal=float(g["signal"]))
    assert x_s.shape == (N, K * shots, D) and x_q.shape == (N, 75, D) and D != K
    for k, a in (("x_s", x_s), ("x_q", x_q), ("y_s", y_s), ("y_q", y_q)):
        assert visual_fs.sha(a.numpy()) == str(g[k + "_sha1"]), k
    assert np.array_equal(g["y_s"], y_s.numpy()) and np.array_equal(g["y_q"], y_q.numpy())
    assert 1 <= int(g["seeds_tried"]) <= 20
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20


def test_fixture_names_stay_out_of_the_other_globs():
    for n in LSHOT + ALPHA_TIM:
        assert n not in golden_names("") and n not in golden_names("fs_lshot_") and n not in golden_names("fs_tim_")
    assert set(golden_names("fs_vis_lshot_")) == set(LSHOT) and set(golden_names("fs_vis_alpha_tim_")) == set(ALPHA_TIM)


@pytest.mark.parametrize("name", LSHOT)
def test_lshot_fixture_satisfies_its_conditions(name):
    g = _load(name)
    N, K, iters, knn = int(g["N"]), int(g["K"]), int(g["iters"]), int(g["knn"])
    assert bool(g["fp32_equals_fp64_neighbours"]) and bool(g["fp32_equals_fp64_assignments"]) and bool(g["fp32_equals_fp64_freeze"])
    assert float(g["knn_margin"]) > 1e-6
    assert g["neighbours"].shape == (N, 75, knn - 1) and g["unary"].shape == (N, 75, K) and g["unary"].dtype == np.float32
    assert g["preds_iter"].shape == (N, iters, 75) and g["acc"].shape == (N, iters) and g["ent_energy"].shape == (N, iters)
    assert g["ent_energy"].dtype == np.float64
    # the bounds are the generator's formula on the stored fp64 results, and nothing wider
    unary64 = g["unary"].astype(np.float64) + g["unary64_minus_unary"]
    gap_u = float(np.abs(g["unary"] / unary64 - 1).max())
    gap_e = float(np.abs(g["ent_energy"] / g["ent_energy64"] - 1).max())
    assert gap_u == pytest.approx(float(g["unary_gap"]), rel=1e-3, abs=1e-12) and gap_e == pytest.approx(float(g["energy_gap"]), rel=1e-6, abs=1e-15)
    assert float(g["unary_rel"]) == max(1e-6, 2 * float(g["unary_gap"])) and float(g["energy_rel"]) == max(1e-7, 2 * float(g["energy_gap"]))
    # the accuracies are those of the stored assignments, the energies repeat from the freeze iteration on
    assert np.array_equal((g["preds_iter"] == g["y_q"][:, None, :]).astype(np.float32).mean(2), g["acc"])
    for n, it in enumerate(g["freeze_iter"]):
        assert np.all(g["ent_energy"][n, it:] == g["ent_energy"][n, min(it, iters - 1)])
    assert 0 <= g["preds_iter"].min() and g["preds_iter"].max() < K and any(0.0 < a < 1.0 for a in g["acc"][:, -1])


def test_lshot_fixtures_cover_what_the_issue_names():
    g = {n: _load(n) for n in LSHOT}
    assert int(g[LSHOT[1]]["knn"]) == 7 and float(g[LSHOT[1]]["lmd"]) != float(g[LSHOT[0]]["lmd"])
    assert {str(v["norm_type"]) for v in g.values()} == {"L2N", "UN"} and str(g[LSHOT[2]]["norm_type"]) == "UN"


@pytest.mark.parametrize("name", ALPHA_TIM)
def test_alpha_tim_fixture_satisfies_its_conditions(name):
    g = _load(name)
    N, K, D, iters = int(g["N"]), int(g["K"]), int(g["D"]), int(g["iters"])
    assert g["weights"].shape == (N, K, D) and g["logits_q"].shape == (N, 75, K) and g["criterions"].shape == (iters,)
    assert 40 <= iters <= 100
    top2 = np.sort(g["logits_q64"], axis=2)[:, :, -2:]
    margin = float((top2[:, :, 1] - top2[:, :, 0]).min())
    assert margin == pytest.approx(float(g["min_logit_margin"]), rel=1e-12) and margin > 4 * float(g["logits_abs"])
    assert np.array_equal(g["logits_q"].argmax(2), g["logits_q64"].argmax(2))
    assert np.array_equal((g["logits_q"].argmax(2) == g["y_q"]).astype(np.float32).mean(1, keepdims=True), g["acc"])
    # the bounds are the generator's formula on the stored fp64 results, and nothing wider
    gaps = (float(np.abs(g["weights64_minus_weights"]).max()), float(np.abs(g["logits_q"] - g["logits_q64"]).max()),
            float(np.abs(g["criterions"] / g["criterions64"] - 1).max()))
    assert gaps[0] == pytest.approx(float(g["weights_gap"]), rel=1e-3) and gaps[1] == pytest.approx(float(g["logits_gap"]), rel=1e-6)
    assert gaps[2] == pytest.approx(float(g["criterions_gap"]), rel=1e-2, abs=1e-7)
    assert float(g["weights_abs"]) == max(1e-6, 2 * float(g["weights_gap"]))
    assert float(g["logits_abs"]) == max(2e-5, 2 * float(g["logits_gap"]))
    assert float(g["criterions_rel"]) == max(1e-5, 2 * float(g["criterions_gap"]))


def test_alpha_tim_fixtures_cover_what_the_issue_names():
    g = _load(ALPHA_TIM[1])
    assert list(g["entropies"]) == ["Shannon"] * 3 and int(g["iters"]) == 60
    assert any("Alpha" in list(_load(n)["entropies"]) for n in ALPHA_TIM)


def test_restatements_run_on_the_host():
    """what the GPU sweeps compare against: shapes at D != K, and ALPHA_TIM's restatement equal to TIM_GD's where the two
    methods coincide up to the marginal entropy's 1e-12 and the criterion's mean"""
    from helpers import alpha_tim, visual_lshot
    from oracle import ref_torch
    x_s, y_s, x_q = visual_fs.random_tasks(2, 5, 33, 2, seed=1, scale=1.0 / 33 ** 0.5)
    t = alpha_tim.run_alpha_tim(x_q, x_s, y_s, n_class=5, iters=4, temp=15.0, lr=1e-3, alpha_value=2.0,
                                entropies=("Shannon", "Alpha", "Alpha"))
    assert t["weights"].shape == (2, 5, 33) and t["logits_q"].shape == (2, 75, 5) and t["criterions"].shape == (4,)
    r = ref_torch.run_laplacian_shot(x_q, x_s, y_s, torch.zeros(2, 75, dtype=torch.long), n_class=5, iters=5, knn=3, lmd=0.7)
    assert r["unary"].shape == (2, 75, 5) and r["neighbours"].shape == (2, 75, 2) and r["ent_energy"].shape == (2, 5)
    assert visual_lshot.knn_margin(x_q, 3, "L2N") > 0
