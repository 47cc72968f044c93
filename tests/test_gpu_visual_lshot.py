"""GPU: LAPLACIAN_SHOT on D-dim embeddings through engine.run_laplacian_shot_visual (tclip_laplacian_shot_visual_run: the row
length D carried separately from the class count K, the queries' pairwise distances by k_lshot_pairdist) - against the
reference's fixtures within the bounds each fixture carries (tests/golden/make_golden_visual_lshot.py: twice the reference's own
fp32-against-fp64 gap, never the HIP path's deviation), against the oracle's restatement at the kernel's tile and chunk edges,
against the probability-feature entry at D = K bit for bit, its argument checks and the NaN case.

Measured on MI355X (deviation from the reference's fp32 run / bound): see DESIGN.md section 8e."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import visual_fs, visual_lshot
from oracle import ref_torch

pytestmark = pytest.mark.gpu


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", visual_lshot.VISUAL)
def test_fixture(name):
    from tclip_amd import engine
    g = visual_lshot.load_fixture(GOLDEN, name)
    K, iters, knn = int(g["K"]), int(g["iters"]), int(g["knn"])
    unary, nbr, preds_iter, e = engine.run_laplacian_shot_visual(
        torch.from_numpy(g["x_q"]).cuda(), torch.from_numpy(g["x_s"]).cuda(), torch.from_numpy(g["y_s"]).cuda(), n_class=K,
        iters=iters, knn=knn, lmd=float(g["lmd"]), norm_type=str(g["norm_type"]))
    torch.cuda.synchronize()
    assert unary.shape == g["unary"].shape and nbr.shape == g["neighbours"].shape and preds_iter.shape == g["preds_iter"].shape
    du = float((np.abs(unary.cpu().numpy() - g["unary"]) / np.maximum(np.abs(g["unary"]), 1e-30)).max())
    de = float(np.abs(e.cpu().numpy() / g["ent_energy"] - 1).max())
    print(f"{name}: deviation from the reference: unary {du:.3e} relative (bound {float(g['unary_rel']):.3e}), energies {de:.3e} "
          f"relative (bound {float(g['energy_rel']):.3e})")
    # everything discrete is equal: the kNN graph, the final assignment and every per-update accuracy
    assert np.array_equal(np.sort(nbr.cpu().numpy(), axis=2), g["neighbours"]), "kNN graph differs"
    assert np.array_equal(preds_iter[:, -1].cpu().numpy(), g["preds_iter"][:, -1]), "final assignment differs"
    acc = (preds_iter.cpu().long() == torch.from_numpy(g["y_q"])[:, None, :]).float().mean(2).numpy()
    assert np.array_equal(acc, g["acc"]), "per-update accuracies differ"
    assert du <= float(g["unary_rel"]), f"unary term differs by {du:.2e} relative (bound {float(g['unary_rel']):.1e})"
    assert de <= float(g["energy_rel"]), f"energies differ by {de:.2e} relative (bound {float(g['energy_rel']):.1e})"


# ---- 2. the kernels' edges against the oracle's restatement -------------------------------------------------------------
# (D, K, shots, knn): D below one 64-feature LDS chunk and no multiple of 4; one partial chunk of 128-bit loads; K > D and a
# scalar-load chunk; three chunks, the last one partial; whole chunks; one below the limit (scalar loads, a 63-feature tail);
# the limit.  Q = 75: three row tiles of 32, the last one of 11 rows.
SWEEP = [(5, 3, 1, 2), (16, 10, 4, 3), (33, 65, 1, 5), (130, 37, 2, 7), (512, 10, 4, 3), (1023, 5, 1, 3), (1024, 6, 2, 3)]


@pytest.mark.parametrize("norm_type", ["L2N", "UN"])
@pytest.mark.parametrize("D,K,shots,knn", SWEEP)
def test_shape_sweep_matches_restatement(D, K, shots, knn, norm_type):
    """fresh seeded inputs, T = 3, 15 updates.  Neighbour lists and the final assignment are equal; the energies agree to 1e-6
    relative (the bound of tests/test_laplacian_shot.py for the same comparison).  The unary term: both sides are fp32 results
    of at most 1024-term sums - the restatement's pairwise fp32 sum, square root and square carry up to log2(D) + 3 = 13
    roundings of 2^-24 (8e-7 relative), and a one-ulp difference in a normalised row or a prototype moves
    ||p - z||^2 by up to 2 * 2^-24 * (|p| + |z|) * |p - z|, which is 2.4e-7 * max|row|^2 where the distance is of the rows' own
    size and an absolute 2.4e-7 * max|row|^2 where it is not: rtol 5e-6, atol 1e-6 * max|row|^2 cover twice that."""
    from tclip_amd import engine
    x_s, y_s, x_q = visual_fs.random_tasks(3, K, D, shots, seed=D * 1019 + K, scale=1.0 / D ** 0.5)
    margin = visual_lshot.knn_margin(x_q, knn, norm_type)
    print(f"D={D} K={K} knn={knn} {norm_type}: restated kNN margin {margin:.3e}")
    if margin < 1e-6:
        pytest.skip("the (knn-1)-th and knn-th neighbour of a query are closer than 1e-6 relative: the lists may differ")
    prm = dict(n_class=K, iters=15, knn=knn, lmd=0.7, norm_type=norm_type)
    unary, nbr, preds_iter, e = engine.run_laplacian_shot_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), **prm)
    torch.cuda.synchronize()
    assert unary.shape == (3, 75, K) and nbr.shape == (3, 75, knn - 1) and preds_iter.shape == (3, 15, 75) and e.shape == (3, 15)
    t = ref_torch.run_laplacian_shot(x_q, x_s, y_s, torch.zeros(3, 75, dtype=torch.long), **prm)
    scale2 = 1.0 if norm_type == "L2N" else float(torch.cat([x_s, x_q], 1).square().sum(2).max())
    du = float(np.abs(unary.cpu().numpy() - t["unary"]).max())
    de = float(np.abs(e.cpu().numpy() / t["ent_energy"] - 1).max())
    print(f"  unary {du:.3e} absolute (values up to {float(t['unary'].max()):.3f}), energies {de:.3e} relative")
    assert np.array_equal(np.sort(nbr.cpu().numpy(), axis=2), t["neighbours"]), "kNN graph differs"
    assert np.array_equal(preds_iter[:, -1].cpu().numpy(), t["preds"]), "final assignment differs"
    assert np.allclose(unary.cpu().numpy(), t["unary"], rtol=5e-6, atol=1e-6 * scale2)
    assert np.allclose(e.cpu().numpy(), t["ent_energy"], rtol=1e-6, atol=0)
    assert int(nbr.min()) >= 0 and int(nbr.max()) < 75 and int(preds_iter.min()) >= 0 and int(preds_iter.max()) < K


# ---- 3. D = K: the probability-feature entry, bit for bit ---------------------------------------------------------------

def test_width_equal_to_class_count_equals_the_probability_entry():
    """the inputs of test_engine_equals_oracle_on_fresh_tasks (tests/test_laplacian_shot.py): k_lshot_pairdist sums in the order
    of k_lshot_task's own loop, so the two entries agree in every bit"""
    from tclip_amd import engine, synth
    K, N, shots = 21, 6, 2
    x_q, _ = synth.make_query_tasks(N, K, seed=91, k_eff=4)
    x_s, y_s = synth.make_support(N, K, shots, seed=91)
    x_q, x_s, y_s = x_q.cuda(), x_s.cuda(), y_s.squeeze(2).cuda()
    for knn, lmd, norm in ((3, 0.7, "L2N"), (6, 2.0, "UN"), (2, 0.1, "L2N")):
        a = engine.run_laplacian_shot(x_q, x_s, y_s, iters=15, knn=knn, lmd=lmd, norm_type=norm)
        b = engine.run_laplacian_shot_visual(x_q, x_s, y_s, n_class=K, iters=15, knn=knn, lmd=lmd, norm_type=norm)
        torch.cuda.synchronize()
        for name, u, v in zip(("unary", "neighbours", "preds_iter", "energies"), a, b):
            assert torch.equal(u, v), f"{name} differs (knn {knn}, {norm})"


# ---- 4. arguments: refused before any launch ---------------------------------------------------------------------------

def test_argument_errors():
    from tclip_amd import engine
    x_s, y_s, x_q = visual_fs.random_tasks(2, 6, 32, 1, seed=1)
    x_s, y_s, x_q = x_s.cuda(), y_s.cuda(), x_q.cuda()
    ok = dict(n_class=6, iters=3, knn=3, lmd=0.7)
    with pytest.raises((RuntimeError, ValueError), match="dim"):
        engine.run_laplacian_shot_visual(x_q[:, :, :0], x_s[:, :, :0], y_s, **ok)
    wide = torch.zeros(2, 75, 1025, device="cuda"), torch.zeros(2, 6, 1025, device="cuda")
    with pytest.raises((RuntimeError, ValueError), match="dim"):
        engine.run_laplacian_shot_visual(wide[0], wide[1], y_s, **ok)
    with pytest.raises(RuntimeError, match="knn"):
        engine.run_laplacian_shot_visual(x_q, x_s, y_s, **dict(ok, knn=1))
    with pytest.raises(RuntimeError, match="iters"):
        engine.run_laplacian_shot_visual(x_q, x_s, y_s, **dict(ok, iters=0))
    bad = y_s.clone()
    bad[1, 2] = 6
    with pytest.raises(ValueError, match="label outside"):
        engine.run_laplacian_shot_visual(x_q, x_s, bad, **ok)
    with pytest.raises(ValueError, match="norm_type"):
        engine.run_laplacian_shot_visual(x_q, x_s, y_s, norm_type="CL2N", **ok)
    unary, nbr, preds_iter, e = engine.run_laplacian_shot_visual(x_q, x_s, y_s, **ok)      # and the arguments are fine otherwise
    torch.cuda.synchronize()
    assert bool(torch.isfinite(unary).all()) and bool(torch.isfinite(e).all()) and nbr.shape == (2, 75, 2)


# ---- 5. a zero row ------------------------------------------------------------------------------------------------------

def test_nan_features_stay_in_bounds():
    """A zero query row has no L2 norm: its distances are NaN in the reference too.  The call must come back (neighbour lists
    inside the task, assignments inside 0..K-1) and leave the other tasks untouched."""
    from tclip_amd import engine
    K, N, D = 12, 3, 64
    x_s, y_s, x_q, _ = visual_fs.make_tasks(N, K, D, 2, seed=5)
    prm = dict(n_class=K, iters=10, knn=3, lmd=0.7)
    clean = engine.run_laplacian_shot_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), **prm)
    x_bad = x_q.clone()
    x_bad[1, 7] = 0.0
    unary, nbr, preds_iter, e = engine.run_laplacian_shot_visual(x_bad.cuda(), x_s.cuda(), y_s.cuda(), **prm)
    torch.cuda.synchronize()
    assert int(nbr.min()) >= 0 and int(nbr.max()) < 75 and int(preds_iter.min()) >= 0 and int(preds_iter.max()) < K
    for k in (0, 2):
        assert torch.equal(preds_iter[k], clean[2][k]) and torch.equal(e[k], clean[3][k]) and torch.equal(nbr[k], clean[1][k])
