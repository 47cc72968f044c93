"""GPU: ALPHA_TIM on D-dim embeddings through engine.run_alpha_tim_visual (tclip_alpha_tim_visual_run: tim_loop with the row
length D carried separately from the class count K, per-batch criterions, selectable entropies) - against the reference's
fixtures within the bounds each fixture carries (tests/golden/make_golden_visual_alpha_tim.py: twice the reference's own
fp32-against-fp64 gap, never the HIP path's deviation), against a torch-autograd restatement at the GEMM tiles' edges with
both entropy triples and two orders, and against the probability-feature entry at D = K bit for bit.

Measured on MI355X (deviation from the reference's fp32 run / bound): see DESIGN.md section 8e."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import alpha_tim, visual_fs

pytestmark = pytest.mark.gpu


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", alpha_tim.VISUAL)
def test_fixture(name):
    from tclip_amd import engine
    g = alpha_tim.load_fixture(GOLDEN, name)
    w, lq, preds, crit = engine.run_alpha_tim_visual(torch.from_numpy(g["x_q"]).cuda(), torch.from_numpy(g["x_s"]).cuda(),
                                                     torch.from_numpy(g["y_s"]).cuda(), n_class=int(g["K"]), **alpha_tim.params(g))
    torch.cuda.synchronize()
    assert w.shape == g["weights"].shape and lq.shape == g["logits_q"].shape and crit.shape == (1, int(g["iters"]))
    w_err = float(np.abs(w.cpu().numpy() - g["weights"]).max())
    l_err = float(np.abs(lq.cpu().numpy() - g["logits_q"]).max())
    c_err = float(np.abs(crit[0].cpu().numpy() / g["criterions"] - 1).max())
    print(f"{name}: deviation from the reference: weights {w_err:.3e} (bound {float(g['weights_abs']):.3e}), logits {l_err:.3e} "
          f"(bound {float(g['logits_abs']):.3e}), criterions {c_err:.3e} relative (bound {float(g['criterions_rel']):.3e})")
    assert w_err <= float(g["weights_abs"]), f"weights differ by {w_err} (bound {float(g['weights_abs'])})"
    assert l_err <= float(g["logits_abs"]), f"query logits differ by {l_err} (bound {float(g['logits_abs'])})"
    assert c_err <= float(g["criterions_rel"]), f"criterions differ by {c_err} relative (bound {float(g['criterions_rel'])})"
    # everything discrete is equal: every prediction and every accuracy
    assert np.array_equal(preds.cpu().numpy(), g["logits_q"].argmax(2)), "predictions differ from the reference's"
    acc = (preds.cpu().long() == torch.from_numpy(g["y_q"])).float().mean(1, keepdim=True).numpy()
    assert np.array_equal(acc, g["acc"]), "accuracies differ from the reference's"


# ---- 2. the GEMMs' edges against the torch restatement, every entropy branch --------------------------------------------
# (D, K, shots): depth below one 16-slice and one partial tile; a small case; depth and classes one past a boundary (K > D);
# D > K with a depth that is no multiple of 16; a long row
SWEEP = [(5, 3, 1), (16, 10, 4), (33, 65, 1), (130, 37, 2), (512, 10, 4)]


@pytest.mark.parametrize("alpha_value", [2.0, 7.0])
@pytest.mark.parametrize("entropies", [("Shannon", "Alpha", "Alpha"), ("Alpha", "Alpha", "Alpha")], ids=["SAA", "AAA"])
@pytest.mark.parametrize("D,K,shots", SWEEP)
def test_shape_sweep_matches_torch(D, K, shots, entropies, alpha_value):
    """fresh seeded inputs, 30 Adam steps at lr 1e-3, four tasks in one batch; the bounds test_gpu_tim_gd.py uses for the same
    comparison: weights 5e-4, logits 5e-2, criterions 1 %.  Rows of norm about 0.3: the reference's Alpha cross-entropy
    multiplies the zeros of the one-hot labels with (p + 1e-12)^(1 - alpha), which is infinite in fp32 once a support row's
    probability of ANY class falls under 4e-7 at alpha = 7 - the loss is then NaN in the reference itself, and on rows of norm 1
    at temp 15 that is the common case; short rows keep every class probability of a support row above it."""
    from tclip_amd import engine
    x_s, y_s, x_q = visual_fs.random_tasks(4, K, D, shots, seed=D * 1019 + K, scale=0.3 / D ** 0.5)
    prm = dict(n_class=K, iters=30, temp=15.0, lr=1e-3, alpha_value=alpha_value, entropies=entropies, loss_weights=[1.0, 1.0, 1.0])
    w, lq, preds, crit = engine.run_alpha_tim_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), **prm)
    torch.cuda.synchronize()
    assert w.shape == (4, K, D) and lq.shape == (4, 75, K) and preds.shape == (4, 75) and crit.shape == (1, 30)
    t = alpha_tim.run_alpha_tim(x_q, x_s, y_s, **prm)
    assert bool(torch.isfinite(t["weights"]).all()) and bool(torch.isfinite(t["criterions"]).all())
    w_err, l_err = float((w.cpu() - t["weights"]).abs().max()), float((lq.cpu() - t["logits_q"]).abs().max())
    c_err = float((crit[0].cpu() / t["criterions"] - 1).abs().max())
    print(f"D={D} K={K} shots={shots} {entropies[0]}/{entropies[1]}/{entropies[2]} alpha={alpha_value}: weights {w_err:.3e}, "
          f"logits {l_err:.3e}, criterions {c_err:.3e} relative")
    assert w_err < 5e-4 and l_err < 5e-2
    torch.testing.assert_close(crit[0].cpu(), t["criterions"], rtol=1e-2, atol=1e-7)
    assert torch.equal(preds.cpu().long(), lq.cpu().argmax(2))


# ---- 3. D = K: the probability-feature entry, bit for bit ---------------------------------------------------------------

def test_width_equal_to_class_count_equals_the_probability_entry():
    from tclip_amd import engine
    g = np.load(os.path.join(GOLDEN, "fs_tim_K37_N2_s3_a2.npz"))
    x_q, x_s = torch.from_numpy(g["x_q"]).cuda(), torch.from_numpy(g["x_s"]).cuda()
    y_s = torch.from_numpy(g["y_s"]).squeeze(2).cuda()
    prm = dict(iters=40, temp=float(g["temp"]), lr=float(g["lr"]), alpha_value=float(g["alpha_value"]),
               loss_weights=[float(v) for v in g["loss_weights"]], entropies=[str(e) for e in g["entropies"]], n_batches=2)
    a = engine.run_alpha_tim(x_q, x_s, y_s, **prm)
    b = engine.run_alpha_tim_visual(x_q, x_s, y_s, n_class=int(g["K"]), **prm)
    torch.cuda.synchronize()
    for name, u, v in zip(("weights", "logits_q", "preds", "criterions"), a, b):
        assert torch.equal(u, v), f"{name} differs"
    assert a[3].shape == (2, 40) and bool(torch.isfinite(a[0]).all())


# ---- 4. arguments: refused before any launch ---------------------------------------------------------------------------

def test_argument_errors():
    from tclip_amd import engine
    x_s, y_s, x_q = visual_fs.random_tasks(2, 6, 32, 1, seed=1)
    x_s, y_s, x_q = x_s.cuda(), y_s.cuda(), x_q.cuda()
    ok = dict(n_class=6, iters=3, temp=15.0, lr=1e-4, alpha_value=7.0)
    with pytest.raises((RuntimeError, ValueError), match="iters"):
        engine.run_alpha_tim_visual(x_q, x_s, y_s, **dict(ok, iters=0))
    with pytest.raises((RuntimeError, ValueError), match="dim"):
        engine.run_alpha_tim_visual(x_q[:, :, :0], x_s[:, :, :0], y_s, **ok)
    wide = torch.zeros(2, 75, 1025, device="cuda"), torch.zeros(2, 6, 1025, device="cuda")
    with pytest.raises((RuntimeError, ValueError), match="dim"):
        engine.run_alpha_tim_visual(wide[0], wide[1], y_s, **ok)
    with pytest.raises((RuntimeError, ValueError), match="n_support"):
        engine.run_alpha_tim_visual(x_q, x_s[:, :0], y_s[:, :0], **ok)
    with pytest.raises(RuntimeError, match="alpha_value"):
        engine.run_alpha_tim_visual(x_q, x_s, y_s, **dict(ok, alpha_value=1.0))
    bad = y_s.clone()
    bad[1, 2] = 6
    with pytest.raises(ValueError, match="label outside"):
        engine.run_alpha_tim_visual(x_q, x_s, bad, **ok)
    w, lq, preds, crit = engine.run_alpha_tim_visual(x_q, x_s, y_s, **ok)        # and the arguments above are fine otherwise
    torch.cuda.synchronize()
    assert bool(torch.isfinite(w).all()) and crit.shape == (1, 3)
