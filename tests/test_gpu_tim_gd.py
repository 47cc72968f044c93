"""GPU: TIM_GD (reference: src/methods/few_shot/tim.py:90-189) on probability features and on D-dim embeddings - the HIP
path (closed-form gradient, the GEMMs with the row length D carried separately from the class count K) against the reference's
fixtures within the bounds each fixture carries (tests/golden/make_golden_tim_gd.py: twice the reference's own fp32-against-
fp64 gap, never the HIP path's deviation), against the torch restatement at the GEMM tiles' edges, against itself at two
launch shapes, its argument checks, and the evaluator's task-batch loop.

Measured on MI355X (deviation from the reference's fp32 run / bound): see DESIGN.md section 8d."""
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import tim_gd, visual_fs

pytestmark = pytest.mark.gpu


def _args(K, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=30, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, use_softmax_feature=True, temp=15,
                loss_weights=[1.0, 0.3, 1.0], lr_tim=1e-4, name_method="TIM-GD")
    a.update(kw)
    return a


# ---- 1. the reference's fixtures, through the drop-in class -----------------------------------------------------------

@pytest.mark.parametrize("name", tim_gd.PROB + tim_gd.VISUAL)
def test_fixture_drop_in(name):
    from src.methods.few_shot.tim import TIM_GD
    g = tim_gd.load_fixture(GOLDEN, name)
    K, prm = int(g["K"]), tim_gd.params(g)
    a = _args(K, iter=prm["iters"], temp=prm["temp"], loss_weights=prm["loss_weights"], lr_tim=prm["lr"], shots=int(g["shots"]),
              use_softmax_feature=name in tim_gd.PROB)
    m = TIM_GD(model=None, device=torch.device("cuda:0"), log_file=None, args=a)
    logs = m.run_task(task_dic={"x_q": torch.from_numpy(g["x_q"]), "y_q": torch.from_numpy(g["y_q"]),
                                "x_s": torch.from_numpy(g["x_s"]), "y_s": torch.from_numpy(g["y_s"])}, shot=int(g["shots"]))
    assert m.weights.shape == g["weights"].shape and m.logits_q.shape == g["logits_q"].shape
    assert logs["criterions"].shape == g["criterions"].shape and logs["criterions"].dtype == np.float32
    assert logs["acc"].shape == g["acc"].shape
    tim_gd.check_within_bounds(m.weights.cpu().numpy(), m.logits_q.cpu().numpy(), logs["criterions"], g)
    # everything discrete is equal: every prediction and every accuracy
    assert np.array_equal(m.preds.cpu().numpy(), g["logits_q"].argmax(2)), "predictions differ from the reference's"
    assert np.array_equal(logs["acc"], g["acc"]), "accuracies differ from the reference's"


# ---- 2. the GEMMs' edges against the torch restatement -----------------------------------------------------------------
# (D, K, shots): depth below one 16-slice and one partial tile; a small case; depth and classes one past a boundary; D > K with
# a depth that is no multiple of 16; exact tiles with D < K; a long row
SWEEP = [(5, 3, 1), (16, 10, 4), (33, 65, 1), (130, 37, 2), (96, 128, 1), (512, 10, 4)]


@pytest.mark.parametrize("D,K,shots", SWEEP)
def test_shape_sweep_matches_torch(D, K, shots):
    """fresh seeded inputs, 30 Adam steps, two batches in one call; the tolerances of test_engine_close_to_oracle_on_fresh_tasks
    (tests/test_alpha_tim.py): weights 5e-4, logits 5e-2, criterions 1 %"""
    from tclip_amd import engine
    x_s, y_s, x_q = visual_fs.random_tasks(4, K, D, shots, seed=D * 1019 + K, scale=1.0 / D ** 0.5)
    prm = dict(n_class=K, iters=30, temp=15.0, lr=1e-3, loss_weights=[1.0, 0.7, 1.2])
    w, lq, preds, crit = engine.run_tim_gd(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_batches=2, **prm)
    torch.cuda.synchronize()
    assert w.shape == (4, K, D) and lq.shape == (4, 75, K) and preds.shape == (4, 75) and crit.shape == (30, 4)
    t = tim_gd.run_tim_gd(x_q, x_s, y_s, **prm)
    w_err, l_err = float((w.cpu() - t["weights"]).abs().max()), float((lq.cpu() - t["logits_q"]).abs().max())
    c_err = float((crit.cpu() / t["criterions"] - 1).abs().max())
    print(f"D={D} K={K} shots={shots}: weights {w_err:.3e}, logits {l_err:.3e}, criterions {c_err:.3e} relative")
    assert w_err < 5e-4 and l_err < 5e-2
    torch.testing.assert_close(crit.cpu(), t["criterions"], rtol=1e-2, atol=1e-7)
    assert torch.equal(preds.cpu().long(), lq.cpu().argmax(2))


# ---- 3. D = K: the per-task reduction against itself -------------------------------------------------------------------

def test_width_equal_to_class_count_per_task_criterions():
    from tclip_amd import engine, synth
    K, N, shots = 21, 4, 2
    x_q, _ = synth.make_query_tasks(N, K, seed=77, k_eff=4)
    x_s, y_s = synth.make_support(N, K, shots, seed=77)
    prm = dict(n_class=K, iters=40, temp=15.0, lr=1e-3, loss_weights=[1.0, 0.7, 1.2])
    w, lq, preds, crit = engine.run_tim_gd(x_q.cuda(), x_s.cuda(), y_s.squeeze(2).cuda(), n_batches=2, **prm)
    assert crit.shape == (40, N) and bool(torch.isfinite(crit).all()) and bool((crit > 0).all())
    for b in range(2):       # one task per batch, the two tasks of batch b: other grids for every kernel of the loop
        sl = slice(2 * b, 2 * b + 2)
        _, _, _, c1 = engine.run_tim_gd(x_q[sl].cuda(), x_s[sl].cuda(), y_s[sl].squeeze(2).cuda(), n_batches=2, **prm)
        torch.testing.assert_close(crit[:, sl].mean(1).cpu(), c1.mean(1).cpu(), rtol=1e-6, atol=0.0)
    assert torch.equal(preds.cpu().long(), lq.cpu().argmax(2))


# ---- 4. arguments: refused before any launch ---------------------------------------------------------------------------

def test_argument_errors():
    from tclip_amd import engine
    x_s, y_s, x_q = visual_fs.random_tasks(2, 6, 32, 1, seed=1)
    x_s, y_s, x_q = x_s.cuda(), y_s.cuda(), x_q.cuda()
    ok = dict(n_class=6, iters=3, temp=15.0, lr=1e-4)
    with pytest.raises((RuntimeError, ValueError), match="iters"):
        engine.run_tim_gd(x_q, x_s, y_s, **dict(ok, iters=0))
    with pytest.raises((RuntimeError, ValueError), match="dim"):
        engine.run_tim_gd(x_q[:, :, :0], x_s[:, :, :0], y_s, **ok)
    wide = torch.zeros(2, 75, 1025, device="cuda"), torch.zeros(2, 6, 1025, device="cuda")
    with pytest.raises((RuntimeError, ValueError), match="dim"):
        engine.run_tim_gd(wide[0], wide[1], y_s, **ok)
    with pytest.raises((RuntimeError, ValueError), match="n_support"):
        engine.run_tim_gd(x_q, x_s[:, :0], y_s[:, :0], **ok)
    bad = y_s.clone()
    bad[1, 2] = 6
    with pytest.raises(ValueError, match="label outside"):
        engine.run_tim_gd(x_q, x_s, bad, **ok)
    w, lq, preds, crit = engine.run_tim_gd(x_q, x_s, y_s, **ok)        # and the arguments above are fine otherwise
    torch.cuda.synchronize()
    assert bool(torch.isfinite(w).all()) and crit.shape == (3, 2)


# ---- 5. the evaluator's task-batch loop --------------------------------------------------------------------------------

@pytest.mark.parametrize("visual", [False, True])
def test_evaluator_equals_the_class_on_materialised_tasks(visual):
    from src.eval_few_shot import Evaluator_few_shot, relabel_batch
    from src.methods.few_shot.tim import TIM_GD
    from tclip_amd import synth
    K, seed = 10, 5300
    if visual:
        feats_s, labels_s, feats_q, labels_q = visual_fs.make_tables(K, 96, 40, seed, signal=0.3)
    else:
        feats_s, labels_s = synth.make_feature_table(K, 40, seed=seed)
        feats_q, labels_q = synth.make_feature_table(K, 40, seed=seed + 1)
    a = _args(K, number_tasks=4, batch_size=2, shots=2, iter=30, used_test_set="test", dataset="synthetic", tunable=False,
              use_softmax_feature=not visual, lr_tim=1e-3)
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    dev = torch.device("cuda", 0)
    ev = Evaluator_few_shot(device=dev, args=a, log_file=None)
    s_idx, q_idx = ev.sample_indices(labels_s.numpy(), labels_q.numpy())
    assert s_idx.shape == (2, 2, K * 2) and q_idx.shape == (2, 2, 75)
    acc, _ = ev.evaluate_tasks(None, feats_s, labels_s, feats_q, labels_q, indices=(s_idx, q_idx))
    assert type(ev.last_method) is TIM_GD
    assert ev.last_task_accuracies.shape == (2, 2) and ev.last_batch_criterions.shape == (2, 30, 2)
    # the same tasks, materialised here as Tasks_Generator_few_shot.get_task builds them, through the class alone
    si, qi = s_idx.reshape(-1), q_idx.reshape(-1)
    x_s, x_q = feats_s[si].view(4, K * 2, -1), feats_q[qi].view(4, 75, -1)
    x_s, x_q, y_s, y_q = relabel_batch(x_s, x_q, labels_s[si].view(4, -1), labels_q[qi].view(4, 75), not visual)
    m = TIM_GD(model=None, device=dev, log_file=None, args=a)
    logs = m.run_task({"x_s": x_s, "x_q": x_q, "y_s": y_s.unsqueeze(2), "y_q": y_q.unsqueeze(2)}, shot=2)
    assert logs["acc"].shape == (4, 1) and logs["criterions"].shape == (30, 4)
    assert np.array_equal(ev.last_task_accuracies.reshape(-1), logs["acc"][:, 0])
    assert np.array_equal(ev.last_batch_criterions.transpose(1, 0, 2).reshape(30, 4), logs["criterions"])
    assert 0 < float(acc) <= 1 and float(acc) == pytest.approx(float(logs["acc"].reshape(2, 2).mean(1).mean()), abs=1e-6)
