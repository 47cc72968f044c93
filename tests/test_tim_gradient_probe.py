"""The gradient probe of tests/helpers/tim_probe.py on the fp32 torch restatements of TIM_GD and ALPHA_TIM (no GPU): it reads
back the gradient autograd computes, and it sees a 1 % change of each of the three loss terms.

Per case: g64 = float64 autograd gradient at the class means; e(x) = max |x - g64| / max(|g64|, 1e-3 max|g64| of the task).
  - the probe measures at least 99 % of the elements;
  - e(probe on the fp32 restatement) <= 4 e(fp32 autograd gradient): the probe adds no error of its own (fp32 rounding of
    w0 - w1 at |w0 - w1| in [0.2, 0.8] is about 1e-7 relative), what is left is the fp32 cancellation of the gradient;
  - loss_weights[i] * 1.01 in the probed run alone, for i = 0, 1, 2 in turn: e >= 10 x the clean e, and >= MUTATION_FLOOR.
    This is a condition on the inputs (weights, alpha, temperature: tim_probe.ENTROPIES), and what gives the bound of
    tests/test_gpu_tim_gradient.py its meaning: c e(ref32) there stays below MUTATION_FLOOR / 10.

Figures of this file (share left out / e(fp32 autograd) / e(probe) / e with loss weight 0, 1, 2 times 1.01):
  TIM_GD    prob D=10 K=10 shots 2 Q=75   0.0000 / 2.2e-05 / 1.5e-05 / 1.7e-01  1.4e-01  1.1e-01
  TIM_GD    rows D=16 K=10 shots 4 Q=1    0.0000 / 2.3e-04 / 1.9e-04 / 1.8e+00  2.5e+00  4.3e+00
  SSS       prob D=10 K=10 shots 2 Q=75   0.0000 / 2.2e-05 / 1.4e-05 / 1.7e-01  1.4e-01  1.1e-01
  SAA2      rows D=33 K=7 shots 2 Q=20    0.0000 / 9.4e-05 / 1.0e-04 / 3.7e-01  9.3e-01  1.3e+00
  AAA7      rows D=33 K=7 shots 1 Q=20    0.0000 / 5.6e-05 / 5.4e-05 / 2.8e-01  2.9e-01  1.8e-01
  ASS05     prob D=10 K=10 shots 1 Q=75   0.0000 / 4.5e-05 / 2.6e-05 / 2.4e-01  2.2e-01  2.1e-01
The smallest mutated figure is 1.1e-01, 570 x the largest clean one (MUTATION_FLOOR = 8e-2: these figures are one-per-cent
effects, not rounding, and move little between machines).  With AAA7 at the loss weights
(1, 0.7, 1.2) and temp 15 of the other settings, the marginal weight times 1.01 left e where it was (the term is negligible at
alpha = 7) and the restatement's fp32 cross-entropy was NaN: hence its own weights (1, 100, 3) and temp 5.
"""
import pytest
import torch

from helpers import tim_probe

# (entropy setting or None for TIM_GD, probability features, D, K, shots, Q); two tasks each
CASES = [(None, True, 10, 10, 2, 75), (None, False, 16, 10, 4, 1), ("SSS", True, 10, 10, 2, 75), ("SAA2", False, 33, 7, 2, 20),
         ("AAA7", False, 33, 7, 1, 20), ("ASS05", True, 10, 10, 1, 75)]


def test_cases_cover_both_methods_every_entropy_setting_and_one_query_row():
    assert {c[0] for c in CASES} == {None} | set(tim_probe.ENTROPIES)
    assert {c[1] for c in CASES} == {True, False} and any(c[5] == 1 for c in CASES)
    got = {tuple(e["entropies"]) for e in tim_probe.ENTROPIES.values()}
    assert got == {("Shannon",) * 3, ("Shannon", "Alpha", "Alpha"), ("Alpha",) * 3, ("Alpha", "Shannon", "Shannon")}
    assert tim_probe.ENTROPIES["AAA7"]["alpha_value"] == 7.0 and tim_probe.ENTROPIES["ASS05"]["alpha_value"] == 0.5


@pytest.mark.parametrize("ent,prob,D,K,shots,Q", CASES)
def test_probe_reads_the_autograd_gradient_and_sees_one_per_cent(ent, prob, D, K, shots, Q):
    x_q, x_s, y_s = tim_probe.make_inputs(prob, D, K, shots, Q, 2)
    prm, grad, run = tim_probe.restatement(ent, x_q, x_s, y_s, K)
    lw = prm["loss_weights"]
    w0, g64, _ = grad(torch.float64, lw)
    e_auto = tim_probe.error(grad(torch.float32, lw)[1], g64)
    g, measured = tim_probe.probe(run, lw, w0, g64)
    left_out, e_clean = tim_probe.share_left_out(measured), tim_probe.error(g, g64, measured)
    mutated = []
    for i in range(3):
        g_mut, m = tim_probe.probe(run, [w * (1.01 if j == i else 1.0) for j, w in enumerate(lw)], w0, g64)
        assert tim_probe.share_left_out(m) <= 0.01
        mutated.append(tim_probe.error(g_mut, g64, m))
    print(f"{ent or 'TIM_GD':9s} {'prob' if prob else 'rows'} D={D} K={K} shots {shots} Q={Q}   {left_out:.4f} / {e_auto:.1e} / "
          f"{e_clean:.1e} / " + "  ".join(f"{e:.1e}" for e in mutated))
    assert bool(torch.isfinite(g64).all()) and e_auto > 0
    assert left_out <= 0.01
    assert e_clean <= 4 * e_auto
    for i, e in enumerate(mutated):
        assert e >= 10 * e_clean and e >= tim_probe.MUTATION_FLOOR, (i, e, e_clean)
