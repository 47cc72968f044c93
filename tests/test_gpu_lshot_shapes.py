"""GPU: LAPLACIAN_SHOT's four kernels (k_lshot_normalize, k_lshot_unary, k_lshot_pairdist, k_lshot_task) over the sweep of
Q, K, T and knn of tests/helpers/lshot_shapes.py, every update checked.  Each case is one engine call plus the host restatement;
the conditions that make the discrete comparisons meaningful are asserted on the CPU by tests/test_lshot_shapes.py, so nothing
here skips.

  A  the distance kernels against oracle/ref_torch.py: neighbour lists equal, the unary term within rtol 5e-6,
     atol 1e-6 max|row|^2 (derived in tests/test_gpu_visual_lshot.py::test_shape_sweep_matches_restatement), and a float64 tier:
     e(gpu) <= 2 e(ref32), e(a) = max |a - ref64| / max|row|^2, ref64 = normalisation, class means and squared distances in
     float64 numpy (the rule of tests/test_gpu_prob_method_shapes.py)
  B  k_lshot_task's loop in isolation: the engine's OWN unary term and neighbour lists go through the float64 restatement
     (lshot_shapes.restated_loop).  preds_iter equal at every (task, update, query) whose restated logit gap is >= tau = 4 s_L
     (at most 2 % left out), frozen_at equal (read off both energy arrays by one function), energies within 4 s_E + floor of the
     restated ones, floor = Q K 2^-53 sum|terms| / |E|.  s_E, s_L: what a last-place change of the fp32 start Y0 does to the
     energies and logits of the restatement; the factor 4 because the engine's start (expf within 1 ulp, its fp32 sum over K in
     lane order, the division) can sit a few places from numpy's where s_E samples one.  Also at iters = 1, 2, 3.
  C  end to end against ref_torch for lmd (knn - 1) <= 2.8: energies to 1e-6 relative, the final assignment equal where the
     restated gap of the last update is >= tau.  The amplifying cases (knn = 13, 20, 40: s_E up to 2.5e-6, past the 1e-6 of this
     comparison for a correct engine) are judged by B alone.
  D  at D = K the visual entry has the probability entry's bits; the entries fed from the feature tables have the dense ones'
  E  refusals before any launch: Q = 1025, knn = Q + 1, a neighbour list past the 60 000-byte LDS check

Seen on an MI355X: neighbour lists, frozen_at and every compared assignment equal, no element left out
(share 0.00 % on every case); unary e(gpu) / e(ref32) at most 1.000; energies e(gpu) / s_E at most 1.46 where s_E >= 1e-10
(K = 2, Q = 75) and 3.6 where s_E = 1.6e-14 (K = 130: the floor's range), e(gpu) / (4 s_E + floor) at most 0.37; largest s_E
2.5e-6 (knn = Q = 20, L2N); end to end the energies are within 5.8e-8 of ref_torch's except at Q = 2 and Q = 3 (1.6e-7 .. 3.5e-7).
With two or three queries the fp32 roundings of the unary term do not average out: with the seeds first tried there, ref_torch's
own energies were 1e-6 .. 5e-6 from those of the float64 unary term and the engine's 1.1e-6 .. 1.3e-6 from ref_torch's, the loop
being within 0.22 of B's bound; hence the CPU condition lshot_shapes.reference_energy_error <= 0.25e-6 for the cases of C."""
import numpy as np
import pytest
import torch

from helpers import lshot_shapes as ls

pytestmark = pytest.mark.gpu

_out, _judged = {}, {}


def engine_out(c):
    """(unary, neighbours, preds_iter, energies) of one engine call per case, shared by A, B and C and never written to"""
    if c not in _out:
        _out[c] = ls.run_engine(c)
        for a in _out[c]:
            a.setflags(write=False)
    return _out[c]


def judged(c):
    """per task, the restated loop fed the engine's own unary term and neighbour lists, with its sensitivities"""
    if c not in _judged:
        unary, nbr, _, _ = engine_out(c)
        _judged[c] = [ls.judge_task(unary[k], nbr[k], ls.LMD, c.iters) for k in range(c.T)]
    return _judged[c]


def check_ranges(c, out):
    unary, nbr, preds_iter, e = out
    assert unary.shape == (c.T, c.Q, c.K) and nbr.shape == (c.T, c.Q, c.knn - 1)
    assert preds_iter.shape == (c.T, c.iters, c.Q) and e.shape == (c.T, c.iters)
    assert nbr.min() >= 0 and nbr.max() < c.Q, "a neighbour outside the task"
    assert not (nbr == np.arange(c.Q)[None, :, None]).any(), "a query is its own neighbour"
    assert preds_iter.min() >= 0 and preds_iter.max() < c.K, "an assignment outside 0..K-1"
    assert np.isfinite(unary).all() and np.isfinite(e).all()


# ---- A. the distance kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", ls.ALL, ids=ls.case_id)
def test_distance_kernels_match_the_restatement(c):
    out = engine_out(c)
    check_ranges(c, out)
    unary, nbr = out[0], out[1]
    t = ls.run_reference(c)
    scale2 = ls.scale2(c)
    ref64 = ls.unary64(c)
    e_gpu = float(np.abs(unary - ref64).max()) / scale2
    e_ref = float(np.abs(t["unary"] - ref64).max()) / scale2
    print(f"{ls.case_id(c)}: unary e(gpu) {e_gpu:.3e}  e(ref32) {e_ref:.3e}  ratio {e_gpu / e_ref if e_ref else float(e_gpu > 0):.3f}  "
          f"(against ref32: {float(np.abs(unary - t['unary']).max()):.3e} absolute, max|row|^2 {scale2:.3f})")
    assert np.array_equal(np.sort(nbr, axis=2), t["neighbours"]), "kNN graph differs"
    assert np.allclose(unary, t["unary"], rtol=5e-6, atol=1e-6 * scale2)
    assert e_gpu <= 2 * e_ref, f"unary: e(gpu) {e_gpu:.3e} > 2 x e(ref32) {e_ref:.3e}"


# ---- B. the loop in isolation -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", ls.ALL, ids=ls.case_id)
def test_loop_matches_the_restatement_on_its_own_inputs(c):
    out = engine_out(c)
    check_ranges(c, out)
    _, _, preds_iter, e = out
    failed, left, total = [], 0, 0
    for k, j in enumerate(judged(c)):
        keep = ~j.left_out
        left, total = left + int(j.left_out.sum()), total + j.left_out.size
        wrong = int((preds_iter[k] != j.loop["preds_iter"])[keep].sum())
        f_gpu, f_ref = ls.frozen_from_energies(e[k]), ls.frozen_from_energies(j.loop["energies"])
        dev = np.abs(e[k] / j.loop["energies"] - 1)
        bound = ls.BOUND_FACTOR * j.s_e + j.floor
        e_gpu = float(dev.max())
        print(f"{ls.case_id(c)} task {k}: frozen at {f_gpu} (restated {f_ref}), energies e(gpu) {e_gpu:.3e}, s_E {j.s_e:.3e}, "
              f"e(gpu)/s_E {e_gpu / j.s_e if j.s_e else float('inf') if e_gpu else 0.0:.3f}, e(gpu)/(4 s_E + floor) {float((dev / bound).max()):.3f}, "
              f"tau {j.tau:.2e}, differing assignments {wrong} of {int(keep.sum())}")
        if wrong:
            failed.append(f"task {k}: {wrong} assignments differ where the gap is >= tau")
        if f_gpu != f_ref:
            failed.append(f"task {k}: frozen at {f_gpu}, restated {f_ref}")
        if not (dev <= bound).all():
            failed.append(f"task {k}: energies off by {e_gpu:.3e}, bound {float(bound.max()):.3e}")
    print(f"{ls.case_id(c)}: left out {left} of {total} ({100.0 * left / total:.2f} %)")
    assert left <= ls.MAX_LEFT_OUT * total
    assert not failed, (ls.case_id(c), failed)


# ---- C. end to end ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in ls.ALL if not ls.amplifying(c)], ids=ls.case_id)
def test_end_to_end_matches_ref_torch(c):
    _, _, preds_iter, e = engine_out(c)
    t = ls.run_reference(c)
    de = float(np.abs(e / t["ent_energy"] - 1).max())
    keep = np.stack([~j.left_out[-1] for j in judged(c)])
    wrong = int((preds_iter[:, -1] != t["preds"])[keep].sum())
    print(f"{ls.case_id(c)}: energies {de:.3e} relative, final assignments differing {wrong} of {int(keep.sum())} ({keep.size} in all)")
    assert np.allclose(e, t["ent_energy"], rtol=1e-6, atol=0)
    assert wrong == 0


# ---- D. the entries agree bit for bit -----------------------------------------------------------------------------------------

NAMES = ("unary", "neighbours", "preds_iter", "energies")


@pytest.mark.parametrize("c", [c for c in ls.SWEEP if c.entry == "prob" and (c.K, c.Q) in ((63, 40), (129, 128), (1000, 75))], ids=ls.case_id)
def test_width_equal_to_class_count_equals_the_probability_entry(c):
    """k_lshot_pairdist sums in the order of k_lshot_task's own loop: at one, three and sixteen class strides too"""
    from tclip_amd import engine
    x_q, x_s, y_s = (a.cuda() for a in ls.make_inputs(c))
    vis = engine.run_laplacian_shot_visual(x_q, x_s, y_s, n_class=c.K, **ls.params(c))
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, vis, engine_out(c)):
        assert np.array_equal(a.cpu().numpy(), b), name


@pytest.mark.parametrize("D,K,S,Q,knn", [(64, 5, 5, 2, 2), (40, 7, 14, 33, 4), (33, 10, 10, 129, 5)])
@pytest.mark.parametrize("softmax", [False, True], ids=["visual", "prob"])
def test_in_place_entries_equal_the_dense_ones(D, K, S, Q, knn, softmax):
    """tables and indices as tests/test_gpu_support_in_place.py builds them (T = 3), at query counts off 75"""
    from tclip_amd import engine
    from test_gpu_support_in_place import _inputs, same
    if softmax:
        D = K
    table_q, q_idx, table_s, s_idx, y_s, cols, x_q, x_s = _inputs(D, K, S, Q, softmax, D * 1009 + K * 13 + Q)
    for norm_type in ls.NORMS:
        prm = dict(iters=6, knn=knn, lmd=ls.LMD, norm_type=norm_type)
        if softmax:
            dense = engine.run_laplacian_shot(x_q, x_s, y_s.cuda(), **prm)
            tasks = engine.run_laplacian_shot_tasks(table_q, q_idx, table_s, s_idx.cuda(), y_s, cols, **prm)
        else:
            dense = engine.run_laplacian_shot_visual(x_q, x_s, y_s.cuda(), n_class=K, **prm)
            tasks = engine.run_laplacian_shot_visual_tasks(table_q, q_idx.cuda(), table_s, s_idx, y_s, n_class=K, **prm)
        torch.cuda.synchronize()
        assert tasks[0].shape == (3, Q, K) and tasks[2].shape == (3, 6, Q)
        for name, a, b in zip(NAMES, tasks, dense):
            assert same(a, b), (name, norm_type)


# ---- E. refusals ----------------------------------------------------------------------------------------------------------------

def _rows(Q, visual):
    D, K = (16, 4) if visual else (4, 4)
    gen = torch.Generator().manual_seed(Q)
    x_q, x_s = torch.rand(1, Q, D, generator=gen) + 0.1, torch.rand(1, 2 * K, D, generator=gen) + 0.1
    return x_q.cuda(), x_s.cuda(), torch.arange(K).repeat(2)[None].cuda()


@pytest.mark.parametrize("visual", [True, False], ids=["visual", "prob"])
def test_refusals(visual):
    from tclip_amd import engine

    def run(Q, knn):
        x_q, x_s, y_s = _rows(Q, visual)
        if visual:
            return engine.run_laplacian_shot_visual(x_q, x_s, y_s, n_class=4, iters=3, knn=knn, lmd=ls.LMD)
        return engine.run_laplacian_shot(x_q, x_s, y_s, iters=3, knn=knn, lmd=ls.LMD)

    with pytest.raises(RuntimeError, match="n_query"):
        run(1025, 3)
    with pytest.raises(RuntimeError, match="knn"):
        run(40, 41)
    with pytest.raises(RuntimeError, match="too large"):
        run(1024, 16)                                    # 1024 * 15 * 4 + 8192 = 69 632 > 60 000
    unary, nbr, preds_iter, e = run(40, 40)              # and knn = Q is fine (knn = 13 at Q = 1024 runs in the sweep)
    torch.cuda.synchronize()
    assert nbr.shape == (1, 40, 39) and bool(torch.isfinite(e).all())
    assert bool((nbr.sort(2).values == torch.tensor([[j for j in range(40) if j != i] for i in range(40)], device=nbr.device)[None]).all())
