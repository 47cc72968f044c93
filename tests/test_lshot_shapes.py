"""CPU: the LAPLACIAN_SHOT shape sweep of tests/helpers/lshot_shapes.py before it reaches a GPU.  The float64 restatement of
the bound-update loop is faithful to oracle/ref_torch.py (and so to the reference's fixtures), and every sweep case meets the
conditions under which tests/test_gpu_lshot_shapes.py compares discrete results - asserted here, with the seeds constants of
the shape table, so that the GPU test never skips:
  kNN margin >= 1e-6; the neighbour lists survive a last-place change of the normalised rows; the break is determined; at most
  2 % of the (task, update, query) elements have a logit gap below tau = 4 s_L; where the energies are compared with ref_torch's
  end to end to 1e-6 (lmd (knn - 1) <= 2.8), ref_torch's own are within a quarter of that of the energies of the correctly
  rounded float64 unary term - the reference's fp32 unary term must leave the bound to the engine.
The break: the comparison of update `it` reads E[it] and E[it-1], so | |E - E_old| / |E_old| - 1e-6 | must be at least 4 x the
larger of those two updates' energy bounds 4 s_E(it) + floor(it) (lshot_shapes.judge_task: freeze_slack >= 1).  With the bound
of the whole run in their place the condition cannot be met at knn = Q = 20 (tried: 400 seeds): there s_E is 1e-7 .. 2.5e-6 at
updates 2 to 4, where lmd (knn - 1) = 13.3 amplifies a last-place change of Y0, and below 1e-9 from update 5 on, where the
iteration has settled and every one of these tasks takes the break - a margin of at most 1e-6 against 16 s_E.
Seen with the table's seeds: kNN margins >= 2.6e-6, s_E 1e-16 .. 2e-8 for knn <= 5 and up to 2.5e-6 at knn = 20 (the reason the
energy bound is 4 s_E + floor and not a constant), freeze_slack >= 770, no gap below tau, reference_energy_error <= 2.45e-7, the restated energies within 4e-15
relative of ref_torch's; 26 tasks freeze at update 2, 81 later (up to 13), 3 never."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_names
from helpers import lshot_shapes as ls
from oracle import ref_torch

FIXTURES = golden_names("fs_lshot_")


def _faithful(t, lmd, iters, label):
    """restated_loop fed ref_torch's own unary term and neighbours returns ref_torch's decisions exactly and its energies to
    1e-9 relative (the tolerance of test_oracle_reproduces_reference between the oracle and the reference)"""
    worst = 0.0
    for k in range(len(t["unary"])):
        r = ls.restated_loop(t["unary"][k], t["neighbours"][k], lmd, iters)
        assert np.array_equal(r["preds_iter"], t["preds_iter"][k]), (label, k, "assignments")
        assert r["frozen_at"] == t["frozen_at"][k], (label, k, "frozen_at", r["frozen_at"], t["frozen_at"][k])
        assert ls.frozen_from_energies(t["ent_energy"][k]) == (-1 if r["frozen_at"] == iters - 1 else r["frozen_at"]), (label, k)
        gap = float(np.abs(r["energies"] / t["ent_energy"][k] - 1).max())
        worst = max(worst, gap)
        assert gap <= 1e-9, (label, k, gap)
    print(f"{label}: energies within {worst:.2e} relative of ref_torch's")


@pytest.mark.parametrize("c", ls.ALL, ids=ls.case_id)
def test_restated_loop_is_faithful_on_the_sweep(c):
    _faithful(ls.run_reference(c), ls.LMD, c.iters, ls.case_id(c))


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_loop_is_faithful_on_the_fixtures(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    t = ref_torch.run_laplacian_shot(torch.from_numpy(g["x_q"]), torch.from_numpy(g["x_s"]), torch.from_numpy(g["y_s"]),
                                     torch.from_numpy(g["y_q"]), n_class=int(g["K"]), iters=int(g["iters"]), knn=int(g["knn"]),
                                     lmd=float(g["lmd"]), norm_type=str(g["norm_type"]))
    assert np.allclose(t["ent_energy"], g["ent_energy"], rtol=1e-9, atol=0)
    _faithful(t, float(g["lmd"]), int(g["iters"]), name)


def test_the_fixtures_are_all_there():
    assert len(FIXTURES) == 7


@pytest.mark.parametrize("c", ls.ALL, ids=ls.case_id)
def test_case_meets_its_conditions(c):
    t = ls.run_reference(c)
    margin = ls.knn_margin(c)
    print(f"{ls.case_id(c)}: kNN margin {margin:.3e}")
    assert margin >= ls.KNN_MARGIN
    assert np.array_equal(ls.neighbours64(c), t["neighbours"]), "the neighbour lists change with the last place of the rows"
    assert t["neighbours"].min() >= 0 and t["neighbours"].max() < c.Q
    assert not (t["neighbours"] == np.arange(c.Q)[None, :, None]).any()
    if not ls.amplifying(c):
        # compared end to end: the reference's own fp32 unary term may use up a quarter of that bound, no more
        own = ls.reference_energy_error(c)
        print(f"  ref_torch's energies are {own:.2e} relative from those of the correctly rounded float64 unary term")
        assert own <= 0.25 * ls.END_TO_END_RTOL
    left = total = 0
    for k in range(c.T):
        j = ls.judge_task(t["unary"][k], t["neighbours"][k], ls.LMD, c.iters)
        print(f"  task {k}: frozen at {j.loop['frozen_at']}, s_E {j.s_e:.2e}, s_L {j.s_l:.2e}, floor {j.floor.max():.2e}, "
              f"energy bound {j.bound:.2e}, freeze margin {j.freeze_margin:.2e} ({j.freeze_slack:.1f} x 4 x the bounds of the updates it "
              f"compares), gaps below tau {int(j.left_out.sum())}")
        assert j.freeze_slack >= 1, (k, j.freeze_margin, j.freeze_slack)
        left, total = left + int(j.left_out.sum()), total + j.left_out.size
    print(f"  left out {left} of {total}")
    assert left <= ls.MAX_LEFT_OUT * total


def test_both_branches_of_the_freeze_are_reached():
    frozen = {(ls.case_id(c), k): int(f) for c in ls.SWEEP for k, f in enumerate(ls.run_reference(c)["frozen_at"])}
    print({f: sum(v == f for v in frozen.values()) for f in sorted(set(frozen.values()))})
    assert any(f == -1 for f in frozen.values()), "no task runs all 15 updates"
    assert any(f == 2 for f in frozen.values()), "no task freezes at update 2, the first the `it > 1` guard lets through"
    assert any(f > 4 for f in frozen.values()), "no task freezes late"
    assert frozen[("visual-D8-K3-s1-Q300-T1-knn40-L2N", 0)] == -1


def test_the_table_is_the_issue_s():
    """the register counts, tile edges and strides the sweep is there for"""
    vis = [c for c in ls.SWEEP if c.entry == "visual"]
    assert {-(-c.Q // 64) for c in vis} >= {1, 2, 3, 5, 16} and {c.Q for c in vis} >= {2, 3, 31, 32, 33, 63, 64, 65, 128, 129, 1024}
    assert {-(-c.K // 64) for c in vis} >= {1, 3, 5, 16} and any(c.K % 64 == 0 and c.K > 64 for c in vis)
    assert any(c.knn == c.Q and c.knn - 1 == 19 for c in vis) and any(c.knn - 1 == 39 for c in vis)
    assert any((c.T * c.Q) % 4 for c in vis) and any((c.T * c.K * c.shots) % 4 for c in vis)
    big = max(((c.Q * (c.knn - 1) * 4 + 7) & ~7) + c.Q * 8 for c in vis)
    assert big == 57344 and ((1024 * 15 * 4 + 7) & ~7) + 1024 * 8 == 69632 > 60000 >= big
    assert {c.K for c in ls.SWEEP if c.entry == "prob"} == {2, 63, 64, 65, 129, 512, 1000, 1024}
    assert [c.iters for c in ls.SHORT_ITERS] == [1, 2, 3]
    assert all(not ls.amplifying(c) for c in ls.SWEEP if c.knn <= 5) and all(ls.amplifying(c) for c in ls.SWEEP if c.knn >= 13)
