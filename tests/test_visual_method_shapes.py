"""CPU: the visual-feature shape sweep of tests/helpers/visual_shapes.py before it reaches a GPU.  The restatements
(helpers/visual.reference_step, helpers/visual_cov, helpers/visual_fs.paddle_step / bdcspn_pass) and the chosen inputs alone meet
the conditions under which tests/test_gpu_visual_method_shapes.py compares bits - asserted here for every listed shape, so that
the GPU test cannot pass on tensors of zeros and ones:
  every output is finite; for SOFT_KMEANS, EM_GAUSSIAN and PADDLE at least 0.5 % of u after the first iteration lies strictly
  between 1e-6 and 1 - 1e-6; HARD_KMEANS at K >= 24 has at least one dead and two live clusters per call after the first
  iteration; the planted classes stay dead through every iteration, with a live cluster beside them.
The restatements take the logarithm as a parameter (restated_log() gives v and what follows it the same bits on every host) and
run in float64 on float64 inputs: the two things the GPU tiers need of them.
Seen with the table's seeds: the lowest interior share is 0.80 % (SOFT_KMEANS and EM_GAUSSIAN at D = 33, K = 130, Q = 76, T = 9;
PADDLE's is above 99.9 % everywhere), HARD_KMEANS keeps at least 2 live (Q = 1, T = 2) and at least 1 dead cluster (D = 7,
Q = 288) per call - at D = 40, K = 24, Q >= 74 only from the u0 with two zeroed columns that helpers/visual_shapes.py gives it
there -, and every planted cluster's size is exactly 0 after each of four iterations."""
import pytest
import torch

from helpers import visual, visual_fs
from helpers import visual_shapes as vs
from helpers.restated import restated_log


@pytest.fixture(scope="module")
def log():
    return restated_log()


def _methods(shape):
    return ("cov",) if shape in vs.COV_CHUNKS else vs.ZERO_SHOT


@pytest.mark.parametrize("shape", vs.ZS_ALL + vs.COV_CHUNKS, ids=vs.shape_id)
def test_zero_shot_case_meets_its_conditions(shape, log):
    inp = vs.make_inputs(shape)
    assert inp["x_q"].shape == (shape[3], shape[2], shape[0]) and inp["u0"].shape == (shape[3], shape[2], shape[1])
    missed = []
    for m in _methods(shape):
        trail = []
        out = vs.run_reference(m, shape, inp, log=log, trail=trail)
        assert len(trail) == vs.ITERS[m]
        missed += vs.unmet_conditions(m, shape, out, trail)
    assert not missed, missed


@pytest.mark.parametrize("case", vs.FS_CASES, ids=vs.case_id)
def test_few_shot_case_meets_its_conditions(case, log):
    method, shape = case
    inp = vs.make_inputs(shape)
    D, K, shots, Q, T = shape
    counts = visual_fs.one_hot(inp["y_s"], K).sum(1)
    if shots:
        assert bool((counts == shots).all())
    else:
        assert torch.equal(counts, torch.tensor([1.0 + k % 3 for k in range(K)]).repeat(T, 1))
        assert not torch.equal(inp["y_s"][0], inp["y_s"][0].sort().values) and not torch.equal(inp["y_s"][0], inp["y_s"][1])
    assert inp["x_q"].shape == (T, Q, D) and inp["x_s"].shape == (T, int(counts[0].sum()), D)
    trail = []
    out = vs.run_reference(method, shape, inp, log=log, trail=trail, norm_type=vs.norm_type_of(case) if method == "bdcspn" else "L2N")
    missed = vs.unmet_conditions(method, shape, out, trail)
    assert not missed, missed


@pytest.mark.parametrize("shape", vs.PLANTED, ids=vs.shape_id)
def test_planted_clusters_stay_dead(shape, log):
    """four iterations, one more than the GPU test runs"""
    inp = vs.make_planted(shape)
    assert bool((inp["u0"][:, :, vs.PLANTED_DEAD] == 0).all()) and torch.allclose(inp["u0"].sum(-1), torch.ones(shape[3], shape[2]), atol=1e-6)
    missed = []
    for m in vs.PLANTED_METHODS:
        trail = []
        out = vs.run_reference(m, shape, inp, iters=4, log=log, trail=trail)
        missed += vs.unmet_conditions(m, shape, out, trail, planted=True)
        w0 = vs.run_reference(m, shape, inp, iters=0, log=log) if m == "cov" else None
        if w0 is not None:          # the restatement itself keeps the rows its init wrote
            for k in ("w", "s"):
                assert torch.equal(out[k][:, vs.PLANTED_DEAD].view(torch.int32), w0[k][:, vs.PLANTED_DEAD].view(torch.int32)), (m, k)
    assert not missed, missed


def test_the_table_is_the_issue_s():
    """the block, level, chunk, tile and task-group edges the sweep is there for"""
    assert len(vs.ZS_ROWS) == 30 and {s[0] for s in vs.ZS_ROWS} == {40, 7} and all(s[1] == 24 and s[3] == 2 for s in vs.ZS_ROWS)
    assert {s[2] for s in vs.ZS_ROWS} == {1, 3, 15, 16, 17, 31, 32, 33, 74, 76, 255, 256, 257, 272, 288}
    assert vs.ZS_LEVEL3 == [(8, 16, 4096, 1), (8, 16, 4097, 1), (8, 16, 4112, 1)]
    assert vs.ZS_CHUNKS == [(520, 72, 16, 2), (520, 72, 17, 2), (1024, 24, 17, 2)] and vs.COV_CHUNKS == [(300, 24, 17, 2)]
    assert vs.ZS_TASKS == [(33, 72, 75, 1), (33, 72, 75, 8), (33, 72, 75, 9), (33, 72, 75, 17), (33, 130, 76, 9)]
    assert [s for s in vs.PADDLE_SHAPES if s[:3] == (40, 24, 2)] == [(40, 24, 2, q, 2) for q in (1, 15, 16, 17, 76, 255, 256, 257, 272, 288)]
    assert set(vs.PADDLE_SHAPES) >= {(520, 24, 1, 17, 2), (8, 16, 1, 4097, 1), (33, 72, 1, 75, 1), (33, 72, 1, 75, 9), (33, 72, 1, 75, 17)}
    assert len(vs.PADDLE_SHAPES) == 15
    assert vs.BDCSPN_SHAPES == [(40, 5, 2, 1, 2), (40, 5, 2, 17, 2), (40, 5, 2, 246, 2), (40, 5, 2, 247, 2), (40, 5, 2, 278, 2),
                                (40, 24, 1, 264, 2), (33, 72, 1, 75, 9)]
    assert {s[1] * s[2] + s[3] for s in vs.BDCSPN_SHAPES} >= {256, 257, 288}                   # augmented rows
    assert vs.UNBALANCED == [(40, 24, 0, 17, 2), (513, 24, 0, 17, 2)]
    assert vs.PLANTED == [(40, 130, 75, 2), (40, 130, 17, 2), (520, 130, 16, 2)]
    assert set(range(16, 32)) <= set(vs.PLANTED_DEAD) and set(range(64, 128)) <= set(vs.PLANTED_DEAD) and len(vs.PLANTED_DEAD) == 80
    assert {vs.norm_type_of(c) for c in vs.FS_CASES if c[0] == "bdcspn"} == set(vs.NORM_TYPES)
    assert set(vs.HKM_ZEROED_AT) < set(vs.ZS_ROWS) and all(s[0] == 40 and s[2] >= 74 for s in vs.HKM_ZEROED_AT)
    assert min(vs.HKM_ZEROED_COLUMNS) < 16 <= max(vs.HKM_ZEROED_COLUMNS) < 24
    every = vs.ZS_ALL + vs.COV_CHUNKS + vs.PLANTED
    assert max(s[0] * s[1] * s[2] * s[3] for s in every) * 4 < 200e6
    assert max(d * k * q * t for d, k, _, q, t in vs.PADDLE_SHAPES + vs.BDCSPN_SHAPES + vs.UNBALANCED) * 4 < 200e6
    assert len({vs.shape_id(s) for s in every}) == len(every) and len({vs.case_id(c) for c in vs.FS_CASES}) == len(vs.FS_CASES)


def test_the_logarithm_is_a_parameter_with_the_default_unchanged(log):
    """reference_step and paddle_step: torch.log by default, and `log` reaches v (and only v, within one iteration)"""
    shape = (40, 24, 17, 2)
    inp = vs.make_inputs(shape)
    calls = []

    def spy(x):
        calls.append(x.shape)
        return torch.log(x)
    a = visual.reference_step("em_gaussian", inp["x_q"], inp["u0"].clone(), lambd=vs.lambd_of(shape))
    b = visual.reference_step("em_gaussian", inp["x_q"], inp["u0"].clone(), lambd=vs.lambd_of(shape), log=spy)
    assert calls == [(2, 24)] and all(torch.equal(x, y) for x, y in zip(a, b))
    c = visual.reference_step("em_gaussian", inp["x_q"], inp["u0"].clone(), lambd=vs.lambd_of(shape), log=log)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.allclose(a[2], c[2], rtol=1e-6, atol=5e-7)
    fs = vs.make_inputs((40, 24, 2, 17, 2))
    del calls[:]
    a = visual_fs.paddle_step(fs["x_s"], fs["x_q"], fs["y_s"], 24, 7.5)
    b = visual_fs.paddle_step(fs["x_s"], fs["x_q"], fs["y_s"], 24, 7.5, log=spy)
    assert calls == [(2, 24)] and all(torch.equal(x, y) for x, y in zip(a, b))
    c = visual_fs.paddle_step(fs["x_s"], fs["x_q"], fs["y_s"], 24, 7.5, log=log)
    assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2]) and torch.allclose(a[1], c[1], rtol=1e-6, atol=5e-7)


@pytest.mark.parametrize("method", vs.ZERO_SHOT + vs.FEW_SHOT)
def test_restatements_run_in_float64(method):
    """float64 in, float64 out, and within float32's reach of the float32 run after one iteration"""
    shape = (40, 24, 17, 2) if method in vs.ZERO_SHOT else (40, 24, 2, 17, 2)
    inp = vs.make_inputs(shape)
    r64 = vs.run_reference(method, shape, inp, iters=1, dtype=torch.float64)
    r32 = vs.run_reference(method, shape, inp, iters=1)
    for k in vs.CONTINUOUS[method]:
        assert r64[k].dtype == torch.float64 and r32[k].dtype == torch.float32, k
        assert (r32[k].double() - r64[k]).abs().max() <= 1e-4 * r64[k].abs().max(), k
        assert not torch.equal(r32[k].double(), r64[k]), k
    assert torch.equal(r64["preds"], r32["preds"])
