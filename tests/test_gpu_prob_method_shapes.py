"""GPU: SOFT_KMEANS, HARD_KMEANS, KL_KMEANS, EM_GAUSSIAN, EM_GAUSSIAN_COV, PADDLE and BD-CSPN on probability features over a sweep
of class counts K, query counts Q and task counts T, against the torch restatements of oracle/ref_torch.py.

The launchers pick a kernel from K, Q and T, and the fixtures (K <= 397, Q = 75, T <= 6) reach one corner of that tree.  Here:
K = 511 .. 1024 (past the LDS-tile kernels: the E = 16 .. 32 register builds of k_kmeans_logits_rows, k_cov_logits_rows and
k_kl_divergences), Q off the special-cased 75 (k_mstats_rows / k_mstats in every mode and in their covariance form,
k_kl_centroids), an augmented BD-CSPN set of exactly 75 rows (the 75-row kernels in PlainQuotient mode), and T = 8, 9, 17 (the
part-filled last group of eight tasks).  Shapes and parameters: tests/helpers/prob_shapes.py.

Two tiers, both computed here from the restatements; no output of the engine is stored anywhere.
  bits   every output has the bits of the fp32 restatement run with the host-independent logarithm and, for KL_KMEANS's
         centroids, batched matrix product (tests/helpers/restated.py, pinned to the reference's fixtures by
         tests/test_restated_log_fixtures.py); criterions to 5e-6 relative.  Torch's CPU sum orders are those of its AVX-512
         kernels with at most 8 threads: on another host this tier skips.
  fp64   after one iteration every continuous output is within twice the fp32 restatement's own distance from the float64
         restatement, e(gpu) <= 2 e(ref32) with e(a) = max |a - ref64| / max(|ref64|, tiny).  Never skips.

Largest e(gpu) / e(ref32) seen on an MI355X whose host's MKL is not the fixture host's (there the logarithm and KL_KMEANS's sgemm
differ from the restated ones in the last place, so the ratio is not 1 where they enter; about 95 % of the figures were exactly 1):
SOFT_KMEANS 1.000, HARD_KMEANS 1.000, BD-CSPN 1.000, KL_KMEANS 1.105 (w, K = 7, Q = 128), EM_GAUSSIAN 1.572 (v, K = 100, Q = 74),
EM_GAUSSIAN_COV 1.736 (v, K = 40, Q = 74), PADDLE 1.810 (v, K = 7, Q = 76).  On that host torch's own bmm gave KL_KMEANS
centroids other than the engine's in 1 to 3 elements at K = 7, Q = 74, 76 and 128 - MKL's order there, not the reference's:
hence the restated product in the bit tier.

The K >= 512 cases take 3 to 20 s each on the host: the restatements of PADDLE and BD-CSPN build (S, K, K) temporaries of 4 to
8 GB from a support set of S = K rows."""
import pytest
import torch

from helpers import prob_shapes as ps
from helpers.restated import restated_bmm, restated_log

pytestmark = pytest.mark.gpu

AVX512 = torch.backends.cpu.get_cpu_capability() == "AVX512"
bits_tier = pytest.mark.skipif(not AVX512, reason="torch's sum orders are pinned for the AVX-512 ATen kernels")


@pytest.fixture(scope="module", autouse=True)
def eight_threads():
    """torch's CPU reductions keep their order up to 8 threads (scripts/host_threads_check.py)"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def log():
    """the host-independent stand-ins for torch.log and for KL_KMEANS's bmm, as keyword arguments of the restatements"""
    return {"log": restated_log(), "bmm": restated_bmm()}


_bdcspn32 = {}


def reference(method, shape, inp, log, iters=None):
    """the fp32 restatement; BD-CSPN is one pass whatever `iters` says and has no logarithm in it, so both tiers share its run
    (at K = 1024 its (S + Q, K, K) temporaries make it the slowest of the seven)"""
    if method != "bdcspn":
        return ps.run_reference(method, shape, inp, iters=iters, **log)
    if shape not in _bdcspn32:
        _bdcspn32[shape] = ps.run_reference(method, shape, inp)
    return _bdcspn32[shape]


def check_bits(method, shape, inp, log):
    """prints the number of differing elements per tensor (and the criterions' gap) before asserting that there is none"""
    want = reference(method, shape, inp, log)
    got = ps.run_engine(method, shape, inp)
    bad = ps.bit_differences(got, want)
    gap = ps.criterion_gap(got, want) if "criterions" in want else 0.0
    print(f"{ps.shape_id(shape)} {method}: differing elements {bad}" + (f", criterions off by {gap:.2e} relative" if "criterions" in want else ""))
    return [f"{method}.{k}: {n} elements" for k, n in bad.items() if n] + ([f"{method}.criterions: {gap:.2e}"] if not gap <= ps.CRIT_RTOL else [])


def check_fp64(method, shape, inp):
    """prints e(gpu) and e(ref32) per tensor before asserting e(gpu) <= 2 e(ref32)"""
    ref64 = ps.run_reference(method, shape, inp, iters=1, dtype=torch.float64)
    ref32 = reference(method, shape, inp, {}, iters=1)
    got = ps.run_engine(method, shape, inp, iters=1)
    failed = []
    for k in ps.CONTINUOUS[method]:
        e_gpu, e_ref = ps.rel_err(got[k], ref64[k]), ps.rel_err(ref32[k], ref64[k])
        print(f"{ps.shape_id(shape)} {method}.{k}: e(gpu) {e_gpu:.3e}  e(ref32) {e_ref:.3e}  ratio {e_gpu / e_ref if e_ref else float(e_gpu > 0):.3f}")
        if not e_gpu <= 2 * e_ref:
            failed.append(f"{method}.{k}: e(gpu) {e_gpu:.3e} > 2 x e(ref32) {e_ref:.3e}")
    return failed


@bits_tier
@pytest.mark.parametrize("shape", ps.ALL_SEVEN, ids=ps.shape_id)
def test_bits_match_torch(shape, log):
    inp = ps.make_inputs(shape)
    failed = [f for m in ps.METHODS for f in check_bits(m, shape, inp, log)]
    assert not failed, (ps.shape_id(shape), failed)


@pytest.mark.parametrize("shape", ps.ALL_SEVEN, ids=ps.shape_id)
def test_one_iteration_within_fp64_bound(shape):
    inp = ps.make_inputs(shape)
    failed = [f for m in ps.METHODS for f in check_fp64(m, shape, inp)]
    assert not failed, (ps.shape_id(shape), failed)


@bits_tier
@pytest.mark.parametrize("shape", ps.AUG75, ids=ps.shape_id)
def test_bits_match_torch_augmented_set_of_75_rows(shape, log):
    assert shape[0] * shape[3] + shape[1] == 75
    inp = ps.make_inputs(shape)
    failed = [f for m in ps.FEW_SHOT for f in check_bits(m, shape, inp, log)]
    assert not failed, (ps.shape_id(shape), failed)


@pytest.mark.parametrize("shape", ps.AUG75, ids=ps.shape_id)
def test_one_iteration_within_fp64_bound_augmented_set_of_75_rows(shape):
    inp = ps.make_inputs(shape)
    failed = [f for m in ps.FEW_SHOT for f in check_fp64(m, shape, inp)]
    assert not failed, (ps.shape_id(shape), failed)


@bits_tier
@pytest.mark.parametrize("method", ["hkm", "klk"])
def test_criterions_are_per_batch(method, log):
    """T = 8 as two batches of four tasks: the tasks' results are those of one batch of eight, and row b of the criterions is the
    mean over batch b's tasks alone - what the restatement logs for those four tasks on their own"""
    shape = (72, 75, 8, 1)
    inp = ps.make_inputs(shape)
    got = ps.run_engine(method, shape, inp, n_batches=2)
    want = ps.run_reference(method, shape, inp, **log)
    bad = ps.bit_differences(got, want)
    print(f"{method}, two batches: differing elements {bad}")
    assert not any(bad.values()), bad
    assert got["criterions"].shape == (2, ps.ITERS[method])
    halves = [ps.run_reference(method, (72, 75, 4, 1), {"x_q": inp["x_q"][4 * b:4 * b + 4]}, **log)["criterions"] for b in range(2)]
    per_batch = torch.cat(halves)
    assert not torch.equal(per_batch[0], per_batch[1]), "the two batches must not log the same criterions for this to tell anything"
    gap = ps.criterion_gap(got, {"criterions": per_batch})
    print(f"{method}, two batches: criterions {got['criterions'].tolist()} against {per_batch.tolist()}, off by {gap:.2e} relative")
    assert gap <= ps.CRIT_RTOL
