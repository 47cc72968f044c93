"""GPU: the accuracy tail's prototype kernels stage by stage - tclip_cluster_prototypes (k_one_hot, k_cluster_sizes, launch_mstats
mode 0, k_gather_prototypes) on probability features and tclip_cluster_prototypes_visual (k_vis_prototypes) on visual ones -
called through tclip_amd._capi on predictions of six patterns (tests/helpers/accuracy_tail.py: one cluster, min(Q, K) clusters
in and against sorted order, random, three classes spread over 0 .. K-1, every query alone but two), over K, Q, D and T away
from the fixtures' Q = 75.  Everything is compared with restatements computed here (pinned to the reference's fixtures by
tests/test_accuracy_tail.py); no output of the engine is stored.

  exact   n_clusters and cluster_ids equal first_appearance, the -1 padding up to Cmax = min(Q, K) included; prototype rows
          from n_clusters[t] on still hold the sentinel they were filled with.
  bits    rows [0, n_clusters[t]) have the bits of the fp32 restatement (torch's AVX-512 sum orders with at most 8 threads:
          on another host this tier skips).
  fp64    e(gpu) <= 2 e(ref32) over the same rows, e(a) = max |a - ref64| / max(|ref64|, tiny) - the kernels claim torch's
          summation order, so the expected ratio is 1.  Never skips.
  composition   engine.clustering_accuracy / clustering_accuracy_visual, graph_matching on and off, matching "host" and
          "device", at Q < K, Q > K and Q != 75: new_preds and acc equal ref_torch.clustering_accuracy (probability features)
          or prototypes_reference -> front-end formula -> scipy (visual ones), on inputs whose fp32 and float64 restatements
          assign alike.

Measured on an MI355X (AVX-512 host): 0 differing elements in the bit tier and e(gpu) / e(ref32) = 1.000 in the fp64 tier (both errors 0
where Q = 1), in all 81 cases of both feature kinds."""
import numpy as np
import pytest
import torch

from helpers import accuracy_tail as at
from oracle import ref_torch

pytestmark = pytest.mark.gpu

AVX512 = torch.backends.cpu.get_cpu_capability() == "AVX512"
bits_tier = pytest.mark.skipif(not AVX512, reason="torch's sum orders are pinned for the AVX-512 ATen kernels")
CASES = [(s, False) for s in at.PROB_SHAPES] + [(s, True) for s in at.VIS_SHAPES]
_ran = {}


def case_id(c):
    return ("vis_" + at.vis_id(c[0])) if c[1] else ("prob_" + at.prob_id(c[0]))


@pytest.fixture(scope="module", autouse=True)
def eight_threads():
    """torch's CPU reductions keep their order up to 8 threads (scripts/host_threads_check.py)"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    yield
    torch.set_num_threads(n)


def ran(case):
    """the restatements of a case and the kernels' raw arrays, the kernels run once"""
    if case not in _ran:
        c = at.prototype_case(*case)
        at.check_prototype_inputs(c, case[0])
        _ran[case] = (c, at.run_prototypes(c["preds"], c["z"], c["K"], case[1]))
    return _ran[case]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_clusters_in_first_appearance_order_and_nothing_written_beyond(case):
    c, (ncl, ids, protos) = ran(case)
    assert ncl.dtype == np.int32 and ids.dtype == np.int32 and ids.shape == c["ids"].shape
    assert np.array_equal(ncl, c["ncl"]), (ncl, c["ncl"])
    assert np.array_equal(ids, c["ids"])
    sentinel = np.float32(at.SENTINEL).view(np.int32)
    for t, n in enumerate(c["ncl"]):
        assert (protos[t, n:].view(np.int32) == sentinel).all(), f"task {t} ({c['patterns'][t]}): a row beyond its {n} clusters was written"
        assert np.isfinite(protos[t, :n]).all() and not (protos[t, :n] == np.float32(at.SENTINEL)).any(), f"task {t}"


@bits_tier
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prototype_rows_have_torchs_bits(case):
    c, (ncl, _, protos) = ran(case)
    assert np.array_equal(ncl, c["ncl"])
    bad = at.bit_differences(protos, c["ref32"].numpy(), c["ncl"])
    print(f"{case_id(case)}: {bad} differing elements of {int(c['ncl'].sum()) * c['W']}")
    assert bad == 0


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prototype_rows_within_fp64_bound(case):
    c, (ncl, _, protos) = ran(case)
    assert np.array_equal(ncl, c["ncl"])
    e_gpu = at.rel_err(torch.from_numpy(protos), c["ref64"], c["ncl"])
    e_ref = at.rel_err(c["ref32"], c["ref64"], c["ncl"])
    print(f"{case_id(case)}: e(gpu) {e_gpu:.3e}  e(ref32) {e_ref:.3e}  ratio {e_gpu / e_ref if e_ref else float(e_gpu > 0):.3f}")
    assert e_gpu <= 2 * e_ref


COMPOSE = [(s, False) for s in at.COMPOSE_PROB] + [(s, True) for s in at.COMPOSE_VIS]


@pytest.mark.parametrize("matching", ["host", "device"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "argmax"])
@pytest.mark.parametrize("case", COMPOSE, ids=case_id)
def test_engine_tail_equals_the_restatement(case, graph, matching):
    from tclip_amd import engine
    shape, visual = case
    c = at.compose_case(shape, visual)                   # asserts that the fp32 and float64 restatements assign alike
    x_q, preds, y = c["x_q"].cuda(), torch.from_numpy(c["preds"]).int().cuda(), torch.from_numpy(c["y"])
    if visual:
        acc, newp = engine.clustering_accuracy_visual(x_q, preds, y, c["text"], at.COMPOSE_T, graph_matching=graph, matching=matching)
        want_p, want_a = c["want", graph]
    else:
        acc, newp = engine.clustering_accuracy(x_q, preds, y, graph_matching=graph, matching=matching)
        hot = ref_torch.one_hot_rows(torch.from_numpy(c["preds"]), c["K"])
        ref_a, ref_p = ref_torch.clustering_accuracy(hot, c["x_q"], y, c["K"], graph_matching=graph)
        want_p, want_a = ref_p.numpy(), ref_a[:, 0].numpy()
        assert np.array_equal(want_p, c["want", graph][0])
    if matching == "device":
        acc = engine.match_status_ok(acc)
    acc, newp = acc.cpu().numpy(), newp.cpu().numpy()
    for t in range(len(want_a)):
        assert np.array_equal(newp[t], want_p[t]), f"task {t}"
    assert np.array_equal(acc, want_a)
