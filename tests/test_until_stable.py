"""CPU: the until-stable entries (tclip_em_dirichlet_run_until_stable and its table twin) are declared, bound and exported, check
their arguments without touching a GPU, and the stop rule they implement - restated on the host in tests/helpers/until_stable.py
- gives, on the reference's own argmax traces, the stop counts the GPU tests expect."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import until_stable as us
from tclip_amd import _capi

NAMES = ("tclip_em_dirichlet_until_stable_workspace_bytes", "tclip_em_dirichlet_run_until_stable",
         "tclip_em_dirichlet_run_tasks_until_stable")


def test_entries_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tclip.h")).read(), flags=re.S)
    lib = _capi.lib()
    for name in NAMES:
        assert name + "(" in header and name in _capi.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert lib.tclip_abi_version() == 5


def test_workspace_query():
    lib = _capi.lib()
    for p in (_capi.Problem(10, 100, 75, 100, 0, 20, 1000, 1500, 0),        # three stream groups
              _capi.Problem(4, 41, 75, 100, 0, 20, 1000, 1500, 0),          # two
              _capi.Problem(1, 3, 75, 37, 74, 10, 1000, 525, 1)):           # one, few-shot
        plain = lib.tclip_workspace_bytes(ctypes.byref(p))
        got = lib.tclip_em_dirichlet_until_stable_workspace_bytes(ctypes.byref(p))
        T = p.n_batches * p.tasks_per_batch
        assert plain > 0 and got >= plain + 4 * T * p.n_query + 8 * p.n_batches        # prev_preds, quiet and done on top
    bad = _capi.Problem(1, 1, 75, 2000, 0, 20, 1000, 1, 0)
    assert lib.tclip_workspace_bytes(ctypes.byref(bad)) == 0
    plain_text = lib.tclip_last_error()
    assert lib.tclip_em_dirichlet_until_stable_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.tclip_last_error() == plain_text and b"n_class" in plain_text


def test_argument_checks_touch_no_gpu():
    lib = _capi.lib()
    p = _capi.Problem(2, 3, 75, 10, 0, 20, 1000, 150, 0)
    one = ctypes.c_void_p(256)          # never dereferenced: the refusals come first
    src = _capi.TaskSource(256, 256, None, None, None)
    outs = [one] * 6
    # patience = 0
    assert lib.tclip_em_dirichlet_run_until_stable(ctypes.byref(p), one, None, None, 0, *outs, one, one, one, 0, None) == 1
    assert b"patience" in lib.tclip_last_error()
    assert lib.tclip_em_dirichlet_run_tasks_until_stable(ctypes.byref(p), ctypes.byref(src), None, 0, *outs, one, one, one, 0, None) == 1
    assert b"patience" in lib.tclip_last_error()
    # null outer_iters / changes
    assert lib.tclip_em_dirichlet_run_until_stable(ctypes.byref(p), one, None, None, 2, *outs, None, one, one, 0, None) == 1
    assert b"outer_iters" in lib.tclip_last_error()
    assert lib.tclip_em_dirichlet_run_tasks_until_stable(ctypes.byref(p), ctypes.byref(src), None, 2, *outs, None, one, one, 0, None) == 1
    assert b"outer_iters" in lib.tclip_last_error()
    assert lib.tclip_em_dirichlet_run_until_stable(ctypes.byref(p), one, None, None, 2, *outs, one, None, one, 0, None) == 1
    assert b"changes" in lib.tclip_last_error()
    # the plain entries' checks: a null output, a support set without labels
    assert lib.tclip_em_dirichlet_run_until_stable(ctypes.byref(p), one, None, None, 2, None, *outs[1:], one, one, one, 0, None) == 1
    assert lib.tclip_em_dirichlet_run_until_stable(ctypes.byref(p), one, one, None, 2, *outs, one, one, one, 0, None) == 1
    assert b"x_s and y_s" in lib.tclip_last_error()
    # a workspace smaller than the query's answer is the workspace error (2), named after the query
    assert lib.tclip_em_dirichlet_run_until_stable(ctypes.byref(p), one, None, None, 2, *outs, one, one, one, 0, None) == 2
    assert b"tclip_em_dirichlet_until_stable_workspace_bytes" in lib.tclip_last_error()


def test_module_refusals():
    from tclip_amd import engine, until_stable
    x = torch.full((2, 75, 10), 0.1)
    for bad in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="patience"):
            until_stable.run_em_dirichlet(x, patience=bad, iters=3, lambd=150)
        with pytest.raises(ValueError, match="patience"):
            until_stable.run_em_dirichlet_tasks(x[0], torch.zeros(2, 75, dtype=torch.long), patience=bad, iters=3, lambd=150)
    # the plain functions' refusals, by type and text
    for mod, kw in ((engine, {}), (until_stable, {"patience": 2})):
        with pytest.raises(RuntimeError, match="x_q must live on the GPU"):
            mod.run_em_dirichlet(x, iters=3, lambd=150, **kw)
        with pytest.raises(RuntimeError, match="table_q must live on the GPU"):
            mod.run_em_dirichlet_tasks(x[0], torch.zeros(2, 75, dtype=torch.long), iters=3, lambd=150, **kw)
    assert until_stable.check_patience(np.int64(3)) == 3
    assert until_stable.UntilStableResult.__slots__ == engine.EMDirichletResult.__slots__ + ("outer_iters", "changes")


@pytest.mark.parametrize("name", sorted(us.STOPS))
def test_restated_rule_on_the_reference_traces(name):
    """the table of stop counts: what the reference's argmax after every outer iteration gives under the rule"""
    g = us.load(name)
    argmax = g["argmax"]
    assert argmax.shape[0] == int(g["iters"]) and argmax.ndim == 3
    changes = us.changes_of(argmax)
    assert changes[0] == argmax.shape[1] * argmax.shape[2]
    assert tuple(us.stop_of(changes, p) for p in (1, 2, 3)) == us.STOPS[name]
    if name in us.CHANGES_HEAD:
        head = us.CHANGES_HEAD[name]
        assert changes[1:1 + len(head)].tolist() == head
    for p in (1, 2, 3):
        s = us.stop_of(changes, p)
        assert s == len(changes) or (s >= p + 1 and (changes[s - p:s] == 0).all())


def test_the_gpu_cases_really_stop_early():
    """the fixtures the GPU test runs with patience 2 stop before their last iteration with the final assignment (K >= 37), and
    its two never-stopping cases run every iteration"""
    for name in ("zs_soft_K10_N4", "zs_soft_K37_N6", "zs_soft_K100_N4", "zs_hard_K37_N6", "fs_soft_K37_N3_s2",
                 "fs_hard_K10_N4_s4", "zs_soft_K1000_N3"):
        g = us.load(name)
        s = us.STOPS[name][1]
        assert s < int(g["iters"])
        if int(g["K"]) >= 37:
            assert np.array_equal(g["argmax"][s - 1], g["argmax"][-1])
    assert us.STOPS["zs_soft_K7_N4"][2] == 20 and us.STOPS["fs_hard_K100_N3_s4"][1] == 10


def _args(method, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=3, iter_mm=100, num_classes_test=10, n_class=10, n_query=75, k_eff=5, T=30, shots=2, use_softmax_feature=True,
                graph_matching=True, name_method=method, lambd=1.0, number_tasks=2, batch_size=1, used_test_set="test",
                dataset="synthetic", tunable=False)
    a.update(kw)
    return a


@pytest.mark.parametrize("method", ["SOFT_KMEANS", "PADDLE"])
def test_other_methods_refuse_the_option(method):
    """before any device work: the tables are CPU tensors, the device is one this machine may not have, nothing is drawn"""
    from src.eval_few_shot import Evaluator_few_shot
    from src.eval_zero_shot import Evaluator_zero_shot
    feats, labels = torch.full((40, 10), 0.1), torch.arange(10).repeat_interleave(4)
    if method == "PADDLE":
        ev = Evaluator_few_shot(device=torch.device("cuda:0"), args=_args(method, stop_patience=2), log_file=None)
        call = lambda: ev.evaluate_tasks(None, feats, labels, feats, labels)      # noqa: E731
    else:
        ev = Evaluator_zero_shot(device=torch.device("cuda:0"), args=_args(method, stop_patience=2), log_file=None)
        call = lambda: ev.evaluate_tasks(None, feats, labels)      # noqa: E731
    with pytest.raises(ValueError, match="stop_patience"):
        call()


def test_the_option_is_absent_unless_given():
    from src._evaluator import arg_hidden, check_stop_patience
    from src.methods.zero_shot.em_dirichlet import EM_DIRICHLET
    from tclip_amd import sharding
    a = _args("EM_DIRICHLET")
    assert check_stop_patience(a) is None and "stop_patience" not in a
    m = EM_DIRICHLET(model=None, device=torch.device("cpu"), log_file=None, args=a)
    assert m._stop_patience() is None and "stop_patience" not in a          # not written into args as a default
    assert sorted(sharding.method_parts(a, None, None, 0, 2, 75, torch.device("cpu"))) == ["acc", "criterions", "mm_iters", "preds"]
    a.stop_patience = 2
    assert check_stop_patience(a) == 2 and m._stop_patience() == 2
    parts = sharding.method_parts(a, None, None, 0, 2, 75, torch.device("cpu"))
    assert sorted(parts) == ["acc", "criterions", "mm_iters", "outer_iters", "preds"] and parts["outer_iters"].shape == (0, 1)
    with arg_hidden(a, "stop_patience"):
        assert check_stop_patience(a) is None
    assert a.stop_patience == 2
    # a bad value is refused by the class before the engine is asked
    a.stop_patience = 0
    with pytest.raises(ValueError, match="patience"):
        m._run_engine(torch.full((2, 75, 10), 0.1))


@pytest.mark.parametrize("name", sorted(us.SYNTHETIC))
def test_recorded_stops_of_the_synthetic_calls(name):
    """what the GPU test asserts for its calls of several batches, from oracle.ref_torch on the CPU: at least two distinct
    values, at least one below iters"""
    c = us.synthetic_case(name)
    stops, _ = us.reference_stops(c["x_q"], c["x_s"], c["y_s"], len(c["specs"]), c["patience"], iters=c["iters"],
                                  iter_mm=c["iter_mm"], lambd=c["lambd"], hard=False)
    assert stops == c["stops"]
    assert len(set(stops)) >= 2 and min(stops) < c["iters"]
    if name == "two_groups":
        assert len(c["specs"]) * c["N"] * c["K"] == 16400        # n_groups_of: 16 400 // 8192 = 2 stream groups
    if name == "isolation":
        assert stops[0] < c["iters"] == stops[-1]


def test_tables_hold_the_tasks():
    c = us.synthetic_case("few_shot")
    table_q, q_idx, table_s, s_idx, cols = us.as_tables(c["x_q"], c["x_s"], seed=5)
    for tab, idx, x in ((table_q, q_idx, c["x_q"]), (table_s, s_idx, c["x_s"])):
        got = torch.gather(tab[idx], 2, cols.long()[:, None, :].expand_as(x))
        assert torch.equal(got, x)
