"""CPU: the value sweeps (tclip_*_sweep_tasks, engine.sweep_*_tasks, Evaluator_few_shot.evaluate_sweep, main_features.py
`sweep_values`): the eight names are declared, bound and exported; bad arguments are refused before any launch (every pointer
below is a fake address nothing may read); the workspace grows affinely with the number of values and LaplacianShot's stays
under twice the single call's; the Python layers refuse what they must without touching a device; and the evaluator falls back
to ordinary runs, value after value, when the tasks cannot be addressed in place."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from tclip_amd import _capi, engine

METHODS = ("paddle", "bdcspn", "laplacian_shot", "alpha_tim")
NEW = tuple(f"tclip_{m}_sweep_tasks{suffix}" for m in METHODS for suffix in ("_workspace_bytes", ""))
ERR_ARG, ERR_WORKSPACE = 1, 2


def test_names_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    version_comment = header[:header.index("#define TCLIP_ABI_VERSION")]
    later = version_comment[version_comment.index("later, without a new number"):]
    assert len(NEW) == 8
    for name in NEW:
        assert re.fullmatch(r"tclip_[a-z_]+", name)
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/tclip.h"
        assert name in _capi.EXPORTS and getattr(_capi.lib(), name).argtypes is not None
        assert re.search(r" T %s$" % name, exported, flags=re.M), f"{name} is not exported by libtclip.so"
        assert name in later, f"{name} is missing from the header's 'later' list"
    assert re.search(r"#define\s+TCLIP_ABI_VERSION\s+5\b", header)
    assert _capi.lib().tclip_abi_version() == 5


# ---- the C entries: every check comes before any HIP call --------------------------------------------------------------------

def _source(cols=None):
    return _capi.TaskSource(0x1000, 0x2000, 0x3000, 0x4000, cols)


def _prm(entropies=(0, 1, 1)):
    return _capi.TimParams(1e-4, 15.0, 0.0, (ctypes.c_float * 3)(1.0, 1.0, 1.0), (ctypes.c_int32 * 3)(*entropies))


NO_SRC, NO_VALUES = object(), object()
N_OUT = {"paddle": 4, "bdcspn": 3, "laplacian_shot": 4, "alpha_tim": 4}


def _call(method, p, dim=0, values=(1.5, 2.0), n_values=None, src=None, null=None, knn=3, ws=0x100000, ws_bytes=1 << 40, prm=None):
    """tclip_<method>_sweep_tasks on fake addresses; null: which of y_s and the outputs is NULL"""
    lib = _capi.lib()
    ptr = [ctypes.c_void_p(0x10000 * i) for i in range(1, 2 + N_OUT[method])]       # y_s, then the outputs
    if null is not None:
        ptr[null] = None
    vals = None if values is NO_VALUES else (ctypes.c_double * max(len(values), 1))(*values)
    n = ctypes.c_int32(len(values) if n_values is None else n_values)
    src_arg = None if src is NO_SRC else ctypes.byref(src or _source())
    y_s, outs, tail = ptr[0], ptr[1:], (ctypes.c_void_p(ws), ws_bytes, None)
    if method == "paddle":
        return lib.tclip_paddle_sweep_tasks(ctypes.byref(p), dim, src_arg, y_s, vals, n, *outs, *tail)
    if method == "bdcspn":
        return lib.tclip_bdcspn_sweep_tasks(ctypes.byref(p), dim, src_arg, y_s, vals, n, 1, *outs, *tail)
    if method == "laplacian_shot":
        return lib.tclip_laplacian_shot_sweep_tasks(ctypes.byref(p), dim, src_arg, y_s, knn, vals, n, 1, *outs, *tail)
    return lib.tclip_alpha_tim_sweep_tasks(ctypes.byref(p), dim, ctypes.byref(prm or _prm()), src_arg, y_s, vals, n, *outs, *tail)


def _ws(method, p, dim, n_values):
    return getattr(_capi.lib(), f"tclip_{method}_sweep_tasks_workspace_bytes")(ctypes.byref(p) if p is not None else None, dim, n_values)


@pytest.mark.parametrize("dim", [0, 512])
@pytest.mark.parametrize("method", METHODS)
def test_argument_errors_come_before_any_launch(method, dim):
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    assert _ws(method, p, dim, 2) > 0
    # null arguments
    assert _call(method, p, dim, src=NO_SRC) == ERR_ARG and b"null pointer" in lib.tclip_last_error()
    for field in ("table_q", "q_idx", "table_s", "s_idx"):
        src = _source()
        setattr(src, field, None)
        assert _call(method, p, dim, src=src) == ERR_ARG and b"null pointer" in lib.tclip_last_error()
    for null in range(1 + N_OUT[method]):
        assert _call(method, p, dim, null=null) == ERR_ARG and b"null pointer" in lib.tclip_last_error()
    assert _call(method, p, dim, ws=0) == ERR_ARG
    assert _call(method, p, dim, values=NO_VALUES, n_values=2) == ERR_ARG and b"null pointer" in lib.tclip_last_error()
    assert _ws(method, None, dim, 2) == 0
    # the values
    assert _call(method, p, dim, values=(), n_values=0) == ERR_ARG and b"n_values" in lib.tclip_last_error()
    assert _call(method, p, dim, n_values=-1) == ERR_ARG and _ws(method, p, dim, 0) == 0 and _ws(method, p, dim, -3) == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _call(method, p, dim, values=(2.0, bad)) == ERR_ARG and b"finite" in lib.tclip_last_error()
    assert _call(method, p, dim, values=(2.0,) * 40000) == ERR_ARG and _ws(method, p, dim, 40000) == 0       # 80000 solves
    # dim
    for bad in (-1, 1025):
        assert _call(method, p, bad) == ERR_ARG and b"dim" in lib.tclip_last_error() and _ws(method, p, bad, 2) == 0
    # cols belong to probability features
    if dim:
        assert _call(method, p, dim, src=_source(cols=0x5000)) == ERR_ARG and b"cols must be NULL" in lib.tclip_last_error()
    # the problem
    assert _call(method, _capi.Problem(1, 2, 75, 10, 0, 3, 1, 0, 0), dim) == ERR_ARG and b"n_support" in lib.tclip_last_error()
    assert _ws(method, _capi.Problem(1, 2, 75, 10, 0, 3, 1, 0, 0), dim, 2) == 0 or method == "alpha_tim"
    assert _call(method, _capi.Problem(1, 2, 75, 1025, 20, 3, 1, 0, 0), dim) == ERR_ARG and _ws(method, _capi.Problem(1, 2, 75, 1, 20, 3, 1, 0, 0), dim, 2) == 0
    if method in ("laplacian_shot", "alpha_tim"):
        assert _call(method, _capi.Problem(1, 2, 75, 10, 20, 0, 1, 0, 0), dim) == ERR_ARG and b"iters" in lib.tclip_last_error()
    if method == "laplacian_shot":
        for knn in (1, 76):
            assert _call(method, p, dim, knn=knn) == ERR_ARG and b"knn" in lib.tclip_last_error()
        big = _capi.Problem(1, 1, 1024, 10, 20, 3, 1, 0, 0)
        assert _call(method, big, dim, knn=1024) == ERR_ARG and b"LDS" in lib.tclip_last_error()
    if method == "alpha_tim":
        assert _call(method, p, dim, values=(2.0, 1.0)) == ERR_ARG and b"differ from 1" in lib.tclip_last_error()
        assert _call(method, p, dim, prm=_prm((0, 2, 1))) == ERR_ARG and b"entropies" in lib.tclip_last_error()
    # the workspace: short, then misaligned, named after the new query
    need = _ws(method, p, dim, 2)
    assert _call(method, p, dim, ws_bytes=need - 1) == ERR_WORKSPACE
    assert f"tclip_{method}_sweep_tasks_workspace_bytes".encode() in lib.tclip_last_error()
    assert _call(method, p, dim, ws=0x100010, ws_bytes=need) == ERR_WORKSPACE and b"aligned" in lib.tclip_last_error()


def test_alpha_value_of_the_params_is_not_read():
    """alpha_value = 1 in the struct would be refused by the single-value entry; the sweep reads its values only, and gets as
    far as the workspace check"""
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    prm = _prm()
    prm.alpha_value = 1.0
    assert _call("alpha_tim", p, 0, prm=prm, ws_bytes=16) == ERR_WORKSPACE
    # all three entropies Shannon: a value of 1 is as good as any other
    assert _call("alpha_tim", p, 0, values=(1.0,), prm=_prm((0, 0, 0)), ws_bytes=16) == ERR_WORKSPACE


@pytest.mark.parametrize("dim", [0, 512])
@pytest.mark.parametrize("T,Q,K,S", [(2, 75, 10, 20), (1, 75, 1000, 4000)])
@pytest.mark.parametrize("method", METHODS)
def test_workspace_grows_affinely_with_the_values(method, T, Q, K, S, dim):
    p = _capi.Problem(1, T, Q, K, S, 3, 1, 0, 0)
    w1, w2, w3, w9 = (_ws(method, p, dim, n) for n in (1, 2, 3, 9))
    assert w1 > 0 and w3 - w2 == w2 - w1 >= 0 and w9 - w3 == 6 * (w2 - w1)
    if method in ("paddle", "bdcspn"):       # the values run one after the other on one value's scratch
        assert w2 == w1
    else:
        assert w2 > w1


def test_laplacian_shot_shares_the_support_rows():
    """K = 1000, 4 shots: the 16 MB of normalised support rows, the class sums and the prototypes are held once; a value adds
    its fp64 assignments (2 * 75 * 1000 * 8 bytes).  From the layout: (25.6 + 9 * 1.2) / (25.6 + 1.2) = 1.36."""
    lib = _capi.lib()
    p = _capi.Problem(1, 1, 75, 1000, 4000, 20, 1, 0, 0)
    single = lib.tclip_laplacian_shot_tasks_workspace_bytes(ctypes.byref(p))
    nine = _ws("laplacian_shot", p, 0, 9)
    assert 0 < single < nine < 2 * single
    per_value = nine - _ws("laplacian_shot", p, 0, 8)                  # the assignments and the value, in 256-byte units
    assert 2 * 75 * 1000 * 8 + 8 <= per_value < 2 * 75 * 1000 * 8 + 8 + 2 * 256
    assert 1.3 < nine / single < 1.45


# ---- engine.sweep_*: refusals before the device -------------------------------------------------------------------------------

def _engine_calls():
    tab = torch.rand(30, 10)
    q_idx, s_idx, y_s = torch.randint(0, 30, (2, 15)), torch.randint(0, 30, (2, 20)), torch.arange(10).repeat(2, 2)
    return {"paddle": lambda values, t=tab: engine.sweep_paddle_tasks(t, q_idx, t, s_idx, y_s, iters=3, values=values),
            "bdcspn": lambda values, t=tab: engine.sweep_bdcspn_tasks(t, q_idx, t, s_idx, y_s, values=values),
            "laplacian_shot": lambda values, t=tab: engine.sweep_laplacian_shot_tasks(t, q_idx, t, s_idx, y_s, iters=3, knn=3, values=values),
            "alpha_tim": lambda values, t=tab: engine.sweep_alpha_tim_tasks(t, q_idx, t, s_idx, y_s, iters=3, temp=15.0, lr=1e-3,
                                                                            values=values)}


@pytest.mark.parametrize("method", METHODS)
def test_engine_refuses_bad_values_and_host_tensors(method):
    call = _engine_calls()[method]
    for bad in ([], (), [1.5, float("nan")], [float("inf")], 3.0, ["a"]):
        with pytest.raises(ValueError):
            call(bad)
    with pytest.raises(RuntimeError, match="GPU"):
        call([1.5, 2.0])


def test_engine_visual_form_checks_n_class_and_cols():
    tab = torch.rand(30, 10)
    q_idx, s_idx, y_s = torch.randint(0, 30, (2, 15)), torch.randint(0, 30, (2, 20)), torch.arange(10).repeat(2, 2)
    with pytest.raises(ValueError, match="n_class"):
        engine.sweep_paddle_tasks(tab, q_idx, tab, s_idx, y_s, iters=3, values=[1.0], n_class=1)
    with pytest.raises(ValueError, match="cols"):
        engine.sweep_bdcspn_tasks(tab, q_idx, tab, s_idx, y_s, torch.zeros(2, 10, dtype=torch.int32), values=[1.0], n_class=5)
    with pytest.raises(ValueError, match="Entropies"):
        engine.sweep_alpha_tim_tasks(tab, q_idx, tab, s_idx, y_s, iters=3, temp=15.0, lr=1e-3, values=[2.0], entropies=("Shannon", "Renyi", "Alpha"))
    with pytest.raises(ValueError, match="norm_type"):
        engine.sweep_laplacian_shot_tasks(tab, q_idx, tab, s_idx, y_s, iters=3, knn=3, values=[2.0], norm_type="CL2N")


# ---- the evaluator and the command line ---------------------------------------------------------------------------------------

def _args(method="PADDLE", **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=5, num_classes_test=10, n_class=10, n_query=15, k_eff=5, T=30.0, use_softmax_feature=True, name_method=method,
                lambd=5.0, temp=15.0, norm_type="L2N", knn=3, lmd=0.7, loss_weights=[1.0, 1.0, 1.0], lr_alpha_tim=1e-3, lr_tim=1e-3,
                entropies=["Shannon", "Alpha", "Alpha"], alpha_value=3.0, number_tasks=4, batch_size=2, shots=2, used_test_set="val",
                dataset="synthetic", tunable=True)
    a.update(kw)
    return a


def _refused(args, values):
    """through every door: the check itself, evaluate_sweep (no table is looked at) and run_full_evaluation (no file is)"""
    from src.eval_few_shot import Evaluator_few_shot, checked_sweep_values
    yield lambda: checked_sweep_values(args, values)
    yield lambda: Evaluator_few_shot(device="cpu", args=args, log_file=None).evaluate_sweep(None, None, None, None, None, values)
    args = type(args)(args)
    args.sweep_values = values
    yield lambda: Evaluator_few_shot(device="cpu", args=args, log_file=None).run_full_evaluation(None, None)


def test_sweep_refusals_need_no_gpu(monkeypatch):
    for call in _refused(_args(used_test_set="test"), [1.0, 2.0]):
        with pytest.raises(ValueError, match="used_test_set must be 'val'"):
            call()
    for method in ("EM_DIRICHLET", "TIM-GD"):
        for call in _refused(_args(method), [1.0, 2.0]):
            with pytest.raises(ValueError, match="no validation-tuned parameter"):
                call()
    for bad in ([], (), None, 3.0, "1.0"):
        for call in list(_refused(_args(), bad))[:2]:
            with pytest.raises(ValueError, match="non-empty list"):
                call()
    for bad in ([1.0, "a"], [None], [True], [float("nan")], [1.0, float("inf")], [[1.0]]):
        for call in _refused(_args(), bad):
            with pytest.raises(ValueError, match="finite numbers"):
                call()
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    for call in _refused(_args(), [1.0, 2.0]):
        with pytest.raises(RuntimeError, match="single-process"):
            call()


def test_checked_values_keep_their_literal_types():
    from src.eval_few_shot import checked_sweep_values
    got = checked_sweep_values(_args(), (5, 5.0, 1e1))
    assert got == [5, 5.0, 10.0] and [type(v) for v in got] == [int, float, float] and [str(v) for v in got] == ["5", "5.0", "10.0"]


def test_main_features_refuses_before_the_device(monkeypatch, tmp_path):
    sys.path.insert(0, PKG)
    import main_features
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("the device was touched before the sweep was refused"))
    base = ["--results-root", str(tmp_path), "--opts", "dataset", "synthetic", "shots", "2"]
    ns, cfg = main_features.parse_args(base + ["method", "paddle", "used_test_set", "val", "sweep_values", "[1.0, 2, 5.0]"])
    assert cfg.sweep_values == [1.0, 2, 5.0] and [type(v) for v in cfg.sweep_values] == [float, int, float]
    with pytest.raises(ValueError, match="used_test_set must be 'val'"):
        main_features.main(base + ["method", "paddle", "sweep_values", "[1.0, 2.0]"])
    with pytest.raises(ValueError, match="no validation-tuned parameter"):
        main_features.main(base + ["method", "tim", "used_test_set", "val", "sweep_values", "[1.0, 2.0]"])
    with pytest.raises(ValueError, match="non-empty list"):
        main_features.main(base + ["method", "paddle", "used_test_set", "val", "sweep_values", "[]"])
    with pytest.raises(ValueError, match="finite numbers"):
        main_features.main(base + ["method", "paddle", "used_test_set", "val", "sweep_values", "[1.0, 'x']"])
    with pytest.raises(ValueError, match="shots must be positive"):
        main_features.main(["--results-root", str(tmp_path), "--opts", "dataset", "synthetic", "method", "paddle", "used_test_set", "val",
                            "sweep_values", "[1.0]"])
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(RuntimeError, match="single-process"):
        main_features.main(base + ["method", "paddle", "used_test_set", "val", "sweep_values", "[1.0, 2.0]"])


def test_tunable_classes_name_their_swept_attribute():
    from src import eval_few_shot
    from tclip_amd import reporting
    for method, attr in reporting.VAL_PARAM.items():
        assert eval_few_shot._METHODS[method].SWEEP_ATTR == attr == eval_few_shot.Evaluator_few_shot._TUNED[method]
    for method in ("EM_DIRICHLET", "HARD_EM_DIRICHLET", "TIM-GD"):
        cls = eval_few_shot._METHODS[method]
        assert cls.SWEEP_ATTR is None
        with pytest.raises(NotImplementedError, match="no validation-tuned parameter"):
            cls.run_tables_sweep([object()], None, None, None, None, None, None, None)


class _Recorder:
    def __init__(self):
        self.calls = []

    def stub(self, name, result=None):
        def f(*a, **kw):
            self.calls.append((name, kw))
            if result is None:
                raise AssertionError(f"{name} must not be called here")
            return result(*a, **kw)
        return f


def _tables():
    from tclip_amd import synth
    return synth.make_feature_table(10, 12, seed=9100) + synth.make_feature_table(10, 12, seed=9101)


@pytest.mark.parametrize("method,attr,single", [("PADDLE", "lambd", "run_paddle"), ("BDCSPN", "temp", "run_bdcspn"),
                                                ("LAPLACIAN_SHOT", "lmd", "run_laplacian_shot"), ("ALPHA_TIM", "alpha_value", "run_alpha_tim")])
def test_evaluate_sweep_falls_back_to_ordinary_runs(method, attr, single, monkeypatch):
    """A support set that misses a class (relabel_indices returns None): no sweep entry is called; every value goes through
    evaluate_tasks' own route for such tasks - the materialised tensors and the method's single-value engine call - in the order
    given, on the indices drawn once.  The engine is replaced by recording stubs; the device by the host."""
    from src import eval_few_shot
    from src.methods._em_dirichlet_base import MethodBase
    rec = _Recorder()
    values = [7.5, 2.5, 4.0]
    for name in ("sweep_paddle_tasks", "sweep_bdcspn_tasks", "sweep_laplacian_shot_tasks", "sweep_alpha_tim_tasks", "run_paddle_tasks",
                 "run_bdcspn_tasks", "run_laplacian_shot_tasks", "run_alpha_tim_tasks", "gather_task_rows"):
        monkeypatch.setattr(engine, name, rec.stub(name))
    monkeypatch.setattr(engine, "gather_rows", lambda table, idx: table[idx])

    def result(x_q, x_s, y_s, **kw):
        T, Q, K = x_q.shape
        preds = torch.zeros(T, Q, dtype=torch.int32)
        if method == "PADDLE":
            return torch.zeros(T, Q, K), torch.zeros(T, K), torch.zeros(T, K, K), preds
        if method == "BDCSPN":
            return torch.zeros(T, K, K), torch.zeros(T, Q, K), preds
        if method == "LAPLACIAN_SHOT":
            return torch.zeros(T, Q, K), torch.zeros(T, Q, 2, dtype=torch.int32), torch.zeros(T, kw["iters"], Q, dtype=torch.int32), \
                torch.zeros(T, kw["iters"], dtype=torch.float64)
        return torch.zeros(T, K, K), torch.zeros(T, Q, K), preds, torch.zeros(kw["n_batches"], kw["iters"])
    monkeypatch.setattr(engine, single, rec.stub(single, result))
    monkeypatch.setattr(MethodBase, "_cuda_device", lambda self, name=None: torch.device("cpu"))
    monkeypatch.setattr(MethodBase, "_timed", lambda self, call: (call(), 1.0))

    args = _args(method)
    ev = eval_few_shot.Evaluator_few_shot(device="cpu", args=args, log_file=None)
    tabs = _tables()
    np.random.seed(5)
    indices = ev.sample_indices(tabs[1].numpy(), tabs[3].numpy())
    ordinary = []
    evaluate_tasks = ev.evaluate_tasks
    monkeypatch.setattr(ev, "evaluate_tasks", lambda *a, **kw: (ordinary.append((args[attr], kw["indices"])), evaluate_tasks(*a, **kw))[1])
    monkeypatch.setattr(eval_few_shot, "relabel_indices", lambda *a, **k: None)
    accs, mean_time = ev.evaluate_sweep(None, *tabs, values=values, indices=indices)
    assert accs.shape == (3,) and mean_time > 0
    assert [v for v, _ in ordinary] == values and all(i is not None and i[0] is indices[0] and i[1] is indices[1] for _, i in ordinary)
    assert [name for name, _ in rec.calls] == [single] * 3
    assert [kw[attr] for _, kw in rec.calls] == values
    assert args[attr] == _args(method)[attr]                           # the evaluator's args are as they were
