"""CPU: ALPHA_TIM and TIM_GD fed from the feature tables (tclip_alpha_tim[_visual]_run_tasks, tclip_tim_gd_run_tasks): the six
names are declared, bound and exported, each workspace query returns what its dense counterpart returns, bad arguments are
refused before any launch (every pointer below is a fake address nothing may read), and the opt-in switch of the drop-in
classes (`IN_PLACE_LOOP`, `can_read_rows_in_place_per_step`, `in_place_loop`)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from tclip_amd import _capi

NEW = ("tclip_alpha_tim_tasks_workspace_bytes", "tclip_alpha_tim_run_tasks", "tclip_alpha_tim_visual_tasks_workspace_bytes",
       "tclip_alpha_tim_visual_run_tasks", "tclip_tim_gd_tasks_workspace_bytes", "tclip_tim_gd_run_tasks")
ERR_ARG, ERR_WORKSPACE = 1, 2


def test_names_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    version_comment = header[:header.index("#define TCLIP_ABI_VERSION")]
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/tclip.h"
        assert name in _capi.EXPORTS and getattr(_capi.lib(), name).argtypes is not None
        assert re.search(r" T %s$" % name, exported, flags=re.M), f"{name} is not exported by libtclip.so"
        assert name in version_comment, f"{name} is missing from the header's version comment"
    assert re.search(r"#define\s+TCLIP_ABI_VERSION\s+5\b", header)
    assert _capi.lib().tclip_abi_version() == 5


# (n_batches, tasks per batch, Q, K, S, D of the visual entries): a small one, the K = 1000 / 4 shots case, odd sizes
PROBLEMS = [(1, 3, 75, 10, 20, 512), (1, 100, 75, 1000, 4000, 1024), (2, 2, 10, 37, 65, 33)]


@pytest.mark.parametrize("B,N,Q,K,S,D", PROBLEMS)
def test_workspace_queries_equal_the_dense_ones(B, N, Q, K, S, D):
    lib = _capi.lib()
    p = ctypes.byref(_capi.Problem(B, N, Q, K, S, 5, 1, 0, 0))
    assert lib.tclip_alpha_tim_tasks_workspace_bytes(p) == lib.tclip_alpha_tim_workspace_bytes(p) > 0
    for dim in (D, K):
        assert lib.tclip_alpha_tim_visual_tasks_workspace_bytes(p, dim) == lib.tclip_alpha_tim_visual_workspace_bytes(p, dim) > 0
        assert lib.tclip_tim_gd_tasks_workspace_bytes(p, dim) == lib.tclip_tim_gd_workspace_bytes(p, dim) > 0
    # and what the dense queries refuse, these refuse
    for dim in (0, 1025):
        assert lib.tclip_alpha_tim_visual_tasks_workspace_bytes(p, dim) == 0 and lib.tclip_tim_gd_tasks_workspace_bytes(p, dim) == 0
    assert lib.tclip_alpha_tim_tasks_workspace_bytes(None) == 0 and lib.tclip_tim_gd_tasks_workspace_bytes(None, D) == 0
    assert lib.tclip_tim_gd_tasks_workspace_bytes(ctypes.byref(_capi.Problem(B, N, Q, K, 0, 5, 1, 0, 0)), D) == 0


def _source(cols=None):
    return _capi.TaskSource(0x1000, 0x2000, 0x3000, 0x4000, cols)


def _prm(alpha_value=7.0, entropies=(0, 1, 1)):
    return _capi.TimParams(1e-4, 15.0, alpha_value, (ctypes.c_float * 3)(1.0, 1.0, 1.0), (ctypes.c_int32 * 3)(*entropies))


NO_SRC = object()


def _alpha(p, dim=None, ws=0x100000, ws_bytes=1 << 40, src=None, null=None, prm=None):
    """tclip_alpha_tim_run_tasks, or with `dim` tclip_alpha_tim_visual_run_tasks; null: which of y_s, weights, logits_q, preds,
    criterions is NULL"""
    ptr = [ctypes.c_void_p(0x10000 * i) for i in range(1, 6)]
    if null is not None:
        ptr[null] = None
    lib = _capi.lib()
    entry, lead = (lib.tclip_alpha_tim_run_tasks, ()) if dim is None else (lib.tclip_alpha_tim_visual_run_tasks, (dim,))
    src_arg = None if src is NO_SRC else ctypes.byref(src or _source())
    return entry(ctypes.byref(p), *lead, ctypes.byref(prm or _prm()), src_arg, *ptr, ctypes.c_void_p(ws), ws_bytes, None)


def _gd(p, dim=None, ws=0x100000, ws_bytes=1 << 40, src=None, null=None, prm=None):
    """tclip_tim_gd_run_tasks on rows of `dim` elements (None: dim = n_class); null as for _alpha"""
    ptr = [ctypes.c_void_p(0x10000 * i) for i in range(1, 6)]
    if null is not None:
        ptr[null] = None
    src_arg = None if src is NO_SRC else ctypes.byref(src or _source())
    return _capi.lib().tclip_tim_gd_run_tasks(ctypes.byref(p), p.n_class if dim is None else dim, ctypes.c_double(1e-4),
                                              ctypes.c_float(15.0), (ctypes.c_float * 3)(1.0, 0.3, 1.0), src_arg, *ptr,
                                              ctypes.c_void_p(ws), ws_bytes, None)


def _query(call, dim):
    lib = _capi.lib()
    if call is _gd:
        return lambda p: lib.tclip_tim_gd_tasks_workspace_bytes(p, 10 if dim is None else dim), b"tclip_tim_gd_tasks_workspace_bytes"
    if dim is None:
        return lib.tclip_alpha_tim_tasks_workspace_bytes, b"tclip_alpha_tim_tasks_workspace_bytes"
    return (lambda p: lib.tclip_alpha_tim_visual_tasks_workspace_bytes(p, dim)), b"tclip_alpha_tim_visual_tasks_workspace_bytes"


@pytest.mark.parametrize("call", [_alpha, _gd])
@pytest.mark.parametrize("dim", [None, 512])
def test_argument_errors_come_before_any_launch(call, dim):
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    assert call(p, dim, src=NO_SRC) == ERR_ARG and b"null pointer" in lib.tclip_last_error()
    for field in ("table_q", "q_idx", "table_s", "s_idx"):
        src = _source()
        setattr(src, field, None)
        assert call(p, dim, src=src) == ERR_ARG and b"null pointer" in lib.tclip_last_error()
    for null in range(5):
        assert call(p, dim, null=null) == ERR_ARG
    assert call(p, dim, ws=0) == ERR_ARG                                # a null workspace is a null pointer
    assert call(_capi.Problem(1, 2, 75, 10, 0, 3, 1, 0, 0), dim) == ERR_ARG and b"n_support" in lib.tclip_last_error()
    assert call(_capi.Problem(1, 2, 75, 10, 20, 0, 1, 0, 0), dim) == ERR_ARG and b"iters" in lib.tclip_last_error()
    assert call(_capi.Problem(1, 2, 75, 1025, 20, 3, 1, 0, 0), dim) == ERR_ARG
    assert call(_capi.Problem(1, 2, 75, 1, 20, 3, 1, 0, 0), dim) == ERR_ARG
    # the workspace: short, then misaligned, named after the new query
    query, name = _query(call, dim)
    need = query(ctypes.byref(p))
    assert need > 0
    assert call(p, dim, ws_bytes=need - 1) == ERR_WORKSPACE and name in lib.tclip_last_error()
    assert call(p, dim, ws=0x100010, ws_bytes=need) == ERR_WORKSPACE and b"aligned" in lib.tclip_last_error()


def test_cols_belong_to_probability_features():
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    with_cols = _source(cols=0x5000)
    assert _alpha(p, 512, src=with_cols) == ERR_ARG and b"cols" in lib.tclip_last_error()
    assert _alpha(p, 10, src=with_cols) == ERR_ARG and b"cols" in lib.tclip_last_error()      # the visual entry never takes them
    assert _gd(p, 512, src=with_cols) == ERR_ARG and b"cols" in lib.tclip_last_error()
    assert _gd(p, 11, src=with_cols) == ERR_ARG and b"cols" in lib.tclip_last_error()
    # accepted where dim == n_class (the next refusal is the workspace's)
    assert _alpha(p, src=with_cols, ws_bytes=1) == ERR_WORKSPACE
    assert _gd(p, 10, src=with_cols, ws_bytes=1) == ERR_WORKSPACE
    for dim in (0, 1025):
        assert _alpha(p, dim) == ERR_ARG and b"dim" in lib.tclip_last_error()
        assert _gd(p, dim) == ERR_ARG and b"dim" in lib.tclip_last_error()


def test_alpha_tim_parameter_checks_are_the_dense_entrys():
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    for dim in (None, 512):
        assert _alpha(p, dim, prm=_prm(entropies=(0, 2, 1))) == ERR_ARG and b"entropies" in lib.tclip_last_error()
        assert _alpha(p, dim, prm=_prm(alpha_value=1.0)) == ERR_ARG and b"alpha_value" in lib.tclip_last_error()
        assert _alpha(p, dim, prm=_prm(alpha_value=1.0, entropies=(0, 0, 0)), ws_bytes=1) == ERR_WORKSPACE


def test_opt_in_switch_of_the_classes():
    from src.methods._em_dirichlet_base import FewShotMixin
    from src.methods.few_shot.bdcspn import BDCSPN
    from src.methods.few_shot.em_dirichlet import EM_DIRICHLET
    from src.methods.few_shot.hard_em_dirichlet import HARD_EM_DIRICHLET
    from src.methods.few_shot.laplacian_shot import LAPLACIAN_SHOT
    from src.methods.few_shot.paddle import PADDLE
    from src.methods.few_shot.tim import ALPHA_TIM, TIM_GD
    assert FewShotMixin.IN_PLACE_LOOP == () and TIM_GD.IN_PLACE_LOOP == ("softmax", "visual") and ALPHA_TIM.IN_PLACE_LOOP == ("softmax",)
    assert (TIM_GD.can_read_rows_in_place_per_step(True), TIM_GD.can_read_rows_in_place_per_step(False)) == (True, True)
    assert (ALPHA_TIM.can_read_rows_in_place_per_step(True), ALPHA_TIM.can_read_rows_in_place_per_step(False)) == (True, False)
    for cls in (EM_DIRICHLET, HARD_EM_DIRICHLET, PADDLE, BDCSPN, LAPLACIAN_SHOT):
        assert cls.IN_PLACE_LOOP == ()
        assert (cls.can_read_rows_in_place_per_step(True), cls.can_read_rows_in_place_per_step(False)) == (False, False)
    # the two older questions are answered as before
    for cls in (TIM_GD, ALPHA_TIM):
        assert cls.IN_PLACE_FEATURES == () and cls.IN_PLACE_SUPPORT == ()
        assert (cls.reads_rows_in_place(True), cls.reads_rows_in_place(False)) == (False, False)
        assert (cls.can_read_rows_in_place(True), cls.can_read_rows_in_place(False)) == (False, False)
        assert cls.run_tables is not FewShotMixin.run_tables
    assert (BDCSPN.can_read_rows_in_place(True), BDCSPN.can_read_rows_in_place(False)) == (True, True)
    assert (LAPLACIAN_SHOT.can_read_rows_in_place(True), LAPLACIAN_SHOT.can_read_rows_in_place(False)) == (True, False)
    assert PADDLE.reads_rows_in_place(True) and PADDLE.reads_rows_in_place(False)
    assert EM_DIRICHLET.reads_rows_in_place(True) and not EM_DIRICHLET.reads_rows_in_place(False)


def test_alpha_tim_run_tables_refuses_visual_features():
    import torch
    from src.methods.few_shot.tim import ALPHA_TIM
    from src.utils import CfgNode
    a = CfgNode(iter=3, num_classes_test=10, n_class=10, n_query=75, k_eff=5, T=30, shots=2, use_softmax_feature=False, temp=15,
                loss_weights=[1.0, 1.0, 1.0], lr_alpha_tim=1e-4, entropies=["Shannon", "Alpha", "Alpha"], alpha_value=7.0)
    m = ALPHA_TIM(model=None, device=torch.device("cpu"), log_file=None, args=a)
    tab = torch.zeros(8, 64)
    idx = torch.zeros(2, 20, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="probability features"):
        m.run_tables(table_s=tab, s_idx=idx, table_q=tab, q_idx=idx, cols=None, y_s=idx, y_q=idx)
    with pytest.raises(NotImplementedError, match="probability features"):
        m.run_method(support=tab.view(1, 8, 64), query=tab.view(1, 8, 64), y_s=idx, y_q=idx)


def test_main_features_takes_the_option():
    import main_features
    _, cfg = main_features.parse_args(["--opts", "method", "tim", "shots", "4", "in_place_loop", "True"])
    assert cfg.in_place_loop is True and cfg.name_method in ("TIM-GD", "TIM_GD")
    _, cfg = main_features.parse_args(["--opts", "method", "alpha_tim", "shots", "4"])
    assert getattr(cfg, "in_place_loop", False) is False
    assert "in_place_loop" not in main_features.MAIN_DEFAULTS
    assert "in_place_loop" in main_features.__doc__
