"""CPU: BD-CSPN and LAPLACIAN_SHOT fed from the feature tables (tclip_bdcspn[_visual]_run_tasks,
tclip_laplacian_shot[_visual]_run_tasks): the eight names are declared, bound and exported, bad arguments are refused before
any launch (every pointer below is a fake address nothing may read), the workspace arithmetic - BD-CSPN's normalised support
rows share the logits' region, LaplacianShot's workspace is the dense one -, and the opt-in switch of the drop-in classes."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from tclip_amd import _capi

NEW = ("tclip_bdcspn_tasks_workspace_bytes", "tclip_bdcspn_run_tasks", "tclip_bdcspn_visual_tasks_workspace_bytes",
       "tclip_bdcspn_visual_run_tasks", "tclip_laplacian_shot_tasks_workspace_bytes", "tclip_laplacian_shot_run_tasks",
       "tclip_laplacian_shot_visual_tasks_workspace_bytes", "tclip_laplacian_shot_visual_run_tasks")
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


def _source(cols=None):
    return _capi.TaskSource(0x1000, 0x2000, 0x3000, 0x4000, cols)


def _bdcspn(p, dim=None, ws=0x100000, ws_bytes=1 << 40, src=None, null=None, norm_type=1):
    """tclip_bdcspn_run_tasks, or with `dim` tclip_bdcspn_visual_run_tasks; null: which of y_s, prototypes, u, preds is NULL"""
    ptr = [ctypes.c_void_p(0x10000 * i) for i in range(1, 5)]
    if null is not None:
        ptr[null] = None
    lib = _capi.lib()
    entry, lead = (lib.tclip_bdcspn_run_tasks, ()) if dim is None else (lib.tclip_bdcspn_visual_run_tasks, (dim,))
    return entry(ctypes.byref(p), *lead, ctypes.byref(src or _source()), ptr[0], ctypes.c_float(15.0), norm_type, *ptr[1:],
                 ctypes.c_void_p(ws), ws_bytes, None)


def _lshot(p, dim=None, ws=0x100000, ws_bytes=1 << 40, src=None, null=None, norm_type=1, knn=3):
    """tclip_laplacian_shot_run_tasks / _visual_run_tasks; null: which of y_s, unary, neighbours, preds_iter, energies is NULL"""
    ptr = [ctypes.c_void_p(0x10000 * i) for i in range(1, 6)]
    if null is not None:
        ptr[null] = None
    lib = _capi.lib()
    entry, lead = (lib.tclip_laplacian_shot_run_tasks, ()) if dim is None else (lib.tclip_laplacian_shot_visual_run_tasks, (dim,))
    return entry(ctypes.byref(p), *lead, ctypes.byref(src or _source()), ptr[0], knn, ctypes.c_double(0.7), norm_type, *ptr[1:],
                 ctypes.c_void_p(ws), ws_bytes, None)


def _queries(dim):
    lib = _capi.lib()
    if dim is None:
        return lib.tclip_bdcspn_tasks_workspace_bytes, lib.tclip_laplacian_shot_tasks_workspace_bytes, ()
    return lib.tclip_bdcspn_visual_tasks_workspace_bytes, lib.tclip_laplacian_shot_visual_tasks_workspace_bytes, (dim,)


@pytest.mark.parametrize("dim", [None, 512])
def test_argument_errors_come_before_any_launch(dim):
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    no_support = _capi.Problem(1, 2, 75, 10, 0, 3, 1, 0, 0)
    bd_query, ls_query, lead = _queries(dim)
    for call, n_ptr in ((_bdcspn, 4), (_lshot, 5)):
        assert call(no_support, dim) == ERR_ARG and b"n_support" in lib.tclip_last_error()
        for null in range(n_ptr):
            assert call(p, dim, null=null) == ERR_ARG
        for field in ("table_q", "q_idx", "table_s", "s_idx"):
            src = _source()
            setattr(src, field, None)
            assert call(p, dim, src=src) == ERR_ARG
        assert call(_capi.Problem(1, 2, 75, 1025, 20, 3, 1, 0, 0), dim) == ERR_ARG
        assert call(_capi.Problem(1, 2, 75, 1, 20, 3, 1, 0, 0), dim) == ERR_ARG
        assert call(p, dim, ws=0) == ERR_ARG                       # a null workspace is a null pointer
    for norm_type in (-1, 3):
        assert _bdcspn(p, dim, norm_type=norm_type) == ERR_ARG and b"norm_type" in lib.tclip_last_error()
    for norm_type in (-1, 2):                                       # CL2N is not LaplacianShot's
        assert _lshot(p, dim, norm_type=norm_type) == ERR_ARG and b"norm_type" in lib.tclip_last_error()
    for knn in (1, 76):
        assert _lshot(p, dim, knn=knn) == ERR_ARG and b"knn" in lib.tclip_last_error()
    assert _lshot(_capi.Problem(1, 2, 75, 10, 20, 0, 1, 0, 0), dim) == ERR_ARG and b"iters" in lib.tclip_last_error()
    # the workspace queries refuse what the entries refuse
    for query in (bd_query, ls_query):
        assert query(ctypes.byref(no_support), *lead) == 0
        assert query(ctypes.byref(_capi.Problem(1, 2, 75, 1025, 20, 3, 1, 0, 0)), *lead) == 0
        assert query(None, *lead) == 0
    # workspace: short, then misaligned
    for call, query in ((_bdcspn, bd_query), (_lshot, ls_query)):
        need = query(ctypes.byref(p), *lead)
        assert need > 0
        assert call(p, dim, ws_bytes=need - 1) == ERR_WORKSPACE and query.__name__.encode() in lib.tclip_last_error()
        assert call(p, dim, ws=0x100010, ws_bytes=need) == ERR_WORKSPACE and b"aligned" in lib.tclip_last_error()


def test_visual_entries_check_dim_and_take_no_cols():
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    for dim in (0, 1025):
        for call, query in ((_bdcspn, lib.tclip_bdcspn_visual_tasks_workspace_bytes),
                            (_lshot, lib.tclip_laplacian_shot_visual_tasks_workspace_bytes)):
            assert call(p, dim) == ERR_ARG and b"dim" in lib.tclip_last_error()
            assert query(ctypes.byref(p), dim) == 0
    for call in (_bdcspn, _lshot):
        assert call(p, 512, src=_source(cols=0x5000)) == ERR_ARG and b"cols" in lib.tclip_last_error()
    # cols belong to the probability-feature entries: accepted there (the next refusal is the workspace's)
    assert _bdcspn(p, src=_source(cols=0x5000), ws_bytes=1) == ERR_WORKSPACE
    assert _lshot(p, src=_source(cols=0x5000), ws_bytes=1) == ERR_WORKSPACE


def _align(n):
    return (n + 255) // 256 * 256


# (T, Q, K, S, D or None): S*D below, equal to and above (S+Q)*K; the issue's K = D = 1000 / S = 4000 case; D = 257, K = 4
SHAPES = [(3, 75, 10, 20, None), (100, 75, 1000, 4000, None), (2, 10, 5, 1, None), (3, 75, 37, 65, 8), (3, 10, 4, 17, 257),
          (3, 75, 4, 130, 257), (1, 75, 1000, 4000, 1024), (2, 75, 10, 75, 20), (2, 75, 10, 74, 20), (2, 75, 10, 76, 20)]


@pytest.mark.parametrize("T,Q,K,S,D", SHAPES)
def test_workspace_arithmetic(T, Q, K, S, D):
    lib = _capi.lib()
    p = ctypes.byref(_capi.Problem(1, T, Q, K, S, 5, 1, 0, 0))
    if D is None:
        dense, tasks = lib.tclip_bdcspn_workspace_bytes(p), lib.tclip_bdcspn_tasks_workspace_bytes(p)
        ls_dense, ls_tasks = lib.tclip_laplacian_shot_workspace_bytes(p), lib.tclip_laplacian_shot_tasks_workspace_bytes(p)
        D = K
    else:
        dense, tasks = lib.tclip_bdcspn_visual_workspace_bytes(p, D), lib.tclip_bdcspn_visual_tasks_workspace_bytes(p, D)
        ls_dense, ls_tasks = (lib.tclip_laplacian_shot_visual_workspace_bytes(p, D),
                              lib.tclip_laplacian_shot_visual_tasks_workspace_bytes(p, D))
    assert dense > 0 and ls_dense > 0
    # one region for zs and the logits, the larger of the two: the dense workspace minus the smaller
    if S * D <= (S + Q) * K:
        assert tasks == dense - _align(T * S * D * 4)
    else:
        assert tasks == dense - _align(T * (S + Q) * K * 4)
    assert ls_tasks == ls_dense


def test_workspace_per_task_at_imagenet_scale():
    """K = D = 1000, 4 shots, Q = 75: 57 MB of dense workspace per task plus 16 MB of x_s become 41 MB"""
    lib = _capi.lib()
    p = ctypes.byref(_capi.Problem(1, 1, 75, 1000, 4000, 1, 1, 0, 0))
    dense, tasks = lib.tclip_bdcspn_workspace_bytes(p), lib.tclip_bdcspn_tasks_workspace_bytes(p)
    assert 57.0e6 < dense < 57.5e6 and 41.0e6 < tasks < 41.5e6 and dense - tasks == 16_000_000


def test_opt_in_switch_of_the_classes():
    from src.methods._em_dirichlet_base import FewShotMixin
    from src.methods.few_shot.bdcspn import BDCSPN
    from src.methods.few_shot.em_dirichlet import EM_DIRICHLET
    from src.methods.few_shot.laplacian_shot import LAPLACIAN_SHOT
    from src.methods.few_shot.paddle import PADDLE
    from src.methods.few_shot.tim import ALPHA_TIM, TIM_GD
    assert FewShotMixin.IN_PLACE_SUPPORT == () and BDCSPN.IN_PLACE_SUPPORT == ("softmax", "visual")
    assert LAPLACIAN_SHOT.IN_PLACE_SUPPORT == ("softmax",)
    assert (BDCSPN.can_read_rows_in_place(True), BDCSPN.can_read_rows_in_place(False)) == (True, True)
    assert (LAPLACIAN_SHOT.can_read_rows_in_place(True), LAPLACIAN_SHOT.can_read_rows_in_place(False)) == (True, False)
    for cls in (EM_DIRICHLET, PADDLE, ALPHA_TIM, TIM_GD):
        assert cls.IN_PLACE_SUPPORT == ()
        assert (cls.can_read_rows_in_place(True), cls.can_read_rows_in_place(False)) == (False, False)
    # the default route's question is answered as before
    for cls in (BDCSPN, LAPLACIAN_SHOT):
        assert cls.IN_PLACE_FEATURES == ()
        assert (cls.reads_rows_in_place(True), cls.reads_rows_in_place(False)) == (False, False)
        assert cls.run_tables is not FewShotMixin.run_tables
    assert PADDLE.reads_rows_in_place(True) and PADDLE.reads_rows_in_place(False)


def test_laplacian_shot_run_tables_refuses_visual_features():
    import torch
    from src.methods.few_shot.laplacian_shot import LAPLACIAN_SHOT
    from src.utils import CfgNode
    a = CfgNode(iter=3, num_classes_test=10, n_class=10, n_query=75, k_eff=5, T=30, shots=2, use_softmax_feature=False, knn=3, lmd=0.7,
                norm_type="L2N", temp=30, batch_size=2)
    m = LAPLACIAN_SHOT(model=None, device=torch.device("cpu"), log_file=None, args=a)
    tab = torch.zeros(8, 64)
    idx = torch.zeros(2, 20, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="probability features"):
        m.run_tables(table_s=tab, s_idx=idx, table_q=tab, q_idx=idx, cols=None, y_s=idx, y_q=idx)


def test_main_features_takes_the_option():
    import main_features
    _, cfg = main_features.parse_args(["--opts", "method", "bdcspn", "shots", "4", "in_place_support", "True"])
    assert cfg.in_place_support is True and cfg.name_method == "BDCSPN"
    _, cfg = main_features.parse_args(["--opts", "method", "bdcspn", "shots", "4"])
    assert getattr(cfg, "in_place_support", False) is False
    assert "in_place_support" not in main_features.MAIN_DEFAULTS
    assert "in_place_support" in main_features.__doc__
