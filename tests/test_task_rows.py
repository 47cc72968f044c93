"""CPU: the fused task builder (tclip_gather_task_rows) and PADDLE fed from the feature tables (tclip_paddle_run_tasks,
tclip_paddle_visual_run_tasks): the names are declared, bound and exported, bad arguments are refused before any launch, the
workspace does not depend on n_support, and the host equivalence the device path relies on holds -
`table[idx][..., cols]` with relabel_indices' outputs is what relabel_batch makes of the gathered tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from tclip_amd import _capi

NEW = ("tclip_gather_task_rows", "tclip_paddle_tasks_workspace_bytes", "tclip_paddle_run_tasks",
       "tclip_paddle_visual_tasks_workspace_bytes", "tclip_paddle_visual_run_tasks")
ERR_ARG, ERR_WORKSPACE = 1, 2


def test_names_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NEW + ("tclip_check_task_indices",):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/tclip.h"
        assert name in _capi.EXPORTS
        assert re.search(r" T %s$" % name, exported, flags=re.M), f"{name} is not exported by libtclip.so"
    assert re.search(r"#define\s+TCLIP_ABI_VERSION\s+5\b", header)
    assert _capi.lib().tclip_abi_version() == 5
    version_comment = header[:header.index("#define TCLIP_ABI_VERSION")]
    for name in NEW:
        assert name in version_comment, f"{name} is missing from the header's version comment"


# fake non-null addresses: every call below must return before anything reads them
A, B, C, D_ = (ctypes.c_void_p(0x1000 * i) for i in range(1, 5))


def test_gather_task_rows_argument_errors():
    lib = _capi.lib()

    def call(table=A, n_rows=10, width=8, idx=B, rows_per_task=2, cols=None, n_out=4, out=C):
        return lib.tclip_gather_task_rows(table, n_rows, width, idx, rows_per_task, cols, n_out, out, None)
    assert call(table=None) == ERR_ARG
    assert call(idx=None) == ERR_ARG
    assert call(out=None) == ERR_ARG
    assert call(width=0) == ERR_ARG
    assert call(rows_per_task=0) == ERR_ARG
    assert call(cols=D_, rows_per_task=3, n_out=4) == ERR_ARG and b"multiple" in lib.tclip_last_error()
    assert call(n_out=0) == 0                      # nothing to do and nothing launched


def _source(cols=None):
    return _capi.TaskSource(0x1000, 0x2000, 0x3000, 0x4000, cols)


def _paddle(p, ws=0x100000, ws_bytes=1 << 40, src=None, null=None):
    ptr = [ctypes.c_void_p(0x10000 * i) for i in range(1, 6)]      # y_s, u, v, w, preds
    if null is not None:
        ptr[null] = None
    return _capi.lib().tclip_paddle_run_tasks(ctypes.byref(p), ctypes.byref(src or _source()), ptr[0], ctypes.c_float(1.0), *ptr[1:],
                                              ctypes.c_void_p(ws), ws_bytes, None)


def _paddle_visual(p, dim, ws=0x100000, ws_bytes=1 << 40, src=None, null=None):
    ptr = [ctypes.c_void_p(0x10000 * i) for i in range(1, 6)]
    if null is not None:
        ptr[null] = None
    return _capi.lib().tclip_paddle_visual_run_tasks(ctypes.byref(p), dim, ctypes.byref(src or _source()), ptr[0], ctypes.c_float(1.0),
                                                     *ptr[1:], ctypes.c_void_p(ws), ws_bytes, None)


def test_paddle_tasks_argument_errors():
    lib = _capi.lib()
    p = _capi.Problem(1, 2, 75, 10, 20, 3, 1, 0, 0)
    no_support = _capi.Problem(1, 2, 75, 10, 0, 3, 1, 0, 0)
    for dim in (0, 1025):
        assert _paddle_visual(p, dim) == ERR_ARG and b"dim" in lib.tclip_last_error()
        assert lib.tclip_paddle_visual_tasks_workspace_bytes(ctypes.byref(p), dim) == 0
    assert _paddle_visual(no_support, 512) == ERR_ARG and b"n_support" in lib.tclip_last_error()
    assert _paddle(no_support) == ERR_ARG and b"n_support" in lib.tclip_last_error()
    assert _paddle_visual(p, 512, src=_source(cols=0x5000)) == ERR_ARG and b"cols" in lib.tclip_last_error()
    for null in range(5):
        assert _paddle(p, null=null) == ERR_ARG
        assert _paddle_visual(p, 512, null=null) == ERR_ARG
    for field in ("table_q", "q_idx", "table_s", "s_idx"):
        src = _source()
        setattr(src, field, None)
        assert _paddle(p, src=src) == ERR_ARG
        assert _paddle_visual(p, 512, src=src) == ERR_ARG
    assert _paddle(_capi.Problem(1, 2, 75, 1025, 20, 3, 1, 0, 0)) == ERR_ARG
    assert _paddle(_capi.Problem(1, 2, 75, 1, 20, 3, 1, 0, 0)) == ERR_ARG
    # workspace: short, then misaligned
    need = lib.tclip_paddle_tasks_workspace_bytes(ctypes.byref(p))
    need_v = lib.tclip_paddle_visual_tasks_workspace_bytes(ctypes.byref(p), 512)
    assert need > 0 and need_v > 0
    assert _paddle(p, ws_bytes=need - 1) == ERR_WORKSPACE and b"tclip_paddle_tasks_workspace_bytes" in lib.tclip_last_error()
    assert _paddle_visual(p, 512, ws_bytes=need_v - 1) == ERR_WORKSPACE
    assert b"tclip_paddle_visual_tasks_workspace_bytes" in lib.tclip_last_error()
    assert _paddle(p, ws=0x100010, ws_bytes=need) == ERR_WORKSPACE and b"aligned" in lib.tclip_last_error()
    assert _paddle_visual(p, 512, ws=0x100080, ws_bytes=need_v) == ERR_WORKSPACE and b"aligned" in lib.tclip_last_error()
    # a null workspace is a null pointer
    assert _paddle(p, ws=0) == ERR_ARG


def test_workspace_does_not_depend_on_n_support():
    lib = _capi.lib()
    K, D, T, Q = 1000, 1024, 8, 75

    def problem(S, K=K):
        return _capi.Problem(1, T, Q, K, S, 20, 1, 0, 0)
    few = lib.tclip_paddle_visual_tasks_workspace_bytes(ctypes.byref(problem(4)), D)
    many = lib.tclip_paddle_visual_tasks_workspace_bytes(ctypes.byref(problem(4000)), D)
    dense = lib.tclip_paddle_visual_workspace_bytes(ctypes.byref(problem(4)), D)
    assert few == many and few >= dense > 0
    assert few >= dense + T * Q * D * 4                         # the gathered queries
    assert few < dense + T * Q * D * 4 + 4096                   # and nothing else
    assert lib.tclip_paddle_visual_tasks_workspace_bytes(ctypes.byref(problem(0)), D) == 0
    assert lib.tclip_paddle_visual_tasks_workspace_bytes(ctypes.byref(problem(4, K=1025)), D) == 0
    assert lib.tclip_paddle_visual_tasks_workspace_bytes(None, D) == 0
    few = lib.tclip_paddle_tasks_workspace_bytes(ctypes.byref(problem(4)))
    many = lib.tclip_paddle_tasks_workspace_bytes(ctypes.byref(problem(4000)))
    dense = lib.tclip_paddle_workspace_bytes(ctypes.byref(problem(4)))
    assert few == many and few >= dense + T * Q * K * 4 and few < dense + T * Q * K * 4 + 4096
    assert lib.tclip_paddle_tasks_workspace_bytes(ctypes.byref(problem(0))) == 0
    assert lib.tclip_paddle_tasks_workspace_bytes(ctypes.byref(problem(4, K=1))) == 0
    assert lib.tclip_paddle_tasks_workspace_bytes(None) == 0


@pytest.mark.parametrize("K,shots,N", [(5, 1, 3), (10, 4, 4), (37, 2, 2)])
def test_index_route_equals_relabel_batch(K, shots, N):
    """what the device path computes, stated on the host: table[idx][..., cols] and the labels of relabel_indices equal
    relabel_batch on the gathered tensors (random labels, every class in every support set)."""
    from src.eval_few_shot import relabel_batch, relabel_indices
    gen = torch.Generator().manual_seed(K * 100 + shots)
    S, Q, rows = K * shots, 75, 8 * K
    table_s, table_q = torch.randn(rows, K, generator=gen), torch.randn(rows, K, generator=gen)
    s_idx, q_idx = torch.randint(0, rows, (N, S), generator=gen), torch.randint(0, rows, (N, Q), generator=gen)
    y_s = torch.stack([torch.arange(K).repeat_interleave(shots)[torch.randperm(S, generator=gen)] for _ in range(N)])
    y_q = torch.randint(0, K, (N, Q), generator=gen)
    rel = relabel_indices(y_s, y_q, K)
    assert rel is not None
    cols, ys2, yq2 = rel
    assert cols.dtype == torch.int32 and tuple(cols.shape) == (N, K)
    x_s, x_q = table_s[s_idx], table_q[q_idx]
    want = relabel_batch(x_s, x_q, y_s, y_q, True)
    take = cols.long().unsqueeze(1)
    got_s = torch.gather(x_s, 2, take.expand(N, S, K))
    got_q = torch.gather(x_q, 2, take.expand(N, Q, K))
    assert torch.equal(got_s.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got_q.view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(ys2, want[2]) and torch.equal(yq2, want[3])
    assert torch.equal(cols, torch.arange(K - 1, -1, -1, dtype=torch.int32).repeat(N, 1))
    # visual features: nothing is permuted and the labels stay
    vis = relabel_batch(x_s, x_q, y_s, y_q, False)
    assert torch.equal(vis[0], x_s) and torch.equal(vis[1], x_q) and torch.equal(vis[2], y_s) and torch.equal(vis[3], y_q)


def test_relabel_indices_is_none_when_a_class_is_missing():
    from src.eval_few_shot import relabel_indices
    K = 6
    y_s = torch.arange(K).repeat(2, 2)
    y_q = torch.zeros(2, 75, dtype=torch.long)
    assert relabel_indices(y_s, y_q, K) is not None
    y_s[1][y_s[1] == 3] = 2
    assert relabel_indices(y_s, y_q, K) is None
