"""CPU: the scoring entries (tclip_em_dirichlet_score, tclip_em_dirichlet_score_tasks) exist, size their workspace without
rows_per_task, refuse bad arguments by name before anything touches a GPU, and tclip_amd.score / the classes' score_rows check
what they are given as the run entries do.  The numbers are judged on the GPU (tests/test_gpu_score.py)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from tclip_amd import _capi

NAMES = ("tclip_em_dirichlet_score_workspace_bytes", "tclip_em_dirichlet_score", "tclip_em_dirichlet_score_tasks")
ERR_ARG = 1
FAKE = ctypes.c_void_p(256)          # a non-null, 256-byte aligned "pointer": nothing is launched before the checks are through


def _problem(T=2, R=7, K=10, lambd=150, Q=75, hard=0):
    return _capi.ScoreProblem(T, R, K, lambd, Q, hard)


def test_entries_resolve_and_are_declared_as_additions():
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    later = header[header.index("later, without a new number"):header.index("#define TCLIP_ABI_VERSION")]
    lib = _capi.lib()
    for name in NAMES:
        assert name + "(" in header and name in later and name in _capi.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert "typedef struct tclip_score_problem" in header
    assert re.search(r"#define TCLIP_ABI_VERSION 5\b", header) and lib.tclip_abi_version() == 5


def test_workspace_query_rejects_bad_input_and_ignores_rows_per_task():
    lib = _capi.lib()
    q = lib.tclip_em_dirichlet_score_workspace_bytes
    assert q(None) == 0
    for bad in (_problem(T=0), _problem(R=0), _problem(K=1), _problem(K=1025), _problem(Q=0)):
        assert q(ctypes.byref(bad)) == 0
    for K in (10, 1000):
        small, large = q(ctypes.byref(_problem(T=3, R=1, K=K))), q(ctypes.byref(_problem(T=3, R=100000, K=K)))
        assert small == large and small >= 3 * K * 4 and small % 256 == 0
        assert small <= 3 * K * 4 + 256                     # the row constants and nothing else: O(T K)
    # the per-task part scales with T
    assert q(ctypes.byref(_problem(T=125, R=75, K=1000))) == 125 * 1000 * 4 + (-125 * 1000 * 4) % 256


BAD = [("x", dict(), "x"), ("alpha", dict(), "alpha"), ("preds", dict(), "preds"), ("n_class", dict(K=1), None),
       ("n_class", dict(K=1025), None), ("rows_per_task", dict(R=0), None), ("n_task", dict(T=0), None), ("n_query", dict(Q=0), None)]


@pytest.mark.parametrize("word,fields,null", BAD, ids=[f"{w}-{f or 'null'}" for w, f, _ in BAD])
def test_dense_entry_names_the_bad_argument(word, fields, null):
    lib = _capi.lib()
    p = _problem(**fields)
    ptrs = dict(x=FAKE, alpha=FAKE, v=FAKE, u=FAKE, preds=FAKE, logits=FAKE)
    if null:
        ptrs[null] = None
    rc = lib.tclip_em_dirichlet_score(ctypes.byref(p), ptrs["x"], ptrs["alpha"], ptrs["v"], ptrs["u"], ptrs["preds"], ptrs["logits"],
                                      FAKE, 1 << 30, None)
    assert rc == ERR_ARG
    assert re.search(r"\b%s\b" % word, lib.tclip_last_error().decode()), lib.tclip_last_error()


BAD_TASKS = [("table", "table"), ("idx", "idx"), ("alpha", "alpha"), ("preds", "preds")]


@pytest.mark.parametrize("word,null", BAD_TASKS)
def test_table_entry_names_the_bad_argument(word, null):
    lib = _capi.lib()
    ptrs = dict(table=FAKE, idx=FAKE, cols=None, alpha=FAKE, v=None, u=None, preds=FAKE, logits=None)
    ptrs[null] = None
    p = _problem()
    rc = lib.tclip_em_dirichlet_score_tasks(ctypes.byref(p), ptrs["table"], ptrs["idx"], ptrs["cols"], ptrs["alpha"], ptrs["v"],
                                            ptrs["u"], ptrs["preds"], ptrs["logits"], FAKE, 1 << 30, None)
    assert rc == ERR_ARG
    assert re.search(r"\b%s\b" % word, lib.tclip_last_error().decode())
    for fields, word2 in ((dict(K=1), "n_class"), (dict(K=1025), "n_class"), (dict(R=0), "rows_per_task"), (dict(T=0), "n_task"),
                          (dict(Q=0), "n_query")):
        p = _problem(**fields)
        assert lib.tclip_em_dirichlet_score_tasks(ctypes.byref(p), FAKE, FAKE, None, FAKE, None, None, FAKE, None, FAKE, 1 << 30,
                                                  None) == ERR_ARG
        assert word2 in lib.tclip_last_error().decode()


def test_workspace_is_checked_after_the_arguments():
    lib = _capi.lib()
    p = _problem()
    need = lib.tclip_em_dirichlet_score_workspace_bytes(ctypes.byref(p))
    args = (ctypes.byref(p), FAKE, FAKE, None, None, FAKE, None)
    assert lib.tclip_em_dirichlet_score(*args, FAKE, need - 1, None) == 2                       # TCLIP_ERR_WORKSPACE
    assert lib.tclip_em_dirichlet_score(*args, ctypes.c_void_p(264), need, None) == 2           # misaligned
    assert lib.tclip_em_dirichlet_score(*args, None, need, None) == ERR_ARG and b"workspace" in lib.tclip_last_error()


def test_python_entries_check_shapes_dtypes_and_devices():
    from tclip_amd import score
    T, R, K = 2, 5, 6
    x, alpha, v = torch.rand(T, R, K), torch.rand(T, K, K) + 0.5, torch.rand(T, K)
    kw = dict(lambd=75, n_query=75)
    with pytest.raises(ValueError, match=r"alpha must be \(T,K,K\)"):
        score.score_em_dirichlet(x, alpha[:1], v, **kw)
    with pytest.raises(ValueError, match=r"alpha must be \(T,K,K\)"):
        score.score_em_dirichlet(x, torch.rand(T, K, K + 1), v, **kw)
    with pytest.raises(ValueError, match=r"v must be \(T,K\)"):
        score.score_em_dirichlet(x, alpha, v[:, :-1], **kw)
    with pytest.raises(ValueError, match="only with one model"):
        score.score_em_dirichlet(x[0], alpha, v, **kw)                 # a 2-D x with T = 2 models
    with pytest.raises(ValueError, match=r"x must be \(T,R,K\)"):
        score.score_em_dirichlet(x[None], alpha, v, **kw)
    with pytest.raises(ValueError, match=r"n_class must be in 2\.\.1024"):
        score.score_em_dirichlet(torch.rand(1, 3, 1), torch.rand(1, 1, 1), None, **kw)
    with pytest.raises(TypeError, match="x must be a floating-point tensor"):
        score.score_em_dirichlet(x.long(), alpha, v, **kw)
    with pytest.raises(TypeError, match="alpha must be a floating-point tensor"):
        score.score_em_dirichlet(x, alpha.long(), v, **kw)
    # host tensors: the run entries' message
    for args in ((x, alpha, v), (x[0], alpha[:1], v[:1])):
        with pytest.raises(RuntimeError, match="x must live on the GPU: the EM-Dirichlet engine has no CPU path"):
            score.score_em_dirichlet(*args, **kw)
    table, idx = torch.rand(20, K), torch.randint(0, 20, (T, R))
    with pytest.raises(RuntimeError, match="table must live on the GPU"):
        score.score_em_dirichlet_tasks(table, idx, alpha, v, **kw)
    with pytest.raises(ValueError, match=r"table must be \(n,K\) and idx \(T,R\)"):
        score.score_em_dirichlet_tasks(table, idx[0], alpha, v, **kw)
    with pytest.raises(TypeError, match="idx and cols must be integer tensors"):
        score.score_em_dirichlet_tasks(table, idx.float(), alpha, v, **kw)
    with pytest.raises(ValueError, match=r"alpha must be \(T,K,K\)"):
        score.score_em_dirichlet_tasks(table, idx[:1], alpha, v, **kw)


def test_score_rows_needs_a_run_and_probability_features():
    from src.methods.few_shot.em_dirichlet import EM_DIRICHLET as FS
    from src.methods.few_shot.hard_em_dirichlet import HARD_EM_DIRICHLET as FSH
    from src.methods.zero_shot.em_dirichlet import EM_DIRICHLET as ZS
    from src.methods.zero_shot.hard_em_dirichlet import HARD_EM_DIRICHLET as ZSH
    from src.methods._em_dirichlet_base import _SIMPLEX_ERROR
    from src.utils import CfgNode
    K = 10
    for cls in (ZS, ZSH, FS, FSH):
        args = CfgNode(iter=2, iter_mm=60, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, use_softmax_feature=True,
                       graph_matching=True)
        m = cls(model=None, device="cuda:0", log_file=None, args=args)
        x = torch.rand(2, 4, K)
        with pytest.raises(RuntimeError, match="no fitted model"):
            m.score_rows(x)
        with pytest.raises(RuntimeError, match="no fitted model"):
            m.score_table_rows(torch.rand(9, K), torch.zeros(2, 4, dtype=torch.long))
        args.use_softmax_feature = False
        with pytest.raises(ValueError, match=re.escape(_SIMPLEX_ERROR)):
            m.score_rows(x)
        assert not hasattr(m, "alpha") or m.alpha is None
