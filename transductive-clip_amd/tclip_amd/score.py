"""Scoring with a fitted EM-Dirichlet model (tclip_em_dirichlet_score, tclip_em_dirichlet_score_tasks): one E-step of a given
alpha (T,K,K), v (T,K) on rows that need not have been queries of the fit - "fit on a sample, label the rest of the table".

    logits[t,r,k] = get_logits: the Dirichlet log density of row r under class k of task t       (em_dirichlet.py:35-39)
    u             = softmax_k(logits + (lambd * v) / n_query)        (v=None: softmax_k(logits));  one-hot of preds if hard
    preds         = first maximum of u, a NaN counting as the maximum

with the operations of the loop's own E-step: scoring a run's x_q with its alpha, v, lambd and n_query returns that run's u and
preds bit for bit, and a row's bits depend on (row, alpha[t], v[t], lambd, n_query, K) only - not on how many rows or tasks share
the call, on the row's position, on the dense or table route or on which outputs were asked for.  No (T,R,K,K) tensor, no
(T,R,K) scratch: the workspace is the per-class row constants, T * K floats.  In zero-shot the classes are clusters; matching
clusters to classes stays with the accuracy tail (engine.clustering_accuracy).

engine.py's public surface is pinned, so the functions live here; they share engine's checks and helpers."""
import torch

from . import _capi, engine


class ScoreResult:
    """u (T,R,K) f32 or None, preds (T,R) i32, logits (T,R,K) f32 or None: cuda tensors"""
    __slots__ = ("u", "preds", "logits")

    def __init__(self, **kw):
        for k, val in kw.items():
            setattr(self, k, val)


def _check_float(t, name):
    if not t.is_floating_point():
        raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")


def _check_model(alpha, v, T, K):
    """shapes and dtypes of the model against the rows' T and K, before anything is asked of a device"""
    _check_float(alpha, "alpha")
    if alpha.dim() != 3 or tuple(alpha.shape) != (T, K, K):
        raise ValueError("alpha must be (T,K,K) with the T and K of the scored rows")
    if v is not None:
        _check_float(v, "v")
        if tuple(v.shape) != (T, K):
            raise ValueError("v must be (T,K) with the T and K of alpha")
    if T < 1:
        raise ValueError("there must be at least one task and one row per task")
    engine._check_n_class(K)


def _model(alpha, v, dev):
    """alpha and v (or None) as contiguous f32 tensors on the rows' device"""
    engine._require_cuda(alpha, "alpha")
    if v is not None:
        engine._require_cuda(v, "v")
    if alpha.device != dev or (v is not None and v.device != dev):
        raise ValueError("alpha and v must live on the device of the scored rows")
    return alpha.contiguous().float(), (v.contiguous().float() if v is not None else None)


def _score(entry, rows_args, dev, T, R, K, alpha, v, lambd, n_query, hard, want_u, want_logits):
    if int(n_query) < 1:
        raise ValueError("n_query must be the fit's query count, >= 1")
    if R < 1:
        raise ValueError("there must be at least one task and one row per task")
    p = _capi.ScoreProblem(T, R, K, int(lambd), int(n_query), int(bool(hard)))
    c = engine._Call(dev, p, "tclip_em_dirichlet_score_workspace_bytes")
    u = c.empty(T, R, K) if want_u else None
    logits = c.empty(T, R, K) if want_logits else None
    preds = c.empty(T, R, dtype=torch.int32)
    ptr = engine._ptr
    c.launch(entry, lambda ws, n, st: (*rows_args, ptr(alpha), ptr(v), ptr(u), ptr(preds), ptr(logits), ws, n, st))
    return ScoreResult(u=u, preds=preds, logits=logits)


def score_em_dirichlet(x, alpha, v=None, *, lambd, n_query, hard=False, want_u=True, want_logits=False):
    """x (T,R,K) f32 cuda rows on the simplex - or (R,K) when alpha holds ONE model (T = 1) -, alpha (T,K,K), v (T,K) or None:
    the model of a fit, with that fit's integer lambd and its n_query (75 in every reference config), NOT the number of rows
    scored.  want_u=False returns labels only (u is 4 R K bytes per task).

    Returns ScoreResult of cuda tensors shaped like x; nothing is synchronised."""
    _check_float(x, "x")
    flat = x.dim() == 2
    if flat:
        if alpha.dim() != 3 or alpha.shape[0] != 1:
            raise ValueError("a 2-D x (R,K) is accepted only with one model: alpha must be (1,K,K)")
        x = x.unsqueeze(0)
    if x.dim() != 3:
        raise ValueError("x must be (T,R,K), or (R,K) with one model")
    T, R, K = x.shape
    _check_model(alpha, v, T, K)
    x = engine._query(x, "x")
    alpha, v = _model(alpha, v, x.device)
    res = _score("tclip_em_dirichlet_score", (engine._ptr(x),), x.device, T, R, K, alpha, v, lambd, n_query, hard, want_u, want_logits)
    if flat:
        res = ScoreResult(u=None if res.u is None else res.u[0], preds=res.preds[0],
                          logits=None if res.logits is None else res.logits[0])
    return res


def score_em_dirichlet_tasks(table, idx, alpha, v=None, cols=None, *, lambd, n_query, hard=False, want_u=True, want_logits=False):
    """The same with the rows read in place from a feature table (tclip_em_dirichlet_score_tasks): table (rows,K) f32 cuda,
    idx (T,R) int64 rows of it, cols (T,K) the per-task column permutation of Tasks_Generator_few_shot.get_task or None; row r
    of task t is table[idx[t,r]][cols[t]].  No (T,R,K) tensor is built; the results are those of score_em_dirichlet on
    engine.gather_task_rows(table, idx, cols), bit for bit.  An index or column outside its range raises IndexError before
    anything is launched.

    Returns ScoreResult of cuda tensors; nothing is synchronised after the index checks."""
    _check_float(table, "table")
    if table.dim() != 2 or idx.dim() != 2:
        raise ValueError("table must be (n,K) and idx (T,R)")
    if idx.is_floating_point() or (cols is not None and cols.is_floating_point()):
        raise TypeError("idx and cols must be integer tensors")
    T, R = idx.shape
    K = table.shape[1]
    _check_model(alpha, v, T, K)
    engine._require_cuda(table, "table")
    table = table.contiguous().float()
    dev = table.device
    idx = engine._index_tensor(idx, table.shape[0], dev, "idx")
    if cols is not None:
        cols = engine._cols_tensor(cols, T, K, dev)
    alpha, v = _model(alpha, v, dev)
    args = (engine._ptr(table), engine._ptr(idx), engine._ptr(cols))
    return _score("tclip_em_dirichlet_score_tasks", args, dev, T, R, K, alpha, v, lambd, n_query, hard, want_u, want_logits)
