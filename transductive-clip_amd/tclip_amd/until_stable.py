"""EM-Dirichlet with a per-batch stop once the argmax assignment stands still (opt-in; tclip_em_dirichlet_run_until_stable).

The reference runs a fixed number of outer iterations and never acts on its criterion; what an evaluation reads is the argmax
assignment, and on many batches that stops moving long before the last iteration.  `patience = p`: a batch stops after the
first outer iteration that ends p consecutive iterations without a change of any of its predictions.  The stop is exact: a
batch that stops after s iterations returns, bit for bit, what engine.run_em_dirichlet returns for that batch alone with
iters = s.  The decision is taken on the device; nothing is synchronised.

engine.py's public surface is pinned, so the two functions live here; they share engine's checks and helpers."""
import operator

import torch

from . import _capi, engine


class UntilStableResult:
    """EMDirichletResult plus outer_iters (n_batches,) i32: the outer iterations each batch ran, and changes (n_batches, iters)
    i32: the (task, query) pairs of the batch whose prediction changed in each of them (N * Q in the first).  criterions,
    mm_iters and changes of a batch are 0 from its outer_iters on."""
    __slots__ = ("u", "v", "alpha", "preds", "criterions", "mm_iters", "outer_iters", "changes")

    def __init__(self, **kw):
        for k, val in kw.items():
            setattr(self, k, val)


def check_patience(patience):
    """patience as an int; ValueError unless it is an integer >= 1 (a bool is not an integer here)"""
    try:
        if isinstance(patience, bool):
            raise TypeError
        p = operator.index(patience)
    except TypeError:
        raise ValueError(f"patience must be an integer >= 1, got {patience!r}")
    if p < 1:
        raise ValueError(f"patience must be an integer >= 1, got {patience!r}")
    return p


def _until_stable(rows, K, patience, n_batches, iters, iter_mm, lambd, hard):
    """engine._em_dirichlet with the until-stable entries: the same Problem and outputs, patience after y_s, outer_iters and
    changes after mm_iters"""
    T, Q, dev = rows.T, rows.Q, rows.dev
    c = engine._Call(dev, _capi.Problem(n_batches, T // n_batches, Q, K, rows.S, iters, iter_mm, int(lambd), int(bool(hard))),
                     "tclip_em_dirichlet_until_stable_workspace_bytes")
    u, v, alpha, preds = c.empty(T, Q, K), c.empty(T, K), c.empty(T, K, K), c.empty(T, Q, dtype=torch.int32)
    per_iter = lambda dtype: torch.zeros(n_batches, max(iters, 1), dtype=dtype, device=dev)[:, :iters].contiguous()      # noqa: E731
    crit, mm, changes = per_iter(torch.float32), per_iter(torch.int32), per_iter(torch.int32)
    outer = torch.zeros(n_batches, dtype=torch.int32, device=dev)
    ptr = engine._ptr
    c.launch("tclip_em_dirichlet" + rows.run + "_until_stable",
             lambda ws, n, st: (*rows.args, ptr(rows.y_s), patience, ptr(u), ptr(v), ptr(alpha), ptr(preds), ptr(crit), ptr(mm),
                                ptr(outer), ptr(changes), ws, n, st))
    return UntilStableResult(u=u, v=v, alpha=alpha, preds=preds, criterions=crit, mm_iters=mm, outer_iters=outer, changes=changes)


def run_em_dirichlet(x_q, x_s=None, y_s=None, *, patience, n_batches=1, iters, iter_mm=1000, lambd, hard=False):
    """engine.run_em_dirichlet, each batch stopped after `patience` consecutive outer iterations without a changed prediction.
    Arguments and checks are engine.run_em_dirichlet's; a patience that is not an integer >= 1 is a ValueError.

    Returns UntilStableResult of cuda tensors; nothing is synchronised."""
    patience = check_patience(patience)
    x_q = engine._query(x_q)
    T, _, K = x_q.shape
    if T % n_batches:
        raise ValueError("number of tasks must be a multiple of n_batches")
    if x_s is not None:
        x_s, y_s = engine._support(x_q, x_s, y_s.to(x_q.device))
    return _until_stable(engine._dense_rows(x_q, x_s, y_s), K, patience, n_batches, iters, iter_mm, lambd, hard)


def run_em_dirichlet_tasks(table_q, q_idx, table_s=None, s_idx=None, y_s=None, cols=None, *, patience, n_batches=1, iters,
                           iter_mm=1000, lambd, hard=False):
    """engine.run_em_dirichlet_tasks (the task rows read in place from the feature tables), each batch stopped after `patience`
    consecutive outer iterations without a changed prediction.  Arguments and checks are engine.run_em_dirichlet_tasks's; a
    patience that is not an integer >= 1 is a ValueError.

    Returns UntilStableResult of cuda tensors; nothing is synchronised after the index checks."""
    patience = check_patience(patience)
    rows, K = engine._em_dirichlet_table_rows(table_q, q_idx, table_s, s_idx, y_s, cols, n_batches)
    return _until_stable(rows, K, patience, n_batches, iters, iter_mm, lambd, hard)
