"""EM-Dirichlet with the penalised clustering objective recorded per task and outer iteration (opt-in;
tclip_em_dirichlet_run_objective).

The reference defines `objective_function` (zero_shot/hard_em_dirichlet.py:179-198, few_shot/hard_em_dirichlet.py:149-168) and
never calls it; the engine reports only `criterions`, the relative change of alpha.  These entries add, after every E-step,
four float64 terms per task - evaluated on the device from the fp32 logits, assignments and support statistics the loop holds
anyway:

    terms[t, it] = (fit_q, fit_s, ent, part)
    fit_q = sum_n sum_k u * get_logits(query)          fit_s = sum_s get_logits(support)[s, y_s]   (0 in zero-shot)
    ent   = sum_n sum_k u * log(u + 1e-15)             part  = sum_k p_k * log(p_k + 1e-15),  p = mean_n u

and `objective(terms, lambd)` composes the reference's value, -(fit_q + fit_s) / 2 + ent - lambd * part.  The run itself is
only observed: u, v, alpha, preds, criterions, mm_iters (and outer_iters, changes) are bit for bit those of
engine.run_em_dirichlet (patience=None) or of until_stable.run_em_dirichlet (patience >= 1).  The terms of a task do not depend
on what shares the call, and the first s iterations do not depend on iters.

engine.py's public surface is pinned, so the functions live here; they share engine's checks and helpers."""
import torch

from . import _capi, engine
from .until_stable import check_patience


class ObjectiveResult:
    """UntilStableResult plus objective_terms (T, iters, 4) f64.  patience=None: outer_iters and changes are None.  With a
    patience, the terms of a batch are 0 from its outer_iters on."""
    __slots__ = ("u", "v", "alpha", "preds", "criterions", "mm_iters", "outer_iters", "changes", "objective_terms")

    def __init__(self, **kw):
        for k, val in kw.items():
            setattr(self, k, val)


def objective(terms, lambd):
    """(..., 4) terms -> (...) float64: the reference's objective_function, -(fit_q + fit_s) / 2 + ent - lambd * part, with
    the integer lambd of the run.  Takes a torch tensor or a numpy array and returns the same kind."""
    return -0.5 * (terms[..., 0] + terms[..., 1]) + terms[..., 2] - float(int(lambd)) * terms[..., 3]


def _objective(rows, K, patience, n_batches, iters, iter_mm, lambd, hard):
    """engine._em_dirichlet with the objective entries: patience after y_s (0: the plain schedule), outer_iters, changes and
    objective_terms after mm_iters"""
    T, Q, dev = rows.T, rows.Q, rows.dev
    p = 0 if patience is None else patience
    c = engine._Call(dev, _capi.Problem(n_batches, T // n_batches, Q, K, rows.S, iters, iter_mm, int(lambd), int(bool(hard))),
                     "tclip_em_dirichlet_objective_workspace_bytes", p)
    u, v, alpha, preds = c.empty(T, Q, K), c.empty(T, K), c.empty(T, K, K), c.empty(T, Q, dtype=torch.int32)
    per_iter = lambda dtype: torch.zeros(n_batches, max(iters, 1), dtype=dtype, device=dev)[:, :iters].contiguous()      # noqa: E731
    crit, mm = per_iter(torch.float32), per_iter(torch.int32)
    changes = per_iter(torch.int32) if p else None
    outer = torch.zeros(n_batches, dtype=torch.int32, device=dev) if p else None
    terms = torch.zeros(T, max(iters, 1), 4, dtype=torch.float64, device=dev)[:, :iters].contiguous()
    ptr = engine._ptr
    c.launch("tclip_em_dirichlet" + rows.run + "_objective",
             lambda ws, n, st: (*rows.args, ptr(rows.y_s), p, ptr(u), ptr(v), ptr(alpha), ptr(preds), ptr(crit), ptr(mm),
                                ptr(outer), ptr(changes), ptr(terms), ws, n, st))
    return ObjectiveResult(u=u, v=v, alpha=alpha, preds=preds, criterions=crit, mm_iters=mm, outer_iters=outer, changes=changes,
                           objective_terms=terms)


def run_em_dirichlet(x_q, x_s=None, y_s=None, *, patience=None, n_batches=1, iters, iter_mm=1000, lambd, hard=False):
    """engine.run_em_dirichlet (patience=None) or until_stable.run_em_dirichlet (patience >= 1) with the objective's terms
    recorded.  Arguments and checks are theirs; a patience that is neither None nor an integer >= 1 is a ValueError.

    Returns ObjectiveResult of cuda tensors; nothing is synchronised."""
    if patience is not None:
        patience = check_patience(patience)
    x_q = engine._query(x_q)
    T, _, K = x_q.shape
    if T % n_batches:
        raise ValueError("number of tasks must be a multiple of n_batches")
    if x_s is not None:
        x_s, y_s = engine._support(x_q, x_s, y_s.to(x_q.device))
    return _objective(engine._dense_rows(x_q, x_s, y_s), K, patience, n_batches, iters, iter_mm, lambd, hard)


def run_em_dirichlet_tasks(table_q, q_idx, table_s=None, s_idx=None, y_s=None, cols=None, *, patience=None, n_batches=1, iters,
                           iter_mm=1000, lambd, hard=False):
    """The same with the task rows read in place from the feature tables: engine.run_em_dirichlet_tasks's arguments and checks.

    Returns ObjectiveResult of cuda tensors; nothing is synchronised after the index checks."""
    if patience is not None:
        patience = check_patience(patience)
    rows, K = engine._em_dirichlet_table_rows(table_q, q_idx, table_s, s_idx, y_s, cols, n_batches)
    return _objective(rows, K, patience, n_batches, iters, iter_mm, lambd, hard)
