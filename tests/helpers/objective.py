"""The objective's terms restated on the host, their bounds, and the fixtures they are pinned on
(tests/test_objective_fixtures.py, tests/test_gpu_objective.py).

terms[..., 4] = fit_q, fit_s, ent, part; objective = -(fit_q + fit_s) / 2 + ent - lambd * part (tclip_amd.objective).
Every bound here comes from the fixture or from a float64 restatement, never from what the device returns:

  fit_q against the fixture     2^-52 (Q K + 4) A_q            u and the logits are the reference's bits: float64 reordering only
  ent, part                     2^-52 (count + 4) A + 1e-9     count = Q K / K; the floor: fp32 log(1 + 1e-15) is 0, float64's is not,
                                                               and p_k = sum_n u / Q is summed in another order
  fit_s                         2^-24 (K + max_k cnt_k + 2) S_s   S_s = sum_s (|rowc[y_s]| + sum_d |alpha[y_s,d] - 1| |log x_s[d]|):
                                                               the engine's fp32 class sums and rowc against the reference's fp32
                                                               per-row logits
  fit_q against the restatement 2^-24 (K + 4) sum_n sum_k u (|lgamma(sum_d a)| + sum_d |lgamma(a_d)| + sum_d |a_d - 1| |log z_nd|)
                                                               the engine's fp32 logits against float64 ones of the same alpha
"""
import os

import numpy as np
import torch

from conftest import GOLDEN

OBJ_DIR = os.path.join(GOLDEN, "objective")
EPS = 1e-15
FLOOR = 1e-9
# fixture -> kind, K, N, shots, iters (the issue's table)
FIXTURES = {
    "obj_zs_soft_K10_N4": ("zs_soft", 10, 4, 0, 20),
    "obj_zs_hard_K37_N6": ("zs_hard", 37, 6, 0, 10),
    "obj_fs_soft_K37_N3_s2": ("fs_soft", 37, 3, 2, 20),
    "obj_fs_hard_K10_N4_s4": ("fs_hard", 10, 4, 4, 10),
    "obj_zs_soft_K100_N2": ("zs_soft", 100, 2, 0, 5),
    "obj_fs_soft_K100_N2_s1": ("fs_soft", 100, 2, 1, 4),
    "obj_zs_soft_K2_N3": ("zs_soft", 2, 3, 0, 6),
}


def load(name):
    return np.load(os.path.join(OBJ_DIR, name + ".npz"))


def compose(terms, lambd):
    return -0.5 * (terms[..., 0] + terms[..., 1]) + terms[..., 2] - float(lambd) * terms[..., 3]


def max_count(y_s, K):
    """max_k cnt_k per task, (T,)"""
    y = np.asarray(y_s).reshape(len(y_s), -1)
    return np.stack([np.bincount(row, minlength=K).max() for row in y]).astype(np.float64)


def bounds(abs_sums, fit_s_scale, Q, K, cnt_max):
    """(..., 4) per-term bounds from the absolute sums (..., 4) of fit_q, -, ent, part and the fit_s scale (...)"""
    b = np.empty(abs_sums.shape, np.float64)
    b[..., 0] = 2.0 ** -52 * (Q * K + 4) * abs_sums[..., 0]
    b[..., 1] = 2.0 ** -24 * (K + cnt_max + 2) * fit_s_scale
    b[..., 2] = 2.0 ** -52 * (Q * K + 4) * abs_sums[..., 2] + FLOOR
    b[..., 3] = 2.0 ** -52 * (K + 4) * abs_sums[..., 3] + FLOOR
    return b


def fixture_bounds(g):
    """(iters, N, 4): the test-1 bounds of a fixture"""
    K, Q = int(g["K"]), g["x_q"].shape[1]
    cnt = max_count(g["y_s"], K) if "y_s" in g.files else np.zeros(int(g["N"]))
    return bounds(g["abs_sums"], g["fit_s_scale"], Q, K, cnt[None, :])


def restate(x_q, x_s, y_s, alpha, u):
    """float64 terms (T, 4) from fp32 alpha (T,K,K), u (T,Q,K) and the inputs, with the loose bounds (T, 4) of the shape sweep.
    All arguments are CPU tensors; x_s (T,S,K) / y_s (T,S) None in zero-shot."""
    a, u = alpha.double(), u.double()
    T, Q, K = u.shape
    logz = torch.log(x_q.double() + EPS)
    lg_sum, lg = torch.lgamma(a.sum(-1)), torch.lgamma(a)
    rowc = lg_sum - lg.sum(-1)                                                       # (T, K)
    logits = rowc[:, None, :] + torch.einsum("tkd,tqd->tqk", a - 1, logz)
    scale_k = lg_sum.abs() + lg.abs().sum(-1)                                        # (T, K)
    scale = scale_k[:, None, :] + torch.einsum("tkd,tqd->tqk", (a - 1).abs(), logz.abs())
    logu = torch.log(u + EPS)
    p = u.sum(1) / Q
    logp = torch.log(p + EPS)
    terms = torch.zeros(T, 4, dtype=torch.float64)
    terms[:, 0] = (u * logits).sum((1, 2))
    terms[:, 2] = (u * logu).sum((1, 2))
    terms[:, 3] = (p * logp).sum(1)
    abs_sums = torch.zeros(T, 4, dtype=torch.float64)
    abs_sums[:, 2] = (u * logu).abs().sum((1, 2))
    abs_sums[:, 3] = (p * logp).abs().sum(1)
    fit_s_scale, cnt = torch.zeros(T, dtype=torch.float64), np.zeros(T)
    if x_s is not None:
        logs = torch.log(x_s.double() + EPS)
        idx = y_s.long()[:, :, None].expand(-1, -1, K)
        a_y = torch.gather(a, 1, idx)                                                # (T, S, K): alpha[y_s]
        rc_y = torch.gather(rowc, 1, y_s.long())
        terms[:, 1] = (rc_y + ((a_y - 1) * logs).sum(-1)).sum(1)
        fit_s_scale = (rc_y.abs() + ((a_y - 1).abs() * logs.abs()).sum(-1)).sum(1)
        cnt = max_count(y_s.numpy(), K)
    b = bounds(abs_sums.numpy(), fit_s_scale.numpy(), Q, K, cnt)
    b[:, 0] = 2.0 ** -24 * (K + 4) * (u * scale).sum((1, 2)).numpy()
    return terms.numpy(), b


def make_tasks(T, Q, K, S, seed, empty_class=False):
    """Seeded rows on the simplex, peaked on a label: x_q (T,Q,K) and, with S > 0, x_s (T,S,K) with unbalanced labels y_s (T,S):
    every class once where S allows, the rest drawn at random; `empty_class`: the rows of class K - 1 are relabelled 0, so that
    class has no support row (cnt = 0) and the first query of every task is drawn from it."""
    gen = torch.Generator().manual_seed(seed)

    def rows(labels):
        logits = torch.randn(labels.numel(), K, generator=gen)
        logits[torch.arange(labels.numel()), labels.reshape(-1)] += 3.0
        return torch.softmax(3.0 * logits, -1).view(*labels.shape, K)

    q_labels = torch.randint(0, K, (T, Q), generator=gen)
    if empty_class and S:
        q_labels[:, 0] = K - 1          # its only mass: a class with neither support nor query mass is 0 / 0 in the M-step
    x_q = rows(q_labels)
    if not S:
        return x_q, None, None
    y_s = torch.randint(0, K, (T, S), generator=gen)
    y_s[:, :min(S, K)] = torch.arange(min(S, K))
    if empty_class:
        y_s[y_s == K - 1] = 0
    return x_q, rows(y_s), y_s


def as_tables(x_q, x_s, seed, permute):
    """The tasks as rows of shuffled feature tables (tables stacked from the task rows), `permute`: with a column permutation
    per task -> table_q, q_idx, table_s, s_idx, cols (None where absent)"""
    gen = torch.Generator().manual_seed(seed)
    T, _, K = x_q.shape
    cols = torch.stack([torch.randperm(K, generator=gen) for _ in range(T)]) if permute else None
    inv = torch.argsort(cols, dim=1) if permute else None

    def table(x):
        if x is None:
            return None, None
        src = torch.gather(x, 2, inv[:, None, :].expand_as(x)) if permute else x
        rows = src.reshape(-1, K)
        place = torch.randperm(rows.shape[0], generator=gen)
        tab = torch.empty_like(rows)
        tab[place] = rows
        return tab, place.view(T, -1)
    table_q, q_idx = table(x_q)
    table_s, s_idx = table(x_s)
    return table_q, q_idx, table_s, s_idx, (cols.to(torch.int32) if permute else None)
