"""The until-stable stop rule restated on the host, and the fixtures it is pinned on (tests/test_until_stable.py,
tests/test_gpu_until_stable.py)."""
import os

import numpy as np

from conftest import GOLDEN

# fixture -> the outer iterations a batch runs with patience 1, 2, 3 (the stopping iteration counted; iters = it never stops),
# read off the reference's own argmax after every outer iteration
STOPS = {
    "bigbatch_zs_soft_K1000_N17": (3, 6, 7),
    "zs_soft_K1000_N3": (3, 4, 5),
    "zs_soft_K397_N1": (11, 12, 13),
    "zs_soft_K100_N4": (3, 4, 5),
    "zs_soft_K37_N6": (4, 5, 6),
    "zs_soft_K10_N4": (4, 9, 10),
    "zs_soft_K7_N4": (7, 8, 20),
    "zs_hard_K37_N6": (3, 4, 5),
    "zs_hard_K397_N2": (3, 4, 5),
    "fs_soft_K37_N3_s2": (5, 8, 9),
    "fs_soft_K100_N4_s4": (10, 11, 12),
    "fs_hard_K10_N4_s4": (3, 4, 5),
    "fs_hard_K100_N3_s4": (9, 10, 10),
    "bigbatch_zs_soft_K100_N170": (14, 19, 20),
}
# the leading changes per iteration, from iteration 1, of the fixtures whose trace the issue's table spells out
CHANGES_HEAD = {
    "bigbatch_zs_soft_K1000_N17": [33, 0, 1, 0, 0],
    "zs_soft_K397_N1": [4, 2, 4, 10, 6, 1, 1, 1, 1, 0],
    "zs_soft_K7_N4": [3, 1, 1, 2, 3, 0, 0, 2, 1, 0, 1, 1, 2, 2, 1, 0, 2, 2, 0],
    "fs_soft_K100_N4_s4": [14, 15, 26, 54, 35, 20, 9, 8, 0],
    "fs_hard_K100_N3_s4": [9, 4, 9, 25, 41, 21, 1, 0, 0],
}


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def changes_of(argmax):
    """argmax (iters, T, Q) of ONE batch -> changes (iters,): changes[0] = T * Q, changes[it] = pairs that differ from it - 1"""
    argmax = np.asarray(argmax)
    out = np.empty(argmax.shape[0], np.int64)
    out[0] = argmax[0].size
    out[1:] = (argmax[1:] != argmax[:-1]).reshape(argmax.shape[0] - 1, -1).sum(1)
    return out


def stop_of(changes, patience):
    """outer iterations run: it + 1 for the first it whose last `patience` changes are all 0, else len(changes)"""
    quiet = 0
    for it, c in enumerate(changes):
        quiet = quiet + 1 if c == 0 else 0
        if quiet >= patience:
            return it + 1
    return len(changes)


def synthetic_batches(K, N, specs, shots=0):
    """One batch of N synthetic tasks per (seed, k_eff) of `specs` (tclip_amd.synth; k_eff: the classes a task's queries are
    drawn from - fewer is easier) -> x_q (B*N, 75, K), y_q (B*N, 75), and with shots > 0 x_s (B*N, K*shots, K), y_s (B*N, K*shots)"""
    import torch
    from tclip_amd import synth
    xq, yq, xs, ys = [], [], [], []
    for seed, k_eff in specs:
        x, y = synth.make_query_tasks(N, K, seed=seed, k_eff=k_eff)
        xq.append(x)
        yq.append(y.squeeze(2))
        if shots:
            s, l = synth.make_support(N, K, shots, seed=seed)
            xs.append(s)
            ys.append(l.squeeze(2))
    if shots:
        return torch.cat(xq), torch.cat(yq), torch.cat(xs), torch.cat(ys)
    return torch.cat(xq), torch.cat(yq)


def reference_stops(x_q, x_s, y_s, n_batches, patience, **kw):
    """oracle.ref_torch on the CPU, batch by batch -> [outer iterations under the rule], [changes (iters,)]"""
    from oracle import ref_torch
    N = x_q.shape[0] // n_batches
    stops, traces = [], []
    for b in range(n_batches):
        sl = slice(b * N, (b + 1) * N)
        trace = {}
        ref_torch.run(x_q[sl], None if x_s is None else x_s[sl], None if y_s is None else y_s[sl], n_class=x_q.shape[2],
                      trace=trace, **kw)
        changes = changes_of(np.stack([a.numpy() for a in trace["argmax"]]))
        stops.append(stop_of(changes, patience))
        traces.append(changes)
    return stops, traces


# Synthetic calls of several batches: name -> K, N, (seed, k_eff) per batch, shots, patience, iters, iter_mm and the outer
# iterations oracle.ref_torch gives every batch under the rule (tests/test_until_stable.py recomputes them on the CPU).
#   two_groups    B * N * K = 16 400 rows: two stream groups of two batches
#   one_group     a single stream group
#   few_shot      through the feature tables with a column permutation per task
#   isolation     the first batch stops early, the last never
SYNTHETIC = {
    "two_groups": dict(K=100, N=41, specs=[(11, 3), (11, 6), (12, 3), (12, 6)], shots=0, patience=2, iters=8, iter_mm=120,
                       stops=[6, 5, 6, 8]),
    "one_group": dict(K=37, N=3, specs=[(21, 3), (21, 10), (22, 3), (22, None), (23, 10)], shots=0, patience=2, iters=12,
                      iter_mm=120, stops=[4, 6, 5, 6, 4]),
    "few_shot": dict(K=37, N=3, specs=[(31, 3), (31, 10), (33, 5), (32, 10), (34, 3)], shots=2, patience=1, iters=12,
                     iter_mm=120, stops=[6, 3, 4, 12, 6]),
    "isolation": dict(K=37, N=3, specs=[(21, 3), (22, None)], shots=0, patience=3, iters=6, iter_mm=120, stops=[5, 6]),
}


def synthetic_case(name):
    """-> the case's dict with its tensors: x_q, y_q[, x_s, y_s] and lambd (the reference's int(K / 5) * n_query)"""
    c = dict(SYNTHETIC[name])
    out = synthetic_batches(c["K"], c["N"], c["specs"], c["shots"])
    c["x_q"], c["y_q"] = out[0], out[1]
    c["x_s"], c["y_s"] = (out[2], out[3]) if c["shots"] else (None, None)
    c["lambd"] = int(c["K"] / 5) * 75
    return c


def as_tables(x_q, x_s, seed):
    """The tasks as rows of two shuffled feature tables with a column permutation per task:
    table_q[q_idx[t, r], cols[t, d]] = x_q[t, r, d], the same for the support set -> table_q, q_idx, table_s, s_idx, cols"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    T, _, K = x_q.shape
    cols = torch.stack([torch.randperm(K, generator=gen) for _ in range(T)])
    inv = torch.argsort(cols, dim=1)

    def table(x):
        rows = torch.gather(x, 2, inv[:, None, :].expand_as(x)).reshape(-1, K)
        place = torch.randperm(rows.shape[0], generator=gen)
        tab = torch.empty_like(rows)
        tab[place] = rows
        return tab, place.view(T, -1)
    table_q, q_idx = table(x_q)
    table_s, s_idx = table(x_s)
    return table_q, q_idx, table_s, s_idx, cols.to(torch.int32)
