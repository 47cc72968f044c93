"""Evaluator default route against `in_place_loop` on one MI355X: TIM-GD on softmax features (K = 1000) and on visual features
(K = 1000, D = 1024), ALPHA_TIM on softmax features (K = 1000); 4 shots, 100 tasks in one batch, STEPS Adam steps per call.  One
warm-up of each variant, then 3 alternated repeats in one process; wall time of evaluate_tasks (a host clock around a call that
ends in a device synchronise) and torch.cuda.max_memory_allocated over the call minus what was allocated before it (the tables
excluded), next to the engine's workspace query and the bytes of x_s + x_q, the expected difference of the two peaks.  The
evaluator's column permutation on softmax features is the reference's reversal K-1..0.
Then, at the engine level, what fetching elements through `cols` does: engine.run_tim_gd_tasks on the softmax tables without
cols (128-bit loads in the interior tiles), with the reversal and with a random permutation per task, next to the dense
engine.run_tim_gd on materialised tensors; same protocol.  The whole call is timed; the two GEMMs are all of a step that reads
the task rows, the other kernels are the same in every variant.
Prints the record as one JSON line; `python scripts/gpu_tim_in_place.py FILE` also writes it to FILE."""
import ctypes, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in")):
    sys.path.insert(0, p)
import numpy as np
import torch
from src.eval_few_shot import Evaluator_few_shot
from src.utils import CfgNode
from tclip_amd import _capi, engine

DEV = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else None      # optional: a file that receives the record after every comparison
T, Q, SHOTS, STEPS = 100, 75, 4, 50
res = {"steps": STEPS}


def args(method, K, visual, **kw):
    a = CfgNode(iter=STEPS, num_classes_test=K, n_class=K, n_query=Q, k_eff=5, T=30.0, use_softmax_feature=not visual,
                name_method=method, temp=15.0, loss_weights=[1.0, 0.3, 1.0], lr_tim=1e-4, lr_alpha_tim=1e-4,
                entropies=["Shannon", "Alpha", "Alpha"], alpha_value=7.0, number_tasks=T, batch_size=T, shots=SHOTS,
                used_test_set="test", dataset="synthetic", tunable=False)
    a.update(kw)
    return a


def tables(K, W, rows_per_class, softmax, seed):
    gen = torch.Generator().manual_seed(seed)
    labels = torch.arange(K).repeat_interleave(rows_per_class)
    out = []
    for _ in range(2):
        x = torch.randn(K * rows_per_class, W, generator=gen)
        if softmax:
            x[torch.arange(x.shape[0]), labels] += 4.0
            x = x.softmax(-1)
        else:
            x = x / W ** 0.5
        out += [x, labels.clone()]
    return out


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base, r


def workspace(method, K, W, visual):
    """the engine's own figure for the problem (one query for both routes), and the tensors the default route builds"""
    lib = _capi.lib()
    S = K * SHOTS
    p = ctypes.byref(_capi.Problem(1, T, Q, K, S, STEPS, 1, 0, 0))
    ws = lib.tclip_tim_gd_tasks_workspace_bytes(p, W) if method == "TIM-GD" else lib.tclip_alpha_tim_tasks_workspace_bytes(p)
    return {"workspace_bytes": ws, "x_s_bytes": T * S * W * 4, "x_q_bytes": T * Q * W * 4}


def alternate(name, variants, same):
    """variants: {label: callable -> comparable result}; one warm-up and three timed calls each, alternated"""
    rec = {k: {"wall_s": [], "peak_bytes": []} for k in variants}
    got = {}
    for rep in range(4):                      # rep 0 is the warm-up
        for k, fn in variants.items():
            t, peak, got[k] = timed(fn)
            if rep:
                rec[k]["wall_s"].append(t)
                rec[k]["peak_bytes"].append(peak)
            print(name, rep, k, f"{t:.4f} s", f"{peak / 1e6:.1f} MB", flush=True)
    first = next(iter(variants))
    rec["identical"] = {k: bool(same(got[first], got[k])) for k in variants if k != first}
    return rec


def compare(name, method, K, W, visual):
    tabs = tables(K, W, 20, not visual, 11)
    dev_tabs = [tabs[0].to(DEV), tabs[1], tabs[2].to(DEV), tabs[3]]
    random.seed(3); torch.manual_seed(3); np.random.seed(3)
    ev0 = Evaluator_few_shot(device=DEV, args=args(method, K, visual), log_file=None)
    indices = ev0.sample_indices(tabs[1].numpy(), tabs[3].numpy())

    def run(**kw):
        ev = Evaluator_few_shot(device=DEV, args=args(method, K, visual, **kw), log_file=None)
        acc, _ = ev.evaluate_tasks(None, *dev_tabs, indices=indices)
        return ev.last_task_predictions.copy(), ev.last_task_accuracies.copy(), float(acc)

    rec = alternate(name, {"default": run, "in_place_loop": lambda: run(in_place_loop=True)},
                    lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2])
    rec.update(workspace(method, K, W, visual))
    res[name] = rec
    if OUT:
        json.dump(res, open(OUT, "w"), indent=1)
    del dev_tabs
    torch.cuda.empty_cache()


def cols_cost(name, K):
    """engine level, softmax tables: the two GEMMs' reads without cols, through the reversal, through a random permutation"""
    tabs = tables(K, K, 20, True, 11)
    table_s, table_q = tabs[0].to(DEV), tabs[2].to(DEV)
    gen = torch.Generator().manual_seed(5)
    S = K * SHOTS
    # SHOTS rows of every class per task (the tables are class-sorted, 20 rows per class), in a shuffled order
    s_idx = (torch.arange(K).view(1, K, 1) * 20 + torch.randint(0, 20, (T, K, SHOTS), generator=gen)).view(T, S)
    s_idx = torch.stack([row[torch.randperm(S, generator=gen)] for row in s_idx]).to(DEV)
    q_idx = torch.randint(0, table_q.shape[0], (T, Q), generator=gen).to(DEV)
    y_s = tabs[1].to(DEV)[s_idx]
    reversal = torch.arange(K - 1, -1, -1, dtype=torch.int32).repeat(T, 1).to(DEV)
    shuffled = torch.stack([torch.randperm(K, generator=gen) for _ in range(T)]).to(torch.int32).to(DEV)
    prm = dict(n_class=K, iters=STEPS, temp=15.0, lr=1e-4, loss_weights=[1.0, 0.3, 1.0])
    # labels follow the columns only through the class means; for a timing the un-permuted labels do
    variants = {
        "dense_no_cols": lambda: engine.run_tim_gd(engine.gather_task_rows(table_q, q_idx), engine.gather_task_rows(table_s, s_idx), y_s, **prm),
        "in_place_no_cols": lambda: engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, **prm),
        "in_place_reversal": lambda: engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, reversal, **prm),
        "in_place_random_cols": lambda: engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, shuffled, **prm),
    }
    rec = alternate(name, variants, lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b)))
    del rec["identical"]["in_place_reversal"], rec["identical"]["in_place_random_cols"]      # other columns: other results
    res[name] = rec
    if OUT:
        json.dump(res, open(OUT, "w"), indent=1)
    torch.cuda.empty_cache()


compare("tim_gd_softmax_K1000_s4_T100", "TIM-GD", 1000, 1000, False)
compare("tim_gd_visual_K1000_D1024_s4_T100", "TIM-GD", 1000, 1024, True)
compare("alpha_tim_softmax_K1000_s4_T100", "ALPHA_TIM", 1000, 1000, False)
cols_cost("tim_gd_softmax_K1000_cols", 1000)
print(json.dumps(res))
