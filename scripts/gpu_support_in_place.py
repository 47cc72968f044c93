"""Evaluator default route against `in_place_support` on one MI355X: BDCSPN on softmax features (K = 1000) and on visual features
(K = 1000, D = 1024), LAPLACIAN_SHOT on softmax features (K = 1000); 4 shots, 100 tasks in one batch.  One warm-up of each
variant, then 3 alternated repeats in one process; wall time of evaluate_tasks and torch.cuda.max_memory_allocated over the call
minus what was allocated before it (the tables excluded), next to the engine's workspace queries for the same problem.
Prints the record as one JSON line; `python scripts/gpu_support_in_place.py FILE` also writes it to FILE."""
import ctypes, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in")):
    sys.path.insert(0, p)
import numpy as np
import torch
from src.eval_few_shot import Evaluator_few_shot
from src.utils import CfgNode
from tclip_amd import _capi

DEV = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else None      # optional: a file that receives the record after every comparison
T, Q, SHOTS = 100, 75, 4
res = {}


def args(method, K, visual, **kw):
    a = CfgNode(iter=20, num_classes_test=K, n_class=K, n_query=Q, k_eff=5, T=30.0, use_softmax_feature=not visual,
                name_method=method, lambd=5.0, temp=15.0, norm_type="L2N", knn=3, lmd=0.7, number_tasks=T, batch_size=T, shots=SHOTS,
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


def workspaces(method, K, W, visual):
    """the engine's own figures for the problem: dense and in-place workspace, and the tensors the default route builds"""
    lib = _capi.lib()
    S = K * SHOTS
    p = ctypes.byref(_capi.Problem(1, T, Q, K, S, 20, 1, 0, 0))
    stem = {"BDCSPN": "tclip_bdcspn", "LAPLACIAN_SHOT": "tclip_laplacian_shot"}[method] + ("_visual" if visual else "")
    dim = (W,) if visual else ()
    return {"dense_workspace_bytes": getattr(lib, stem + "_workspace_bytes")(p, *dim),
            "in_place_workspace_bytes": getattr(lib, stem + "_tasks_workspace_bytes")(p, *dim),
            "x_s_bytes": T * S * W * 4, "x_q_bytes": T * Q * W * 4}


def compare(name, method, K, W, visual):
    tabs = tables(K, W, 20, not visual, 11)
    dev_tabs = [tabs[0].to(DEV), tabs[1], tabs[2].to(DEV), tabs[3]]
    random.seed(3); torch.manual_seed(3); np.random.seed(3)
    ev0 = Evaluator_few_shot(device=DEV, args=args(method, K, visual), log_file=None)
    indices = ev0.sample_indices(tabs[1].numpy(), tabs[3].numpy())
    variants = {"default": {}, "in_place_support": {"in_place_support": True}}
    rec = {k: {"wall_s": [], "peak_bytes": []} for k in variants}
    rec.update(workspaces(method, K, W, visual))
    preds = {}
    for rep in range(4):                      # rep 0 is the warm-up
        for k, kw in variants.items():
            ev = Evaluator_few_shot(device=DEV, args=args(method, K, visual, **kw), log_file=None)
            t, peak, (acc, _) = timed(lambda: ev.evaluate_tasks(None, *dev_tabs, indices=indices))
            preds[k] = (ev.last_task_predictions.copy(), ev.last_task_accuracies.copy(), float(acc))
            if rep:
                rec[k]["wall_s"].append(t)
                rec[k]["peak_bytes"].append(peak)
            print(name, rep, k, f"{t:.4f} s", f"{peak / 1e6:.1f} MB", float(acc), flush=True)
    a, b = preds["default"], preds["in_place_support"]
    rec["identical"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2])
    res[name] = rec
    if OUT:
        json.dump(res, open(OUT, "w"), indent=1)
    del dev_tabs
    torch.cuda.empty_cache()


compare("bdcspn_softmax_K1000_s4_T100", "BDCSPN", 1000, 1000, False)
compare("bdcspn_visual_K1000_D1024_s4_T100", "BDCSPN", 1000, 1024, True)
compare("laplacian_shot_softmax_K1000_s4_T100", "LAPLACIAN_SHOT", 1000, 1000, False)
print(json.dumps(res))
