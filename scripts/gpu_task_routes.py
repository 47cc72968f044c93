"""Evaluator default route against materialise_tasks on one MI355X: PADDLE on visual features at K = 1000, D = 1024, 4 shots,
100 tasks, 20 iterations; BDCSPN on softmax features at K = 1000.  One warm-up of each variant, then 3 alternated repeats.
Prints the record as one JSON line; `python scripts/gpu_task_routes.py FILE` also writes it to FILE."""
import json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in")):
    sys.path.insert(0, p)
import numpy as np
import torch
from src.eval_few_shot import Evaluator_few_shot, relabel_batch, relabel_indices
from src.utils import CfgNode
from tclip_amd import engine

DEV = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else None      # optional: a file that receives the record after every comparison
res = {}


def args(method, K, visual, **kw):
    a = CfgNode(iter=20, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=not visual,
                name_method=method, lambd=5.0, temp=15.0, norm_type="L2N", number_tasks=100, batch_size=100, shots=4,
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


def compare(name, method, K, W, visual):
    tabs = tables(K, W, 20, not visual, 11)
    dev_tabs = [tabs[0].to(DEV), tabs[1], tabs[2].to(DEV), tabs[3]]
    random.seed(3); torch.manual_seed(3); np.random.seed(3)
    ev0 = Evaluator_few_shot(device=DEV, args=args(method, K, visual), log_file=None)
    indices = ev0.sample_indices(tabs[1].numpy(), tabs[3].numpy())
    variants = {"default": {}, "materialise_tasks": {"materialise_tasks": True}}
    rec = {k: {"wall_s": [], "peak_bytes": []} for k in variants}
    preds = {}
    for rep in range(4):                      # rep 0 is the warm-up
        for k, kw in variants.items():
            ev = Evaluator_few_shot(device=DEV, args=args(method, K, visual, **kw), log_file=None)
            t, peak, (acc, _) = timed(lambda: ev.evaluate_tasks(None, *dev_tabs, indices=indices))
            preds[k] = (ev.last_task_predictions.copy(), float(acc))
            if rep:
                rec[k]["wall_s"].append(t)
                rec[k]["peak_bytes"].append(peak)
            print(name, rep, k, f"{t:.4f} s", f"{peak / 1e6:.1f} MB", float(acc), flush=True)
    rec["identical"] = bool(np.array_equal(preds["default"][0], preds["materialise_tasks"][0]) and preds["default"][1] == preds["materialise_tasks"][1])
    res[name] = rec
    if OUT:
        json.dump(res, open(OUT, "w"), indent=1)
    return dev_tabs, tabs, indices


compare("paddle_visual_K1000_D1024_s4_T100", "PADDLE", 1000, 1024, True)
dev_tabs, tabs, (s_idx, q_idx) = compare("bdcspn_softmax_K1000_s4_T100", "BDCSPN", 1000, 1000, False)

# the task construction alone, BDCSPN's inputs at K = 1000: fused builder against gather_rows + relabel_batch
K, S, Q = 1000, 4000, 75
si, qi = s_idx.reshape(-1, S), q_idx.reshape(-1, Q)
y_s, y_q = tabs[1][si.reshape(-1)].view(-1, S), tabs[3][qi.reshape(-1)].view(-1, Q)


def builder():
    cols, a, b = relabel_indices(y_s, y_q, K)
    return engine.gather_task_rows(dev_tabs[0], si, cols), engine.gather_task_rows(dev_tabs[2], qi, cols), a, b


def host_route():
    x_s = engine.gather_rows(dev_tabs[0], si.reshape(-1)).view(-1, S, K)
    x_q = engine.gather_rows(dev_tabs[2], qi.reshape(-1)).view(-1, Q, K)
    return relabel_batch(x_s, x_q, y_s, y_q, True)


rec = {"builder": {"wall_s": [], "peak_bytes": []}, "gather_rows_relabel_batch": {"wall_s": [], "peak_bytes": []}}
for rep in range(4):
    for k, fn in (("builder", builder), ("gather_rows_relabel_batch", host_route)):
        t, peak, out = timed(fn)
        if rep:
            rec[k]["wall_s"].append(t)
            rec[k]["peak_bytes"].append(peak)
        if k == "builder":
            ref = out
        else:
            rec["identical"] = bool(all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(ref, out)))
        del out
        print("task construction", rep, k, f"{t:.4f} s", f"{peak / 1e6:.1f} MB", flush=True)
    del ref
res["task_construction_softmax_K1000_s4_T100"] = rec
if OUT:
    json.dump(res, open(OUT, "w"), indent=1)
print(json.dumps(res))
