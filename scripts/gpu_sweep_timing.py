"""One value-sweep call (engine.sweep_*_tasks) against the sum of its single-value run_*_tasks calls on one GPU: device events
around each, one warm-up each, five alternating repeats in one process; per method the median, minimum and maximum of both and
the allocator's peak rise during a call.  Sizes: the reference's tuning size (5 tasks, Q = 35, K = 100, 4 shots,
the grids of its scripts/opt_parameters.sh) and K = 1000, 4 shots, 100 tasks (ALPHA_TIM there with 3 values and 20 steps).

    python scripts/gpu_sweep_timing.py [small|large|both] [FILE]

Prints one JSON line per method and size; with FILE also writes the records there."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transductive-clip_amd"))
from tclip_amd import engine, synth  # noqa: E402

DEV = "cuda:0"
GRIDS = {"alpha_tim": [1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0],
         "bdcspn": [1.0, 3.0, 5.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0],
         "paddle": [0.0, 1.0, 2.0, 5.0, 10.0, 20.0, 35.0, 50.0, 100.0],
         "lshot": [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]}


def inputs(T, Q, K, shots, seed=1):
    per_class = 2 * shots
    (ts, labels), (tq, _) = synth.make_feature_table(K, per_class, seed=seed), synth.make_feature_table(K, per_class, seed=seed + 1)
    gen = torch.Generator().manual_seed(seed)
    s_idx = torch.stack([torch.cat([k * per_class + torch.randperm(per_class, generator=gen)[:shots] for k in range(K)]) for _ in range(T)])
    q_idx = torch.randint(0, K * per_class, (T, Q), generator=gen)
    y_s = (K - 1 - labels[s_idx]).to(DEV)
    cols = torch.arange(K - 1, -1, -1, dtype=torch.int32).repeat(T, 1).to(DEV)      # the evaluator's reversal
    return tq.to(DEV), q_idx.to(DEV), ts.to(DEV), s_idx.to(DEV), y_s, cols


def calls(name, inp, values, tim_iters):
    tq, qi, ts, si, ys, cols = inp
    if name == "paddle":
        return (lambda: engine.sweep_paddle_tasks(tq, qi, ts, si, ys, cols, iters=20, values=values),
                lambda v: engine.run_paddle_tasks(tq, qi, ts, si, ys, cols, iters=20, lambd=v))
    if name == "bdcspn":
        return (lambda: engine.sweep_bdcspn_tasks(tq, qi, ts, si, ys, cols, values=values),
                lambda v: engine.run_bdcspn_tasks(tq, qi, ts, si, ys, cols, temp=v))
    if name == "lshot":
        return (lambda: engine.sweep_laplacian_shot_tasks(tq, qi, ts, si, ys, cols, iters=20, knn=3, values=values),
                lambda v: engine.run_laplacian_shot_tasks(tq, qi, ts, si, ys, cols, iters=20, knn=3, lmd=v))
    kw = dict(iters=tim_iters, temp=15.0, lr=1e-4)
    return (lambda: engine.sweep_alpha_tim_tasks(tq, qi, ts, si, ys, cols, values=values, **kw),
            lambda v: engine.run_alpha_tim_tasks(tq, qi, ts, si, ys, cols, alpha_value=v, **kw))


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return a.elapsed_time(b), peak


def measure(name, size, inp, values, tim_iters, repeats=5):
    sweep, single = calls(name, inp, values, tim_iters)

    def singles():
        for v in values:
            single(v)                      # outputs dropped, as separate runs drop them
    timed(sweep), timed(singles)           # warm-up
    ts, tl, ps, pl = [], [], 0, 0
    for _ in range(repeats):
        t, p = timed(sweep)
        ts.append(t)
        ps = max(ps, p)
        t, p = timed(singles)
        tl.append(t)
        pl = max(pl, p)
    med = lambda x: sorted(x)[len(x) // 2]      # noqa: E731
    rec = dict(method=name, size=size, n_values=len(values), tim_iters=tim_iters if name == "alpha_tim" else None,
               sweep_ms=dict(median=med(ts), min=min(ts), max=max(ts)), singles_ms=dict(median=med(tl), min=min(tl), max=max(tl)),
               sweep_peak_bytes=ps, singles_peak_bytes=pl)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    out = []
    if which in ("small", "both"):
        inp = inputs(5, 35, 100, 4)
        for name in ("paddle", "bdcspn", "lshot", "alpha_tim"):
            out.append(measure(name, "T=5 Q=35 K=100 S=400", inp, GRIDS[name], 1000))
    if which in ("large", "both"):
        inp = inputs(100, 75, 1000, 4)
        for name in ("paddle", "bdcspn", "lshot"):
            out.append(measure(name, "T=100 Q=75 K=1000 S=4000", inp, GRIDS[name], 0))
        out.append(measure("alpha_tim", "T=100 Q=75 K=1000 S=4000", inp, [2.0, 4.5, 7.0], 20, repeats=5))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
