#!/usr/bin/env python3
"""The measurements of DESIGN.md 8o (EM-Dirichlet stopped per batch once its assignments are stable), on one GPU:

  1. default path   with --parent DIR (a checkout of the parent commit with its library built): `bench.py --gpus 1` of this tree
                    and of DIR as child processes, alternating, --runs each; ms per step of every run, and the difference of the
                    medians next to the parent's own run-to-run spread
  2. machinery      the until-stable entry with patience = iters (it never stops) against the plain entry on the bench's
                    K = 1000 and K = 100 tasks, interleaved rounds in one process: the ratio of the medians, and that the bits agree
  3. what it buys   patience 1, 2, 3 on the same tasks: the distribution of outer_iters over the batches, wall time against the
                    plain run, mean accuracy against the plain run's

The tasks are bench.py's synthetic ones (tclip_amd.synth): what real CLIP features do is not measured here.

    python scripts/gpu_until_stable.py [--parent DIR] [--runs 3] [--rounds 2] [--out profiles/until_stable_ab.txt]"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = None


def say(text=""):
    print(text, flush=True)
    if OUT is not None:
        OUT.write(text + "\n")
        OUT.flush()


def bench_ms(tree, steps, warmup):
    """ms per step of one `bench.py --gpus 1` process of `tree`"""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True, timeout=600).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def default_path(parent, runs, steps, warmup):
    say(f"1. default path: bench.py --gpus 1 --steps {steps} --warmup {warmup}, this tree and the parent alternating, ms per step")
    ms = {"parent": [], "this": []}
    for r in range(runs):
        for name, tree in (("parent", parent), ("this", ROOT)):
            ms[name].append(bench_ms(tree, steps, warmup))
            say(f"   run {r} {name:6s} {ms[name][-1]:10.2f}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["parent"]) - min(ms["parent"])
    say(f"   medians: parent {med['parent']:.2f}, this {med['this']:.2f}: difference {med['this'] - med['parent']:+.2f} ms "
        f"({100 * (med['this'] / med['parent'] - 1):+.3f} %); the parent's own spread (max - min): {spread:.2f} ms "
        f"({100 * spread / med['parent']:.3f} %)")


def tasks_of(w):
    """the tasks of a bench workload as bench.py draws them: x_q (T,Q,K) and y_q (T,Q) on the device, the batch count"""
    import random

    import numpy as np
    import torch
    from src.eval_zero_shot import Evaluator_zero_shot
    from src.utils import CfgNode
    from tclip_amd import engine, synth
    K, N, B = w["K"], w["tasks_per_batch"], w["batches_per_gpu"]
    feats, labels = synth.make_feature_table(K, w["rows_per_class"], seed=2020)
    cfg = CfgNode(iter=20, iter_mm=1000, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, use_softmax_feature=True,
                  graph_matching=True, shots=0, number_tasks=N * B, batch_size=N, name_method="EM_DIRICHLET", used_test_set="test")
    ev = Evaluator_zero_shot(device=torch.device("cuda:0"), args=cfg, log_file=None)
    random.seed(2020)
    np.random.seed(2020)
    torch.manual_seed(2020)
    idx = ev.sample_indices(labels.numpy()).reshape(-1)
    x_q = engine.gather_rows(feats.cuda(), idx).view(B * N, 75, K)
    return x_q, labels[idx].view(B * N, 75), B


def timed(call):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = call()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def engine_level(w, rounds):
    import torch
    from tclip_amd import engine, until_stable
    x_q, y_q, B = tasks_of(w)
    K, iters = w["K"], 20
    kw = dict(n_batches=B, iters=iters, iter_mm=1000, lambd=int(K / 5) * 75)
    plain = lambda: engine.run_em_dirichlet(x_q, **kw)                                      # noqa: E731
    stable = lambda p: until_stable.run_em_dirichlet(x_q, patience=p, **kw)                 # noqa: E731
    accuracy = lambda r: float(engine.clustering_accuracy(x_q, r.preds, y_q, graph_matching=True)[0].mean())      # noqa: E731
    say(f"{w['name']}: K = {K}, {B} batches of {w['tasks_per_batch']} tasks, iter = {iters} x iter_mm = 1000")
    timed(plain)                                                                             # warm-up
    t = {"plain": [], "never": []}
    for _ in range(rounds):
        ref, s = timed(plain)
        t["plain"].append(s)
        never, s = timed(lambda: stable(iters))
        t["never"].append(s)
    same = all(torch.equal(getattr(ref, k), getattr(never, k)) for k in engine.EMDirichletResult.__slots__)
    mp, mn = statistics.median(t["plain"]), statistics.median(t["never"])
    say(f"   2. machinery: plain {['%.4f' % v for v in t['plain']]} s, until-stable with patience = iters {['%.4f' % v for v in t['never']]} s: "
        f"ratio of the medians {mn / mp:.4f}; results bit-identical: {same}; outer_iters {sorted(set(never.outer_iters.tolist()))}")
    acc0 = accuracy(ref)
    say(f"   3. what it buys (plain run: {mp:.4f} s, mean accuracy {acc0:.5f})")
    for p in (1, 2, 3):
        res, s = timed(lambda: stable(p))
        dist = collections.Counter(res.outer_iters.tolist())
        say(f"      patience {p}: outer_iters {dict(sorted(dist.items()))}, {s:.4f} s = {s / mp:.3f} of the plain run, "
            f"mean accuracy {accuracy(res):.5f} ({accuracy(res) - acc0:+.5f})")
    del x_q
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: runs part 1")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "until_stable_ab.txt"))
    args = ap.parse_args()
    global OUT
    OUT = open(args.out, "w")
    say("EM-Dirichlet until stable: synthetic tasks (tclip_amd.synth, bench.py's); real-feature behaviour is not measured")
    if args.parent:        # child processes, before this process opens the GPU
        default_path(os.path.abspath(args.parent), args.runs, args.steps, args.warmup)
    import bench
    for w in (bench.HEADLINE, bench.SECONDARY):
        engine_level(w, args.rounds)
    OUT.close()


if __name__ == "__main__":
    main()
