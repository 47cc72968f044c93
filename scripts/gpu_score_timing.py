#!/usr/bin/env python3
"""The measurements of DESIGN.md 8q (scoring with a fitted EM-Dirichlet model, tclip_amd.score), on one GPU:

  1. default path   with --parent-tree DIR (a built checkout of the parent commit): `python bench.py --gpus 1` of DIR and of this
                    tree in child processes, alternating, --runs each; every child's tasks/s, the medians, their ratio and the
                    parent's own run-to-run spread.  Runs first, before this process opens the GPU.
  2. scoring        the two regimes of the issue - many tasks x 75 rows (T = 125, K = 1000) and one task x many rows (T = 1,
                    R = 50 000, K = 1000) - timed with device events: --warmup calls, then --reps calls, the median; with u and
                    for labels only.  The fp32 multiply-add rate is 2 T R K^2 flop over that time, as a fraction of the 157.3
                    TFLOP/s vector peak (the contraction only: the row constants, logarithms and softmax are not counted).  The
                    workspace bytes are the query's.
  3. for scale      the torch restatement of the same call on this host's CPU at 16 threads, on --cpu-chunks chunks of one task
                    x 75 rows, scaled to the call (the full call is T R / 75 such chunks).

There is no threshold: the numbers are a record.  The script ends itself after --limit seconds and retries nothing.

    python scripts/gpu_score_timing.py [--parent-tree DIR] [--runs 2] [--out profiles/score_timing.txt]"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PEAK_VALU_FLOPS = 157.3e12
REGIMES = (("many tasks x 75 rows", 125, 75, 1000), ("one task x many rows", 1, 50000, 1000))
OUT = None


def say(text=""):
    print(text, flush=True)
    if OUT is not None:
        OUT.write(text + "\n")
        OUT.flush()


def bench_value(tree, steps, warmup, timeout):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True, timeout=timeout).stdout
    return float(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["value"])


def default_path(parent_tree, runs, steps, warmup, timeout):
    say(f"1. default path: python bench.py --gpus 1 --steps {steps} --warmup {warmup} in child processes, the parent's tree and this "
        f"one alternating, tasks/s")
    vals = {"parent": [], "this": []}
    for r in range(runs):
        for which, tree in (("parent", parent_tree), ("this", ROOT)):
            vals[which].append(bench_value(tree, steps, warmup, timeout))
            say(f"   run {r} {which:6s} {vals[which][-1]:9.3f}")
    mp, mt = statistics.median(vals["parent"]), statistics.median(vals["this"])
    spread = max(vals["parent"]) - min(vals["parent"])
    say(f"   medians: parent {mp:.3f}, this {mt:.3f} tasks/s: ratio {mt / mp:.5f} ({100 * (mt / mp - 1):+.3f} %); the parent's own "
        f"spread (max - min of its runs): {spread:.3f} tasks/s ({100 * spread / mp:.3f} %)")


def model(T, R, K, seed=0):
    """a seeded model and rows on the device: alpha log-uniform in [1e-1, 1e2], v = log(p) + 1, peaked simplex rows"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    alpha = torch.exp(torch.rand(T, K, K, device="cuda", generator=gen) * 6.9 - 2.3)
    v = torch.log_softmax(torch.randn(T, K, device="cuda", generator=gen), -1) + 1
    x = torch.softmax(3 * torch.randn(T, R, K, device="cuda", generator=gen), -1)
    return x, alpha, v


def device_ms(call, warmup, reps):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def cpu_restatement_s(x, alpha, v, lambd, n_query, chunks):
    """the reference's get_logits + u_update in torch fp32 on the host, on `chunks` chunks of one task x 75 rows -> seconds per
    chunk (median)"""
    import torch
    a, vv = alpha[0].cpu(), v[0].cpu()
    rows = x.reshape(-1, x.shape[-1])[:75 * chunks].cpu()
    secs = []
    for c in range(chunks):
        z = rows[75 * c:75 * (c + 1)]
        t0 = time.perf_counter()
        l1 = torch.lgamma(a.sum(-1)).unsqueeze(0)
        l2 = -torch.lgamma(a).sum(-1).unsqueeze(0)
        l3 = ((a.unsqueeze(0) - 1) * torch.log(z + 1e-15).unsqueeze(1)).sum(-1)
        u = (l1 + l2 + l3 + lambd * vv.unsqueeze(0) / n_query).softmax(1)
        u.argmax(1)
        secs.append(time.perf_counter() - t0)
    return statistics.median(secs)


def scoring(warmup, reps, cpu_chunks):
    import torch
    from tclip_amd import _capi, score
    torch.set_num_threads(16)
    say(f"2. scoring, device events, {warmup} warm-up calls, median of {reps} (min .. max), ms; 3. torch fp32 on the host CPU, "
        f"{torch.get_num_threads()} threads")
    for name, T, R, K in REGIMES:
        x, alpha, v = model(T, R, K)
        kw = dict(lambd=int(K / 5) * 75, n_query=75)
        p = _capi.ScoreProblem(T, R, K, kw["lambd"], 75, 0)
        ws = _capi.lib().tclip_em_dirichlet_score_workspace_bytes(ctypes.byref(p))
        flop = 2.0 * T * R * K * K
        say(f"   {name}: T = {T}, R = {R}, K = {K}; workspace {ws} bytes; contraction {flop / 1e9:.1f} GFLOP; u is "
            f"{4 * T * R * K / 1e6:.1f} MB, alpha {4 * T * K * K / 1e6:.1f} MB")
        for label, opts in (("u and preds", dict()), ("preds only", dict(want_u=False)), ("u, preds and logits", dict(want_logits=True))):
            ms = device_ms(lambda: score.score_em_dirichlet(x, alpha, v, **opts, **kw), warmup, reps)
            med = statistics.median(ms)
            say(f"      {label:20s} {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f}): {flop / (med * 1e-3) / 1e12:6.2f} TFLOP/s = "
                f"{100 * flop / (med * 1e-3) / PEAK_VALU_FLOPS:5.2f} % of the {PEAK_VALU_FLOPS / 1e12:.1f} TFLOP/s fp32 vector peak")
        per_chunk = cpu_restatement_s(x, alpha, v, kw["lambd"], 75, cpu_chunks)
        n_chunks = T * R / 75.0
        say(f"      torch on the CPU     {1e3 * per_chunk:9.1f} ms per chunk of one task x 75 rows (median of {cpu_chunks}); the call is "
            f"{n_chunks:.0f} chunks: {per_chunk * n_chunks:.1f} s scaled")
        del x, alpha, v
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: runs part 1")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--bench-timeout", type=int, default=300, help="seconds per bench.py child")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-chunks", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="the script ends itself after this many seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_timing.txt"))
    args = ap.parse_args()
    signal.alarm(args.limit)
    global OUT
    OUT = open(args.out, "w")
    say("Scoring with a fitted EM-Dirichlet model: seeded synthetic models and rows, one MI355X")
    if args.parent_tree:       # child processes, before this process opens the GPU
        default_path(os.path.abspath(args.parent_tree), args.runs, args.bench_steps, args.bench_warmup, args.bench_timeout)
    scoring(args.warmup, args.reps, args.cpu_chunks)
    OUT.close()


if __name__ == "__main__":
    main()
