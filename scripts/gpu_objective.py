#!/usr/bin/env python3
"""The measurements of DESIGN.md 8p (EM-Dirichlet with the objective recorded per task and outer iteration), on one GPU, on
bench.py's K = 1000 and K = 100 synthetic shapes at 20 outer iterations:

  1. default path   with --parent-lib FILE (libtclip.so built from the parent commit): the plain entry of this tree's library and
                    of FILE in child processes, alternating, --runs each; the median seconds per call of every child, the ratio
                    of the medians next to the parent's own run-to-run spread.  The child that loads FILE drops the three symbols
                    the parent's library does not have from the binding's table; nothing else differs between the two.
  2. the opt-in     the objective entry at patience 0 against the plain entry, interleaved rounds in one process: the ratio of
                    the medians, the extra seconds per outer iteration next to the traffic estimate (3 T Q K 4 bytes: logit0 once,
                    u twice), and that the shared outputs keep their bits

No threshold is fixed in advance: both ratios are recorded as they come.

    python scripts/gpu_objective.py [--parent-lib FILE] [--runs 3] [--rounds 3] [--out profiles/objective_ab.txt]"""
import argparse
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

NEW_SYMBOLS = ("tclip_em_dirichlet_objective_workspace_bytes", "tclip_em_dirichlet_run_objective",
               "tclip_em_dirichlet_run_tasks_objective")
HBM_BYTES_PER_S = 8e12          # MI355X peak; the estimate's yardstick, not a measurement
OUT = None


def say(text=""):
    print(text, flush=True)
    if OUT is not None:
        OUT.write(text + "\n")
        OUT.flush()


def timed(call):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = call()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def workloads():
    import bench
    return {w["name"]: w for w in (bench.HEADLINE, bench.SECONDARY)}


def tasks_and_kw(w):
    from gpu_until_stable import tasks_of
    x_q, _, B = tasks_of(w)
    return x_q, dict(n_batches=B, iters=20, iter_mm=1000, lambd=int(w["K"] / 5) * 75)


def child(name, rounds):
    """one process: the plain entry on workload `name`, one warm-up and `rounds` timed calls -> a JSON line"""
    from tclip_amd import _capi, engine
    if os.environ.get("TCLIP_LIB"):
        for n in NEW_SYMBOLS:
            _capi._SIGNATURES.pop(n, None)
    x_q, kw = tasks_and_kw(workloads()[name])
    timed(lambda: engine.run_em_dirichlet(x_q, **kw))
    secs = [timed(lambda: engine.run_em_dirichlet(x_q, **kw))[1] for _ in range(rounds)]
    print(json.dumps({"seconds": secs}), flush=True)


def default_path(parent_lib, names, runs, rounds):
    say(f"1. default path: engine.run_em_dirichlet in child processes, the parent's library and this tree's alternating, "
        f"median of {rounds} calls per child, seconds")
    for name in names:
        med = {"parent": [], "this": []}
        for r in range(runs):
            for which in ("parent", "this"):
                env = dict(os.environ)
                env.pop("TCLIP_LIB", None)
                if which == "parent":
                    env["TCLIP_LIB"] = parent_lib
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(rounds)], env=env,
                                     stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True, timeout=900).stdout
                secs = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["seconds"]
                med[which].append(statistics.median(secs))
                say(f"   {name} run {r} {which:6s} {med[which][-1]:9.4f}   {['%.4f' % s for s in secs]}")
        mp, mt = statistics.median(med["parent"]), statistics.median(med["this"])
        spread = max(med["parent"]) - min(med["parent"])
        say(f"   {name}: medians parent {mp:.4f}, this {mt:.4f}: ratio {mt / mp:.5f} ({100 * (mt / mp - 1):+.3f} %); the parent's own "
            f"spread (max - min of its children): {spread:.4f} s ({100 * spread / mp:.3f} %)")


def opt_in(w, rounds):
    import torch
    from tclip_amd import engine, objective
    x_q, kw = tasks_and_kw(w)
    T, Q, K = x_q.shape
    plain = lambda: engine.run_em_dirichlet(x_q, **kw)              # noqa: E731
    seen = lambda: objective.run_em_dirichlet(x_q, **kw)            # noqa: E731
    say(f"{w['name']}: K = {K}, {kw['n_batches']} batches of {T // kw['n_batches']} tasks, iter = 20 x iter_mm = 1000")
    timed(plain)
    timed(seen)
    t = {"plain": [], "objective": []}
    for _ in range(rounds):
        ref, s = timed(plain)
        t["plain"].append(s)
        res, s = timed(seen)
        t["objective"].append(s)
    same = all(torch.equal(getattr(ref, k), getattr(res, k)) for k in engine.EMDirichletResult.__slots__)
    mp, mo = statistics.median(t["plain"]), statistics.median(t["objective"])
    traffic = 3.0 * T * Q * K * 4
    extra = (mo - mp) / kw["iters"]
    say(f"   2. the opt-in: plain {['%.4f' % v for v in t['plain']]} s, objective {['%.4f' % v for v in t['objective']]} s: ratio of the "
        f"medians {mo / mp:.5f}; shared outputs bit-identical: {same}")
    say(f"      extra per outer iteration {1e3 * extra:+.3f} ms of {1e3 * mp / kw['iters']:.1f} ms; traffic estimate {traffic / 1e9:.3f} GB = "
        f"{1e3 * traffic / HBM_BYTES_PER_S:.3f} ms at {HBM_BYTES_PER_S / 1e12:.0f} TB/s: measured / estimate = "
        f"{extra / (traffic / HBM_BYTES_PER_S):.1f}; the plain run's own spread {1e3 * (max(t['plain']) - min(t['plain'])):.1f} ms per call")
    obj = objective.objective(res.objective_terms, kw["lambd"])
    rises = int((obj[:, 1:] > obj[:, :-1]).sum())
    say(f"      objective, mean over the tasks, first / last iteration: {float(obj[:, 0].mean()):.6g} / {float(obj[:, -1].mean()):.6g}; "
        f"(task, iteration) pairs where it rises: {rises} of {obj[:, 1:].numel()}")
    del x_q
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", default=None, help="libtclip.so built from the parent commit: runs part 1")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_ab.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if args.child:
        return child(args.child, args.rounds)
    global OUT
    OUT = open(args.out, "w")
    say("EM-Dirichlet with the objective recorded: synthetic tasks (tclip_amd.synth, bench.py's), one MI355X")
    ws = workloads()
    if args.parent_lib:        # child processes, before this process opens the GPU
        default_path(os.path.abspath(args.parent_lib), list(ws), args.runs, args.rounds)
    for w in ws.values():
        opt_in(w, args.rounds)
    OUT.close()


if __name__ == "__main__":
    main()
