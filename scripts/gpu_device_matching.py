#!/usr/bin/env python3
"""Accuracy tail with the matching on the host against the matching on the device (engine.clustering_accuracy, matching="host" /
"device") at the three bench shapes, predictions from a SOFT_KMEANS run so that the cluster counts are the workload's.
Warm-up, best of several, the device synchronised around the timed region, the two paths alternated; the results of both
are compared bit for bit first.  `--one K T` runs the device path of one shape a few times and nothing else (for a kernel
trace).  Prints the host's load average and tclip_host_threads()."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from tclip_amd import _capi, engine, synth  # noqa: E402

SHAPES = [(100, 1000), (397, 1000), (1000, 1250)]


def inputs(K, T):
    x_q, y_q = synth.make_query_tasks(T, K, seed=3)
    x, y = x_q.cuda(), y_q.squeeze(2).cuda()
    preds = engine.run_soft_kmeans(x, iters=20, temperature=30)[-1]
    torch.cuda.synchronize()
    return x, y, preds


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        K, T = int(sys.argv[2]), int(sys.argv[3])
        x, y, preds = inputs(K, T)
        for _ in range(5):
            engine.clustering_accuracy(x, preds, y, matching="device")
        torch.cuda.synchronize()
        return
    print(f"load average {os.getloadavg()}  tclip_host_threads {_capi.lib().tclip_host_threads()}  "
          f"cpus of this process {len(os.sched_getaffinity(0))}", flush=True)
    for K, T in SHAPES:
        x, y, preds = inputs(K, T)
        host = lambda: engine.clustering_accuracy(x, preds, y)  # noqa: E731
        dev = lambda: engine.clustering_accuracy(x, preds, y, matching="device")  # noqa: E731
        acc_h, new_h = host()
        acc_d, new_d = dev()
        same = torch.equal(acc_d.cpu(), acc_h) and torch.equal(new_d.cpu(), new_h)
        clusters = torch.stack([torch.tensor(len(torch.unique(p))) for p in preds.cpu()]).float()
        for fn in (host, dev):
            timed(fn)
        best_h = best_d = 1e9
        for _ in range(7):
            best_h = min(best_h, timed(host))
            best_d = min(best_d, timed(dev))
        # the device path's result on the host, as get_logs fetches it
        best_dl = min(timed(lambda: engine.match_status_ok(dev()[0])) for _ in range(5))
        print(f"K={K} tasks={T} clusters/task mean {clusters.mean():.1f} max {int(clusters.max())}  bit-equal {same}  "
              f"tail host {best_h:.2f} ms  device {best_d:.2f} ms  device + acc to host {best_dl:.2f} ms  "
              f"mean acc {float(acc_h.mean()):.4f}", flush=True)
        assert same
    print(f"load average after {os.getloadavg()}", flush=True)


if __name__ == "__main__":
    main()
