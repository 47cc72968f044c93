#!/usr/bin/env python3
"""TIM_GD on the GPU: deviations from the reference fixtures next to the bounds they carry, and timings of run_tim_gd at
D = K and D != K alongside ALPHA_TIM at the D = K shape (best of 3 calls after a warm-up, device synchronised around each).

    python scripts/gpu_tim_gd_check.py            # fixtures + the timing table
    python scripts/gpu_tim_gd_check.py one K D shots tasks iters     # one warm-up and one timed call of a single shape (for a profiler)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from helpers import tim_gd, visual_fs  # noqa: E402
from tclip_amd import engine, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def inputs(K, D, shots, N):
    if D == K:
        x_q, _ = synth.make_query_tasks(N, K, seed=5, k_eff=5)
        x_s, y_s = synth.make_support(N, K, shots, seed=5)
        return x_q.cuda(), x_s.cuda(), y_s.squeeze(2).cuda()
    x_s, y_s, x_q, _ = visual_fs.make_tasks(N, K, D, shots, 5, signal=0.3)
    return x_q.cuda(), x_s.cuda(), y_s.cuda()


def timed(fn, calls=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.time() - t0)
    return best


def main():
    if sys.argv[1:2] == ["one"]:
        K, D, shots, N, iters = (int(v) for v in sys.argv[2:7])
        x_q, x_s, y_s = inputs(K, D, shots, N)
        dt = timed(lambda: engine.run_tim_gd(x_q, x_s, y_s, n_class=K, iters=iters, temp=15.0, lr=1e-4), calls=1)
        print(f"TIM_GD K={K} D={D} shots={shots} N={N} iters={iters}: {dt:.3f} s")
        return
    for name in tim_gd.PROB + tim_gd.VISUAL:
        g = tim_gd.load_fixture(GOLDEN, name)
        w, lq, preds, crit = engine.run_tim_gd(torch.from_numpy(g["x_q"]).cuda(), torch.from_numpy(g["x_s"]).cuda(),
                                               torch.from_numpy(g["y_s"]).squeeze(2).cuda(), n_class=int(g["K"]), **tim_gd.params(g))
        torch.cuda.synchronize()
        acc = (preds.cpu().long() == torch.from_numpy(g["y_q"]).squeeze(2)).float().mean(1)
        print(f"{name:32s} max|dW| {np.abs(w.cpu().numpy() - g['weights']).max():.2e} (bound {float(g['weights_abs']):.2e})  "
              f"max|dlogit| {np.abs(lq.cpu().numpy() - g['logits_q']).max():.2e} (bound {float(g['logits_abs']):.2e})  "
              f"crit rel {np.abs(crit.cpu().numpy() / g['criterions'] - 1).max():.2e} (bound {float(g['criterions_rel']):.2e})  "
              f"pred mismatches {(preds.cpu().numpy() != g['logits_q'].argmax(2)).sum()}  "
              f"acc equal {np.array_equal(acc.numpy(), g['acc'][:, 0])}", flush=True)
    for K, D, shots, N, iters in ((100, 100, 4, 100, 1000), (100, 512, 4, 100, 1000), (397, 1024, 4, 20, 1000), (1000, 1024, 4, 4, 1000)):
        x_q, x_s, y_s = inputs(K, D, shots, N)
        dt = timed(lambda: engine.run_tim_gd(x_q, x_s, y_s, n_class=K, iters=iters, temp=15.0, lr=1e-4))
        flop = 4.0 * N * (K * shots + 75) * K * D * iters
        print(f"TIM_GD    K={K} D={D} shots={shots} N={N} iters={iters}: {dt:.3f} s  ({N / dt:.1f} tasks/s, "
              f"{flop / dt / 1e12:.2f} TFLOP/s fp32 in the two GEMMs)", flush=True)
        if D == K:
            dt = timed(lambda: engine.run_alpha_tim(x_q, x_s, y_s, iters=iters, temp=15.0, lr=1e-4, alpha_value=7.0))
            print(f"ALPHA_TIM K={K} D={D} shots={shots} N={N} iters={iters}: {dt:.3f} s  ({N / dt:.1f} tasks/s, "
                  f"{flop / dt / 1e12:.2f} TFLOP/s fp32 in the two GEMMs)", flush=True)


if __name__ == "__main__":
    main()
