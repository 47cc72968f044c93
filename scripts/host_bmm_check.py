#!/usr/bin/env python3
"""Does this host's torch evaluate KL_KMEANS's centroid product u^T z the way the fixture host did?  There MKL's sgemm sums
every output as one chain of fused multiply-adds over the query rows in ascending order (below 400 multiply-adds per matrix
ATen's own loop: rounded product plus add) - what k_kl_centroids and tests/helpers/restated.py:restated_bmm restate.  MKL picks
its kernel by the CPU, so on another host some shapes differ; this prints them.  Run from the repository root; no GPU."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers.restated import restated_bmm      # noqa: E402

torch.set_num_threads(min(8, torch.get_num_threads()))
bmm = restated_bmm()
gen = torch.Generator().manual_seed(1)
for K in (2, 3, 5, 7, 8, 9, 12, 16, 17, 24, 40, 100, 397, 1000):
    differ = []
    for Q in list(range(1, 140)) + [200, 256, 300]:
        z = (3 * torch.randn(2, Q, K, generator=gen)).softmax(-1)
        hot = torch.zeros_like(z).scatter_(2, z.argmax(2, keepdim=True), 1.0)
        if not all(torch.equal(u.transpose(1, 2) @ z, bmm(u.transpose(1, 2), z)) for u in (z, hot)):
            differ.append(Q)
    print(f"K = {K}: torch's bmm differs from the chain at Q = {differ}" if differ else f"K = {K}: the chain at every Q", flush=True)
