#!/usr/bin/env python3
"""Golden vectors of the zero-shot EM_GAUSSIAN_COV class on VISUAL features (use_softmax_feature == False), produced by RUNNING
the reference (TCLIP_REFERENCE; imported, never copied; clip and torchvision stubbed, clip_weights replaced by seeded text
features as in make_golden_visual.py) on torch CPU with 8 threads.

u0, the responsibilities the text-prompt initialisation produces, is recorded by wrapping the first w_init call.  Each case
asserts that every output is finite; the cases named in NEED_DEAD that some cluster is empty (sum_q u <= eps) at the start of an
iteration >= 1 (checked by wrapping w_update), so that the keep-w-and-s path is exercised; and at least one case that s reaches
the sum_q u / eps clamp.  A seed that failed a condition would be replaced by the next one and recorded here: none did.

The full fixtures are full_vis_emgc_*: a name that began with vis_ would join the list of SOFT_KMEANS / HARD_KMEANS / EM_GAUSSIAN
fixtures tests/test_gpu_visual_kmeans.py builds from that prefix, and one without the _emgc_ tag the engine-level list of
conftest.golden_names().  A fixture that would exceed 1 MiB keeps w and s as sha1 digests (x_q, u0, u, v stay); the lean case keeps u, v, w, s as digests
and regenerates x_q from the seed.

    python tests/golden/make_golden_visual_cov.py
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import visual  # noqa: E402
sys.path.pop(0)
sys.path[:] = [p for p in sys.path if "transductive-clip_amd" not in p]

for _m in ("clip", "torchvision", "torchvision.transforms"):
    sys.modules.setdefault(_m, types.ModuleType(_m))
REF = os.environ.get("TCLIP_REFERENCE", "")      # a checkout of the reference, SegoleneMartin/transductive-CLIP
if not os.path.isdir(REF):
    sys.exit("set TCLIP_REFERENCE to a checkout of the reference (SegoleneMartin/transductive-CLIP)")


class Args(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


# name: (D, K, N, seed) - the seeds used; every one passed its conditions at the first try
CASES = {
    "full_vis_emgc_D512_K10_N3": (512, 10, 3, 3130),
    "full_vis_emgc_D1024_K37_N2": (1024, 37, 2, 3131),
    "full_vis_emgc_D768_K100_N1": (768, 100, 1, 3132),
    "full_vis_emgc_D5_K4_N2": (5, 4, 2, 3133),
}
LEAN = {"lean_vis_emc_D1024_K1000_N1": (1024, 1000, 1, 3230)}
NEED_DEAD = ("full_vis_emgc_D1024_K37_N2", "full_vis_emgc_D768_K100_N1")
ITERS = 20
T_SCALE = 30.0
EPS = 1e-15
MAX_BYTES = 1 << 20


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(name, spec, lean=False):
    D, K, N, seed = spec
    sys.path.insert(0, REF)
    mod = __import__("src.methods.zero_shot.em_gaussian_cov", fromlist=["EM_GAUSSIAN_COV"])
    sys.path.pop(0)
    x_q, y_q, text = visual.make_tasks(N, K, D, seed)
    mod.clip_weights = lambda model, classnames, template, device, _t=text: _t.clone().to(device)
    args = Args(iter=ITERS, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=T_SCALE, use_softmax_feature=False,
                graph_matching=True, classnames=[f"c{k}" for k in range(K)], template=["a photo of a {}."])
    cls = mod.EM_GAUSSIAN_COV
    m = cls(model=None, device=torch.device("cpu"), log_file="/tmp/golden_visual_cov.log", args=args)
    rec = {"updates": 0, "dead": 0}
    orig_init, orig_update = cls.w_init, cls.w_update

    def w_init(self, query):
        if "u0" not in rec:
            rec["u0"] = self.u.clone()
        return orig_init(self, query)

    def w_update(self, query):
        if rec["updates"] >= 1:
            rec["dead"] = max(rec["dead"], int((self.u.sum(1) <= EPS).sum()))
        rec["updates"] += 1
        return orig_update(self, query)
    cls.w_init, cls.w_update = w_init, w_update
    try:
        logs = m.run_task({"x_q": x_q.clone(), "y_q": y_q.clone().unsqueeze(2)})
    finally:
        cls.w_init, cls.w_update = orig_init, orig_update
    for k in ("u", "v", "w", "s"):
        assert torch.isfinite(getattr(m, k)).all(), (name, k, "not finite")
    assert rec["updates"] == ITERS
    if name in NEED_DEAD:
        assert rec["dead"] > 0, (name, "no empty cluster at the start of an iteration >= 1: take the next seed")
    preds = m.u.argmax(2).int().numpy()
    out = {"method": "em_gaussian_cov", "D": D, "K": K, "N": N, "seed": seed, "iters": ITERS, "T": T_SCALE,
           "inputs": "helpers.visual", "u0": rec["u0"].numpy(), "u": m.u.numpy(), "v": m.v.numpy(), "w": m.w.numpy(),
           "s": m.s.numpy(), "preds": preds, "acc": logs["acc"][:, -1].astype(np.float32), "lambd": int(m.lambd),
           "dead_clusters": rec["dead"], "s_max": np.float32(m.s.max())}
    if lean:
        out["x_q_sha1"] = sha(x_q.numpy())
        for k in ("u", "v", "w", "s"):         # u0 stays: the loop starts from it
            out[k + "_sha1"] = sha(out.pop(k))
    else:
        out["x_q"] = x_q.numpy()
        out["y_q"] = y_q.numpy()
        out["text"] = text.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    if not lean and os.path.getsize(path) > MAX_BYTES:
        for k in ("w", "s"):
            out[k + "_sha1"] = sha(out.pop(k))
        np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
    print(name, "acc", out["acc"], "dead", rec["dead"], "s_max", out["s_max"], "digests", sorted(k for k in out if k.endswith("_sha1")),
          "bytes", os.path.getsize(path), flush=True)
    return float(out["s_max"])


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    only = set(sys.argv[1:])
    s_max = []
    for name, spec in CASES.items():
        if not only or name in only:
            s_max.append(run_case(name, spec))
    for name, spec in LEAN.items():
        if not only or name in only:
            s_max.append(run_case(name, spec, lean=True))
    if not only:      # sum_q u / eps with sum_q u of order 1 .. 75
        assert max(s_max) >= 1e14, "no case has s at the sum u / eps clamp"


if __name__ == "__main__":
    main()
