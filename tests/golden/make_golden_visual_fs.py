#!/usr/bin/env python3
"""Golden vectors of the few-shot PADDLE and BDCSPN classes on VISUAL features (use_softmax_feature == False), produced by
RUNNING the reference (TCLIP_REFERENCE; imported, never copied; clip and torchvision stubbed as in make_golden_visual.py) on
torch CPU with at most 8 threads (tests/conftest.py explains the thread count).

The reference's PADDLE calls clip_weights(model, classnames, template, device) on visual features (paddle.py:189-190), which
needs the CLIP model; the `paddle` module's name `clip_weights` is replaced (not edited) by a function that returns seeded
unit-norm text features (tests/helpers/visual.py).  The u built from them is overwritten by the first u_update before anything
reads it, so the results do not depend on the text features.

Inputs come from tests/helpers/visual_fs.py: the support set is every class x `shots` rows in class order with the labels
unchanged (visual features are not relabelled).  `signal` per case is chosen so that the accuracies lie strictly between 0 and
1, and PADDLE's lambd is non-zero in all but one case so that the v term acts.

    python tests/golden/make_golden_visual_fs.py          # fs_vis_{paddle,bdcspn}_*, the lean cases, eval_fs_vis_*

The method-level names start with fs_vis_ (not vis_fs_): tests/test_gpu_visual_kmeans.py takes every file that starts with
vis_ for a zero-shot k-means fixture.
"""
import os
import random
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import visual, visual_fs  # noqa: E402
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


# name: (method, D, K, shots, N, seed, signal, parameter (PADDLE: lambd; BDCSPN: temp), norm_type)
CASES = {
    "fs_vis_paddle_D512_K10_S4_N3": ("paddle", 512, 10, 4, 3, 4100, 0.2, 5.0, None),
    "fs_vis_paddle_D1024_K37_S2_N2": ("paddle", 1024, 37, 2, 2, 4101, 0.25, 20.0, None),
    "fs_vis_paddle_D768_K100_S1_N1": ("paddle", 768, 100, 1, 1, 4102, 0.35, 0.0, None),
    "fs_vis_bdcspn_D512_K10_S4_N3": ("bdcspn", 512, 10, 4, 3, 4110, 0.2, 15.0, "L2N"),
    "fs_vis_bdcspn_D1024_K37_S2_N2": ("bdcspn", 1024, 37, 2, 2, 4111, 0.25, 15.0, "CL2N"),
    "fs_vis_bdcspn_D768_K100_S1_N1": ("bdcspn", 768, 100, 1, 1, 4112, 0.35, 30.0, "UN"),
}
LEAN = {
    "lean_fs_vis_paddle_D1024_K1000_S1_N1": ("paddle", 1024, 1000, 1, 1, 4200, 0.3, 5.0, None),
    "lean_fs_vis_bdcspn_D1024_K1000_S1_N1": ("bdcspn", 1024, 1000, 1, 1, 4210, 0.3, 15.0, "L2N"),
}
PADDLE_ITERS = 20


def load(module):
    sys.path.insert(0, REF)
    mod = __import__(f"src.methods.few_shot.{module}", fromlist=["x"])
    sys.path.pop(0)
    return mod


def run_case(name, spec, lean=False):
    method, D, K, shots, N, seed, signal, param, norm_type = spec
    x_s, y_s, x_q, y_q = visual_fs.make_tasks(N, K, D, shots, seed, signal=signal)
    task = {"x_s": x_s.clone(), "x_q": x_q.clone(), "y_s": y_s.clone().unsqueeze(2), "y_q": y_q.clone().unsqueeze(2)}
    args = Args(iter=PADDLE_ITERS, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=False,
                classnames=[f"c{k}" for k in range(K)], template=["a photo of a {}."], lambd=param, temp=param,
                norm_type=norm_type)
    out = {"method": method, "D": D, "K": K, "N": N, "shots": shots, "seed": seed, "signal": signal,
           "inputs": "helpers.visual_fs"}
    if method == "paddle":
        mod = load("paddle")
        text = visual.make_text(K, D, seed)
        mod.clip_weights = lambda model, classnames, template, device, _t=text: _t.clone().to(device)
        m = mod.PADDLE(model=None, device=torch.device("cpu"), log_file="/tmp/golden_visual_fs.log", args=args)
        t0 = time.time()
        logs = m.run_task(task, shots)
        seconds = time.time() - t0
        assert float(np.abs(logs["criterions"]).max()) == 0.0
        arrays = {"u": m.u.numpy(), "v": m.v.numpy(), "w": m.w.numpy()}
        out.update(iters=PADDLE_ITERS, lambd=np.float32(param), preds=m.u.argmax(2).int().numpy())
        u = m.u
    else:
        mod = load("bdcspn")
        rec = {}
        orig = mod.BDCSPN.proto_rectification

        def proto_rectification(self, **kw):
            rec["prototypes"] = orig(self, **kw)
            return rec["prototypes"]
        orig_logits = mod.BDCSPN.get_logits

        def get_logits(self, w, samples):
            r = orig_logits(self, w, samples)
            if w.dim() == 3:                      # the prediction call of run_method (:190-191)
                rec["u"] = (self.temp * r).softmax(-1)
            return r
        mod.BDCSPN.proto_rectification, mod.BDCSPN.get_logits = proto_rectification, get_logits
        try:
            m = mod.BDCSPN(model=None, device=torch.device("cpu"), log_file="/tmp/golden_visual_fs.log", args=args)
            t0 = time.time()
            logs = m.run_task(task, shots)
            seconds = time.time() - t0
        finally:
            mod.BDCSPN.proto_rectification, mod.BDCSPN.get_logits = orig, orig_logits
        u = rec["u"]
        arrays = {"prototypes": rec["prototypes"].numpy(), "u": u.numpy()}
        out.update(temp=np.float32(param), norm_type=norm_type, preds=u.argmax(2).int().numpy())
    out["acc"] = logs["acc"][:, -1].astype(np.float32)
    out["reference_seconds_per_task"] = np.float64(seconds / N)
    interior = int(((u > 1e-6) & (u < 1 - 1e-6)).sum())
    assert interior > 0 and any(0.0 < a < 1.0 for a in out["acc"]), (name, out["acc"], interior)
    for k, a in (("x_s", x_s), ("x_q", x_q), ("y_s", y_s), ("y_q", y_q)):
        out[k + "_sha1"] = visual_fs.sha(a.numpy())
    if lean:
        for k, a in arrays.items():
            out[k + "_sha1"] = visual_fs.sha(a)
    else:
        out.update(arrays)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "acc", out["acc"], "interior u", interior, "s/task", round(seconds / N, 2), "bytes", os.path.getsize(path),
          flush=True)


def run_eval(method, D=512, K=10, seed=4300, signal=0.2):
    """Evaluator_few_shot.evaluate_tasks on seeded visual tables, seeds as main.py:42-46 sets them; the index tensors the
    samplers yield are recorded."""
    sys.path.insert(0, REF)
    import src.eval_few_shot as ef
    mod = __import__("src.methods.few_shot.paddle", fromlist=["x"])
    sys.path.pop(0)
    feats_s, labels_s, feats_q, labels_q = visual_fs.make_tables(K, D, 40, seed, signal=signal)
    text = visual.make_text(K, D, seed)
    mod.clip_weights = lambda model, classnames, template, device, _t=text: _t.clone().to(device)
    n_tasks, bs, shots = 20, 10, 2
    args = Args(iter=PADDLE_ITERS, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=False,
                shots=shots, number_tasks=n_tasks, batch_size=bs, name_method=method, used_test_set="test", tunable=False,
                lambd=5.0, temp=15.0, norm_type="L2N", method=method.lower(), dataset="synthetic",
                classnames=[f"c{k}" for k in range(K)], template=["a photo of a {}."], backbone="RN50")
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    q, s = [], []

    def record(cls, sink):
        orig = cls.__iter__

        def wrapped(self):
            for item in orig(self):
                sink.append(item.clone())
                yield item
        cls.__iter__ = wrapped
        return orig
    oq, os_ = record(ef.SamplerQuery_few_shot, q), record(ef.SamplerSupport_few_shot, s)
    per_task = []
    real_ci = ef.compute_confidence_interval

    def recording_ci(data, *a, **k):
        per_task.append(np.asarray(data, np.float32).copy())
        return real_ci(data, *a, **k)
    ef.compute_confidence_interval = recording_ci
    try:
        ev = ef.Evaluator_few_shot(device=torch.device("cpu"), args=args, log_file="/tmp/golden_visual_fs_eval.log")
        acc, _ = ev.evaluate_tasks(None, feats_s, labels_s, feats_q, labels_q)
    finally:
        ef.compute_confidence_interval = real_ci
        ef.SamplerQuery_few_shot.__iter__, ef.SamplerSupport_few_shot.__iter__ = oq, os_
    name = f"eval_fs_vis_{method.lower()}_D{D}_K{K}"
    out = {"method": method, "D": D, "K": K, "seed": seed, "signal": signal, "rows_per_class": 40, "shots": shots,
           "iters": PADDLE_ITERS, "lambd": np.float32(5.0), "temp": np.float32(15.0), "norm_type": "L2N", "number_tasks": n_tasks,
           "batch_size": bs, "inputs": "helpers.visual_fs", "mean_accuracy": np.float64(acc), "task_accuracy": np.stack(per_task),
           "query_idx": torch.stack(q).numpy().reshape(n_tasks // bs, bs, 75),
           "support_idx": torch.stack(s).numpy().reshape(n_tasks // bs, bs, K * shots)}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "acc", acc, flush=True)


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    only = set(sys.argv[1:])
    for name, spec in CASES.items():
        if not only or name in only:
            run_case(name, spec)
    for name, spec in LEAN.items():
        if not only or name in only:
            run_case(name, spec, lean=True)
    for method in ("PADDLE", "BDCSPN"):
        if not only or method in only:
            run_eval(method)


if __name__ == "__main__":
    main()
