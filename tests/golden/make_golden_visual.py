#!/usr/bin/env python3
"""Golden vectors of the zero-shot SOFT_KMEANS, HARD_KMEANS, EM_GAUSSIAN and CLIP classes on VISUAL features
(use_softmax_feature == False), produced by RUNNING the reference (TCLIP_REFERENCE; imported, never copied; clip and
torchvision stubbed as in make_golden.py) on torch CPU with 8 threads.

The reference builds its text features with clip_weights(model, classnames, template, device) (src/utils.py:363-377), which
needs the CLIP model; the module-level name `clip_weights` of each method module is replaced (not edited) by a function that
returns seeded unit-norm text features (tests/helpers/visual.py).  u0, the responsibilities the reference's text-prompt
initialisation produces, is recorded by wrapping the first w_update call, so that the GPU loop can be pinned bit for bit from
the reference's own u0.

    python tests/golden/make_golden_visual.py            # loop fixtures vis_*, the lean case, evaluator fixtures eval_zs_vis_*
"""
import hashlib
import os
import random
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


METHODS = {"skm": ("soft_kmeans", "SOFT_KMEANS", 20), "hkm": ("hard_kmeans", "HARD_KMEANS", 10),
           "emg": ("em_gaussian", "EM_GAUSSIAN", 20)}
# name: (method key, D, K, N, seed)
CASES = {}
for _i, (_key, _) in enumerate(METHODS.items()):
    CASES[f"vis_{_key}_D512_K10_N3"] = (_key, 512, 10, 3, 3100 + 10 * _i)
    CASES[f"vis_{_key}_D1024_K37_N2"] = (_key, 1024, 37, 2, 3101 + 10 * _i)
    CASES[f"vis_{_key}_D768_K100_N1"] = (_key, 768, 100, 1, 3102 + 10 * _i)
LEAN = {"lean_vis_skm_D1024_K1000_N1": ("skm", 1024, 1000, 1, 3200)}
T_SCALE = 30.0


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def patch_text(mods, text):
    for m in mods:
        m.clip_weights = lambda model, classnames, template, device, _t=text: _t.clone().to(device)


def run_case(name, spec, lean=False):
    key, D, K, N, seed = spec
    module, cls_name, iters = METHODS[key]
    sys.path.insert(0, REF)
    mod = __import__(f"src.methods.zero_shot.{module}", fromlist=[cls_name])
    sys.path.pop(0)
    x_q, y_q, text = visual.make_tasks(N, K, D, seed)
    patch_text([mod], text)
    args = Args(iter=iters, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=T_SCALE, use_softmax_feature=False,
                graph_matching=True, classnames=[f"c{k}" for k in range(K)], template=["a photo of a {}."])
    cls = getattr(mod, cls_name)
    m = cls(model=None, device=torch.device("cpu"), log_file="/tmp/golden_visual.log", args=args)
    rec = {}
    orig = cls.w_update

    def w_update(self, query):
        if "u0" not in rec:
            rec["u0"] = self.u.clone()
        return orig(self, query)
    cls.w_update = w_update
    try:
        logs = m.run_task({"x_q": x_q.clone(), "y_q": y_q.clone().unsqueeze(2)})
    finally:
        cls.w_update = orig
    preds = m.u.argmax(2).int().numpy()
    out = {"method": module, "D": D, "K": K, "N": N, "seed": seed, "iters": iters, "T": T_SCALE, "inputs": "helpers.visual",
           "u0": rec["u0"].numpy(), "u": m.u.numpy(), "w": m.w.numpy(), "preds": preds,
           "criterions": np.asarray(logs["criterions"], np.float32), "acc": logs["acc"][:, -1].astype(np.float32),
           "lambd": int(getattr(m, "lambd", 0))}
    if key == "emg":
        out["v"] = m.v.numpy()
    if lean:
        out["x_q_sha1"] = sha(x_q.numpy())
        for k in ("u", "w", "v"):              # u0 stays: the loop starts from it
            if k in out:
                out[k + "_sha1"] = sha(out.pop(k))
    else:
        out["x_q"] = x_q.numpy()
        out["y_q"] = y_q.numpy()
        out["text"] = text.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "acc", out["acc"], "bytes", os.path.getsize(path), flush=True)


def run_eval(method, D=512, K=10, seed=3300):
    """Evaluator_zero_shot.evaluate_tasks on a seeded visual table, seeds as main.py:42-46 sets them; the index tensors the
    sampler yields are recorded."""
    sys.path.insert(0, REF)
    import src.eval_zero_shot as ez
    mods = [__import__(f"src.methods.zero_shot.{m}", fromlist=["x"]) for m in ("soft_kmeans", "hard_kmeans", "em_gaussian",
                                                                              "inductive_clip")]
    sys.path.pop(0)
    feats, labels, text = visual.make_table(K, D, 40, seed)
    patch_text(mods, text)
    n_tasks, bs = 20, 10
    iters = {"HARD_KMEANS": 10}.get(method, 20)
    args = Args(iter=iters, iter_mm=1000, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=T_SCALE, use_softmax_feature=False,
                graph_matching=True, shots=2, number_tasks=n_tasks, batch_size=bs, name_method=method, used_test_set="test",
                tunable=False, lambd=5.0, method=method.lower(), dataset="synthetic", classnames=[f"c{k}" for k in range(K)],
                template=["a photo of a {}."], backbone="RN50")
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    q = []
    orig = ez.SamplerQuery_zero_shot.__iter__

    def wrapped(self):
        for item in orig(self):
            q.append(item.clone())
            yield item
    ez.SamplerQuery_zero_shot.__iter__ = wrapped
    per_task = []
    real_ci = ez.compute_confidence_interval

    def recording_ci(data, *a, **k):
        per_task.append(np.asarray(data, np.float32).copy())
        return real_ci(data, *a, **k)
    ez.compute_confidence_interval = recording_ci
    try:
        ev = ez.Evaluator_zero_shot(device=torch.device("cpu"), args=args, log_file="/tmp/golden_visual_eval.log")
        acc, _ = ev.evaluate_tasks(None, feats, labels)
    finally:
        ez.compute_confidence_interval = real_ci
        ez.SamplerQuery_zero_shot.__iter__ = orig
    name = f"eval_zs_vis_{method.lower()}_D{D}_K{K}"
    out = {"method": method, "D": D, "K": K, "seed": seed, "rows_per_class": 40, "iters": iters, "T": T_SCALE,
           "number_tasks": n_tasks, "batch_size": bs, "inputs": "helpers.visual", "mean_accuracy": np.float64(acc),
           "task_accuracy": np.stack(per_task), "query_idx": torch.stack(q).numpy().reshape(n_tasks // bs, bs, 75)}
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
    for method in ("SOFT_KMEANS", "HARD_KMEANS", "EM_GAUSSIAN", "CLIP"):
        if not only or method in only:
            run_eval(method)


if __name__ == "__main__":
    main()
