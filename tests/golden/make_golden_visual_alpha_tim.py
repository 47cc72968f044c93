#!/usr/bin/env python3
"""Golden vectors for ALPHA_TIM on VISUAL features (rows of D elements, D independent of the class count; reference:
src/methods/few_shot/tim.py:192-322, which never reads use_softmax_feature and normalises nothing) from the REFERENCE's own
class, CPU autograd + torch.optim.Adam with at most 8 torch threads, on the seeded unit-norm class-mean-plus-noise embeddings
of tests/helpers/visual_fs.py.  Needs a checkout of the reference (TCLIP_REFERENCE; imported, never copied; clip and
torchvision stubbed); the .npz files are committed.

    python tests/golden/make_golden_visual_alpha_tim.py

Every case runs the reference's class twice on the same inputs: as it is (fp32), and with inputs, weights and the whole loop in
fp64 (a subclass whose run_task takes the `.double()` variant the reference keeps commented in place, and a double one-hot; both
exist in this process only - the device of make_golden_tim_gd.py).  There is no bit-level target for an implementation with
another operation order, so each fixture carries its own bounds, derived from the reference alone (floors and rationale:
DESIGN.md section 8d):

    weights_abs    = max(1e-6, 2 * max|weights - weights64|)
    logits_abs     = max(2e-5, 2 * max|logits_q - logits_q64|)
    criterions_rel = max(1e-5, 2 * max|criterions / criterions64 - 1|)

The reference's fp32 run and another fp32 implementation are two roundings of the same fp64 trajectory; each may sit one such
gap away from it, on opposite sides: hence the factor 2.  A seed is accepted only if every query's gap between its largest and
second-largest fp64 logit exceeds 4 * logits_abs, so that predictions and accuracies have to be EQUAL to the reference's; seeds
are tried in order from the first one and `seeds_tried` records how many.

Each file: y_s, y_q and the SHA-1 of x_s / x_q (helpers.visual_fs.make_tasks regenerates the inputs from D, K, shots, N, seed,
signal); weights, logits_q, criterions (iter,), acc of the fp32 run; weights64_minus_weights (fp32, to stay under the size
limit), logits_q64, criterions64; the three bounds and the gaps they come from, min_logit_margin, the parameters and
torch_version."""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TCLIP_REFERENCE", "")      # a checkout of the reference, SegoleneMartin/transductive-CLIP
if not os.path.isdir(REF):
    sys.exit("set TCLIP_REFERENCE to a checkout of the reference (SegoleneMartin/transductive-CLIP)")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import visual_fs  # noqa: E402
sys.path.pop(0)
sys.path[:] = [p for p in sys.path if "transductive-clip_amd" not in p]
for _m in ("clip", "torchvision", "torchvision.transforms"):      # absent from this image, unused on this path
    sys.modules.setdefault(_m, types.ModuleType(_m))


class Args(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


DEFAULT = ("Shannon", "Alpha", "Alpha")      # alpha_tim.yaml
# name -> (D, K, shots, N, first seed, signal, iters, alpha_value, entropies, loss_weights, temp, lr); step counts and learning
# rates follow the fs_vis_gd_tim_* fixtures
CASES = {
    "fs_vis_alpha_tim_D512_K10_S4_N3": (512, 10, 4, 3, 7100, 0.2, 100, 7.0, DEFAULT, (1.0, 1.0, 1.0), 15, 1e-4),
    "fs_vis_alpha_tim_D1024_K37_S2_N2": (1024, 37, 2, 2, 7101, 0.25, 60, 2.0, ("Shannon", "Shannon", "Shannon"), (1.0, 1.0, 1.0), 15, 1e-3),
    "fs_vis_alpha_tim_D768_K100_S1_N1": (768, 100, 1, 1, 7102, 0.35, 40, 7.0, DEFAULT, (1.0, 1.0, 1.0), 15, 1e-4),
}


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_reference(mod, double, args, task, shots):
    """the reference's ALPHA_TIM on one task dictionary -> (weights, last logits_q, criterions (iter,), acc)"""
    model = types.SimpleNamespace(eval=lambda: None, train=lambda: None)       # the class only toggles its mode

    class ALPHA_TIM64(mod.ALPHA_TIM):
        def run_task(self, task_dic, shot=10):       # BASE.run_task with its commented `.double()` taken
            support = task_dic['x_s'].to(self.device).double()
            query = task_dic['x_q'].to(self.device).double()
            y_s = task_dic['y_s'].long().squeeze(2).to(self.device)
            y_q = task_dic['y_q'].long().squeeze(2).to(self.device)
            self.run_method(support=support, query=query, y_s=y_s, y_q=y_q)
            return self.get_logs()

    one_hot = mod.get_one_hot
    if double:
        mod.get_one_hot = lambda y, n: one_hot(y, n).double()
    try:
        m = (ALPHA_TIM64 if double else mod.ALPHA_TIM)(model=model, device=torch.device("cpu"), log_file="/tmp/golden_vis_alpha_tim.log", args=args)
        seen = {}
        real_acc = m.compute_acc

        def acc(y_q, logits_q):
            seen["logits_q"] = logits_q.detach().clone()
            return real_acc(y_q=y_q, logits_q=logits_q)
        m.compute_acc = acc
        logs = m.run_task(task_dic={k: v.clone() for k, v in task.items()}, shot=shots)
    finally:
        mod.get_one_hot = one_hot
    assert m.weights.dtype == (torch.float64 if double else torch.float32)
    return m.weights.detach().numpy(), seen["logits_q"].numpy(), np.asarray(logs["criterions"]), np.asarray(logs["acc"], np.float32)


def make(mod, name, D, K, shots, N, seed0, signal, iters, alpha, ent, lw, temp, lr):
    for tried, seed in enumerate(range(seed0, seed0 + 20), 1):
        x_s, y_s, x_q, y_q = visual_fs.make_tasks(N, K, D, shots, seed, signal=signal)
        task = {"x_s": x_s, "y_s": y_s.unsqueeze(2), "x_q": x_q, "y_q": y_q.unsqueeze(2)}
        args = Args(iter=iters, loss_weights=list(lw), temp=temp, lr_alpha_tim=lr, entropies=list(ent), alpha_value=alpha,
                    num_classes_test=K, n_class=K, T=30)
        w, lq, crit, acc = run_reference(mod, False, args, task, shots)
        w64, lq64, crit64, acc64 = run_reference(mod, True, args, task, shots)
        gaps = (float(np.abs(w - w64).max()), float(np.abs(lq - lq64).max()), float(np.abs(crit / crit64 - 1).max()))
        bounds = (max(1e-6, 2 * gaps[0]), max(2e-5, 2 * gaps[1]), max(1e-5, 2 * gaps[2]))
        top2 = np.sort(lq64, axis=2)[:, :, -2:]
        margin = float((top2[:, :, 1] - top2[:, :, 0]).min())
        print(f"{name} seed {seed}: fp32-fp64 gaps weights {gaps[0]:.3e} logits {gaps[1]:.3e} criterions(rel) {gaps[2]:.3e}; "
              f"smallest top-2 logit margin {margin:.3e} (needs > {4 * bounds[1]:.3e})", flush=True)
        if margin > 4 * bounds[1]:
            break
    else:
        sys.exit(f"{name}: no seed with a sufficient logit margin")
    assert np.array_equal(lq.argmax(2), lq64.argmax(2)) and np.array_equal(acc, acc64)
    assert crit.shape == (iters,) and acc.shape == (N, 1) and w.shape == (N, K, D)
    out = {"D": D, "K": K, "N": N, "shots": shots, "seed": seed, "signal": signal, "seeds_tried": tried, "iters": iters,
           "alpha_value": alpha, "entropies": np.array(ent), "loss_weights": np.asarray(lw, np.float64), "temp": temp, "lr": lr,
           "inputs": "helpers.visual_fs", "y_s": y_s.numpy(), "y_q": y_q.numpy(), "x_s_sha1": sha(x_s.numpy()),
           "x_q_sha1": sha(x_q.numpy()), "y_s_sha1": sha(y_s.numpy()), "y_q_sha1": sha(y_q.numpy()),
           "weights": w, "logits_q": lq, "criterions": crit.astype(np.float32), "acc": acc,
           "weights64_minus_weights": (w64 - w.astype(np.float64)).astype(np.float32), "logits_q64": lq64,
           "criterions64": crit64.astype(np.float64),
           "weights_abs": np.float64(bounds[0]), "logits_abs": np.float64(bounds[1]), "criterions_rel": np.float64(bounds[2]),
           "weights_gap": np.float64(gaps[0]), "logits_gap": np.float64(gaps[1]), "criterions_gap": np.float64(gaps[2]),
           "min_logit_margin": np.float64(margin), "torch_version": torch.__version__}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: acc={acc.ravel().round(3).tolist()} crit[0,-1]={crit[[0, -1]].tolist()} bounds={bounds} seeds tried {tried} "
          f"-> {os.path.getsize(path) / 1e3:.0f} kB", flush=True)
    assert os.path.getsize(path) < 1 << 20


def main():
    sys.path.insert(0, REF)
    import src.methods.few_shot.tim as mod
    sys.path.pop(0)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for name in (sys.argv[1:] or list(CASES)):
        make(mod, name, *CASES[name])


if __name__ == "__main__":
    main()
