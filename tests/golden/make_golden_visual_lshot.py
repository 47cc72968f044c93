#!/usr/bin/env python3
"""Golden vectors for LAPLACIAN_SHOT on VISUAL features (rows of D elements, D independent of the class count) from the
REFERENCE's own class (src/methods/few_shot/laplacian_shot.py; it never reads use_softmax_feature), CPU (numpy / scipy.sparse /
sklearn kNN), on the seeded unit-norm class-mean-plus-noise embeddings of tests/helpers/visual_fs.py.  Needs a checkout of the
reference (TCLIP_REFERENCE; imported and wrapped, never copied; clip and torchvision stubbed, the removed alias `np.float`
restored for this process and matplotlib stubbed when absent, as in make_golden_lshot.py); the .npz files are committed.

    python tests/golden/make_golden_visual_lshot.py

Every case runs the reference's class twice on the same inputs: as it is (float32 tensors in), and with float64 tensors in
(the class converts nothing, so normalisation, prototypes, distances and the kNN search then run in double).  There is no
bit-level target for an implementation with another operation order, so each fixture carries its own bounds, derived from the
reference alone (gap = the fp32 run's deviation from the fp64 run):

    unary_rel  = max(1e-6, 2 * max|unary / unary64 - 1|)
    energy_rel = max(1e-7, 2 * max|ent_energy / ent_energy64 - 1|)

The fp32 run and another fp32 implementation are two roundings of the same fp64 computation; each may sit one such gap away
from it, on opposite sides: hence the factor 2.  The floors are the orders of tests/golden/f4_tolerances.json's entries.
A seed is accepted only if the reference alone satisfies two conditions, so that everything discrete has to be EQUAL to the
reference's (neighbour lists, every per-update assignment and accuracy):
  - the fp32 and the fp64 run give identical neighbour lists, per-update assignments and freeze iteration;
  - for every query the fp64 squared distances to its (knn-1)-th and knn-th nearest OTHER query differ by more than 1e-6
    relative (the stored knn_margin is the smallest such difference).
Seeds are tried in order from the first one; `seeds_tried` records how many.

Each file: y_s, y_q and the SHA-1 of x_s / x_q / y_s / y_q (helpers.visual_fs.make_tasks regenerates the inputs from D, K, shots,
N, seed, signal); of the fp32 run the sorted kNN lists, unary, the assignment after every update (N, iter, Q), per-update
accuracies (N, iter) and bound energies (N, iter); unary64_minus_unary (fp32), ent_energy64; the two bounds, knn_margin, the
equality flags, freeze_iter (N,) and the parameters."""
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
try:
    import matplotlib  # noqa: F401
except ImportError:
    _mpl = types.ModuleType("matplotlib")
    _mpl.use = lambda *a, **k: None
    sys.modules["matplotlib"] = _mpl
if not hasattr(np, "float"):
    np.float = float


class Args(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


# name: (D, K, shots, N, first seed, signal, knn, lmd, norm_type, iters)
CASES = {
    "fs_vis_lshot_D512_K10_S4_N3": (512, 10, 4, 3, 6100, 0.2, 3, 0.7, "L2N", 20),
    "fs_vis_lshot_D1024_K37_S2_N2": (1024, 37, 2, 2, 6101, 0.25, 7, 0.3, "L2N", 12),
    "fs_vis_lshot_D768_K100_S1_N1_un": (768, 100, 1, 1, 6102, 0.35, 5, 1.5, "UN", 20),
}


def run_reference(mod, double, args, task, shots):
    """the reference's LAPLACIAN_SHOT on one task dictionary -> dict of what it computed, per task"""
    one_hot = mod.get_one_hot
    if double:                                       # the class multiplies the one-hot labels with the support rows
        mod.get_one_hot = lambda y, n: one_hot(y, n).double()
    try:
        return _run_reference(mod.LAPLACIAN_SHOT, double, args, task, shots)
    finally:
        mod.get_one_hot = one_hot


def _run_reference(cls, double, args, task, shots):
    m = cls(model=None, device=torch.device("cpu"), log_file="/tmp/golden_vis_lshot.log", args=args)
    seen = {"knn": [], "unary": [], "preds_iter": [], "query": []}
    real_aff, real_bound = m.create_affinity, m.bound_update

    def aff(X):
        assert X.dtype == (np.float64 if double else np.float32)
        seen["query"].append(np.asarray(X, np.float64))
        W = real_aff(X)
        dense = W.toarray()
        seen["knn"].append(np.stack([np.sort(np.nonzero(dense[i])[0]) for i in range(dense.shape[0])]))
        return W

    def bound(**kw):
        seen["unary"].append(np.asarray(kw["unary"]).copy())
        real_stack = torch.stack
        calls = []

        def stack(tensors, dim=0):                   # bound_update stacks its per-update assignments first, then the hits
            calls.append([t.clone() for t in tensors])
            return real_stack(tensors, dim=dim)
        torch.stack = stack
        try:
            out = real_bound(**kw)
        finally:
            torch.stack = real_stack
        seen["preds_iter"].append(real_stack(calls[0]).numpy())
        return out
    m.create_affinity, m.bound_update = aff, bound
    cast = (lambda t: t.double()) if double else (lambda t: t.float())
    logs = m.run_task(task_dic={"x_s": cast(task["x_s"].clone()), "y_s": task["y_s"].clone(), "x_q": cast(task["x_q"].clone()),
                                "y_q": task["y_q"].clone()}, shot=shots)
    energy = np.asarray(logs["ent_energy"], np.float64)
    return {"neighbours": np.stack(seen["knn"]).astype(np.int32), "unary": np.stack(seen["unary"]),
            "preds_iter": np.stack(seen["preds_iter"]).astype(np.int32), "acc": np.asarray(logs["acc"], np.float32),
            "ent_energy": energy, "query": np.stack(seen["query"])}


def freeze_iter(energy):
    """per task the update after which the reference repeats its results (`iters` when it never froze): the freeze rule read
    back from the energies alone"""
    out = []
    for e in energy:
        old, it = float("inf"), len(e)
        for i, v in enumerate(e):
            if i > 1 and abs(v - old) <= 1e-6 * abs(old):
                it = i
                break
            old = v
        out.append(it)
    return np.asarray(out, np.int32)


def knn_margin(query64, knn):
    """min over tasks and queries of the relative difference between the fp64 squared distances to the (knn-1)-th and the
    knn-th nearest other query"""
    worst = np.inf
    for z in query64:
        d2 = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(d2, np.inf)
        s = np.sort(d2, axis=1)
        worst = min(worst, float(((s[:, knn - 1] - s[:, knn - 2]) / s[:, knn - 1]).min()))
    return worst


def make(mod, name, D, K, shots, N, seed0, signal, knn, lmd, norm_type, iters):
    for tried, seed in enumerate(range(seed0, seed0 + 20), 1):
        x_s, y_s, x_q, y_q = visual_fs.make_tasks(N, K, D, shots, seed, signal=signal)
        task = {"x_s": x_s, "y_s": y_s.unsqueeze(2), "x_q": x_q, "y_q": y_q.unsqueeze(2)}
        args = Args(knn=knn, norm_type=norm_type, iter=iters, batch_size=N, shots=shots, lmd=lmd, temp=30, num_classes_test=K,
                    n_class=K)
        r32, r64 = run_reference(mod, False, args, task, shots), run_reference(mod, True, args, task, shots)
        same_nbr = np.array_equal(r32["neighbours"], r64["neighbours"])
        same_preds = np.array_equal(r32["preds_iter"], r64["preds_iter"]) and np.array_equal(r32["acc"], r64["acc"])
        fr32, fr64 = freeze_iter(r32["ent_energy"]), freeze_iter(r64["ent_energy"])
        same_freeze = np.array_equal(fr32, fr64)
        margin = knn_margin(r64["query"], knn)
        gaps = (float(np.abs(r32["unary"] / r64["unary"] - 1).max()), float(np.abs(r32["ent_energy"] / r64["ent_energy"] - 1).max()))
        print(f"{name} seed {seed}: fp32-fp64 gaps unary {gaps[0]:.3e} energies {gaps[1]:.3e} (relative); equal neighbours "
              f"{same_nbr}, assignments {same_preds}, freeze {same_freeze} {fr32.tolist()}; kNN margin {margin:.3e}", flush=True)
        if same_nbr and same_preds and same_freeze and margin > 1e-6:
            break
    else:
        sys.exit(f"{name}: no seed satisfies the conditions")
    bounds = (max(1e-6, 2 * gaps[0]), max(1e-7, 2 * gaps[1]))
    assert r32["preds_iter"].shape == (N, iters, 75) and r32["acc"].shape == (N, iters) and r32["ent_energy"].shape == (N, iters)
    assert r32["unary"].dtype == np.float32 and r64["unary"].dtype == np.float64
    out = {"D": D, "K": K, "N": N, "shots": shots, "seed": seed, "signal": signal, "seeds_tried": tried, "knn": knn, "lmd": lmd,
           "norm_type": norm_type, "iters": iters, "inputs": "helpers.visual_fs", "y_s": y_s.numpy(), "y_q": y_q.numpy(),
           "x_s_sha1": visual_fs.sha(x_s.numpy()), "x_q_sha1": visual_fs.sha(x_q.numpy()), "y_s_sha1": visual_fs.sha(y_s.numpy()),
           "y_q_sha1": visual_fs.sha(y_q.numpy()),
           "neighbours": r32["neighbours"], "unary": r32["unary"], "preds_iter": r32["preds_iter"], "acc": r32["acc"],
           "ent_energy": r32["ent_energy"], "unary64_minus_unary": (r64["unary"] - r32["unary"].astype(np.float64)).astype(np.float32),
           "ent_energy64": r64["ent_energy"], "unary_rel": np.float64(bounds[0]), "energy_rel": np.float64(bounds[1]),
           "unary_gap": np.float64(gaps[0]), "energy_gap": np.float64(gaps[1]), "knn_margin": np.float64(margin),
           "fp32_equals_fp64_neighbours": same_nbr, "fp32_equals_fp64_assignments": same_preds, "fp32_equals_fp64_freeze": same_freeze,
           "freeze_iter": fr32, "torch_version": torch.__version__, "numpy_version": np.__version__}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: acc first/last={out['acc'][:, 0].round(3).tolist()} / {out['acc'][:, -1].round(3).tolist()} bounds={bounds} "
          f"seeds tried {tried} -> {os.path.getsize(path) / 1e3:.0f} kB", flush=True)
    assert os.path.getsize(path) < 1 << 20


def main():
    sys.path.insert(0, REF)
    import src.methods.few_shot.laplacian_shot as mod
    sys.path.pop(0)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for name in (sys.argv[1:] or list(CASES)):
        make(mod, name, *CASES[name])


if __name__ == "__main__":
    main()
