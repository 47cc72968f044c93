#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by RUNNING the reference.

Needs a checkout of the reference (TCLIP_REFERENCE).  The reference's Python
sources are imported (never copied): `clip` and `torchvision` are absent from this image and
are not used on the EM-Dirichlet path, so empty stub modules satisfy the import lines
(SURVEY.md section 8c).  What is committed is data only: seeded inputs and the outputs the
reference produced for them on torch CPU (fp32), plus per-outer-iteration traces obtained by
wrapping (not editing) the reference's methods.

    python tests/golden/make_golden.py [case ...]      # default: all small cases
    python tests/golden/make_golden.py --large         # K=397 / K=1000 cases (minutes)
"""
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
# The product package also has a top-level `src/` (it mirrors the reference's module names), so it
# must NOT be importable while the reference is: load the synthetic-data module by file path.
import importlib.util  # noqa: E402
_spec = importlib.util.spec_from_file_location(
    "tclip_synth", os.path.join(ROOT, "transductive-clip_amd", "tclip_amd", "synth.py"))
synth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(synth)
sys.path[:] = [p for p in sys.path if "transductive-clip_amd" not in p]

for _m in ("clip", "torchvision", "torchvision.transforms"):
    sys.modules.setdefault(_m, types.ModuleType(_m))
REF = os.environ.get("TCLIP_REFERENCE", "")      # a checkout of the reference, SegoleneMartin/transductive-CLIP
if not os.path.isdir(REF):
    sys.exit("set TCLIP_REFERENCE to a checkout of the reference (SegoleneMartin/transductive-CLIP)")


class Args(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def make_args(K, iters, iter_mm=1000, k_eff=5, shots=0, lambd=0.0):
    return Args(iter=iters, iter_mm=iter_mm, num_classes_test=K, n_class=K, n_query=75,
                k_eff=k_eff, T=30, use_softmax_feature=True, graph_matching=True, shots=shots, lambd=lambd)


def load_reference_classes():
    sys.path.insert(0, REF)
    from src.methods.zero_shot.em_dirichlet import EM_DIRICHLET as ZS
    from src.methods.zero_shot.hard_em_dirichlet import HARD_EM_DIRICHLET as ZSH
    from src.methods.few_shot.em_dirichlet import EM_DIRICHLET as FS
    from src.methods.few_shot.hard_em_dirichlet import HARD_EM_DIRICHLET as FSH
    from src.methods.zero_shot.soft_kmeans import SOFT_KMEANS as SKM
    from src.methods.zero_shot.hard_kmeans import HARD_KMEANS as HKM
    from src.methods.few_shot.paddle import PADDLE
    from src.methods.zero_shot.em_gaussian import EM_GAUSSIAN as EMG
    from src.methods.zero_shot.kl_kmeans import KL_KMEANS as KLK
    from src.methods.zero_shot.em_gaussian_cov import EM_GAUSSIAN_COV as EMGC
    sys.path.pop(0)
    return {"zs_soft": ZS, "zs_hard": ZSH, "fs_soft": FS, "fs_hard": FSH, "zs_skm": SKM, "zs_hkm": HKM,
            "fs_paddle": PADDLE, "zs_emg": EMG, "zs_klk": KLK, "zs_emgc": EMGC}


# PADDLE's lambd is a tunable float (paddle.yaml: 0.0); the fixtures also use a value that makes the
# class-proportion term matter
PADDLE_LAMBD = {"fs_paddle_K5_N3_s2": 2.5, "fs_paddle_K10_N4_s4": 0.0, "fs_paddle_K37_N3_s2": 20.0, "fs_paddle_K100_N3_s1": 5.0,
                "fs_paddle_K397_N1_s1": 10.0}


# name: (kind, K, N, iters, shots, seed, full_alpha)
SMALL = {
    "zs_soft_K10_N4": ("zs_soft", 10, 4, 20, 0, 2020, True),
    "zs_soft_K37_N6": ("zs_soft", 37, 6, 20, 0, 2021, True),
    "zs_soft_K100_N4": ("zs_soft", 100, 4, 20, 0, 2022, True),
    "zs_hard_K10_N4": ("zs_hard", 10, 4, 10, 0, 2020, True),
    "zs_hard_K37_N6": ("zs_hard", 37, 6, 10, 0, 2021, True),
    "zs_hard_K100_N4": ("zs_hard", 100, 4, 10, 0, 2022, True),
    "fs_soft_K10_N4_s4": ("fs_soft", 10, 4, 20, 4, 2020, True),
    "fs_soft_K37_N3_s2": ("fs_soft", 37, 3, 20, 2, 2021, True),
    "fs_hard_K10_N4_s4": ("fs_hard", 10, 4, 10, 4, 2020, True),
    "fs_hard_K37_N3_s3": ("fs_hard", 37, 3, 10, 3, 2021, True),
    # few-shot at BASELINE class counts (caltech101-sized): 4-shot, S = 400 support rows
    "fs_soft_K100_N4_s4": ("fs_soft", 100, 4, 20, 4, 2060, True),
    "fs_hard_K100_N3_s4": ("fs_hard", 100, 3, 10, 4, 2061, True),
    "zs_skm_K10_N4": ("zs_skm", 10, 4, 20, 0, 2020, True),
    "zs_skm_K37_N6": ("zs_skm", 37, 6, 20, 0, 2021, True),
    "zs_skm_K100_N4": ("zs_skm", 100, 4, 20, 0, 2022, True),
    "zs_skm_K397_N2": ("zs_skm", 397, 2, 20, 0, 2023, True),
    "zs_hkm_K10_N4": ("zs_hkm", 10, 4, 20, 0, 2020, True),
    "zs_hkm_K37_N6": ("zs_hkm", 37, 6, 20, 0, 2021, True),
    "zs_hkm_K100_N4": ("zs_hkm", 100, 4, 20, 0, 2022, True),
    "zs_hkm_K397_N2": ("zs_hkm", 397, 2, 20, 0, 2023, True),
    # the class counts of the reference's other datasets (dtd 47, flowers102 102, stanfordcars 196): rows of these lengths
    # run on 16 lanes with 3, 7 and 13 registers per lane
    "zs_soft_K47_N3": ("zs_soft", 47, 3, 20, 0, 2070, True),
    "zs_soft_K102_N2": ("zs_soft", 102, 2, 20, 0, 2071, True),
    "zs_hard_K196_N2": ("zs_hard", 196, 2, 10, 0, 2072, True),
    "fs_hard_K47_N3_s2": ("fs_hard", 47, 3, 10, 2, 2073, True),
    # found by tests/golden/find_borderline.py: a stop test of these runs lands within 1e-4 (relative) of the 1e-11 threshold
    "zs_soft_K8_N2_borderline": ("zs_soft", 8, 2, 20, 0, 6087, True),
    "zs_soft_K5_N2_borderline": ("zs_soft", 5, 2, 20, 0, 5574, True),
    # fewer than 8 classes: ATen's scalar reduction paths (scalar_inner_sum, scalar_outer_sum)
    "zs_soft_K7_N4": ("zs_soft", 7, 4, 20, 0, 2030, True),
    "zs_soft_K2_N4": ("zs_soft", 2, 4, 20, 0, 2031, True),
    "zs_hard_K5_N4": ("zs_hard", 5, 4, 10, 0, 2032, True),
    "fs_soft_K6_N3_s2": ("fs_soft", 6, 3, 20, 2, 2033, True),
    "zs_skm_K7_N4": ("zs_skm", 7, 4, 20, 0, 2034, True),
    "zs_skm_K2_N4": ("zs_skm", 2, 4, 20, 0, 2035, True),
    "zs_hkm_K2_N4": ("zs_hkm", 2, 4, 20, 0, 2036, True),
    "zs_hkm_K5_N4": ("zs_hkm", 5, 4, 20, 0, 2037, True),
    "zs_emg_K7_N4": ("zs_emg", 7, 4, 20, 0, 2038, True),
    "fs_paddle_K5_N3_s2": ("fs_paddle", 5, 3, 20, 2, 2039, True),
    "zs_klk_K2_N4": ("zs_klk", 2, 4, 10, 0, 2040, True),
    "zs_klk_K7_N4": ("zs_klk", 7, 4, 10, 0, 2041, True),
    # one iteration: the centroids of the SOFT initial assignment (products are inexact, unlike those of one-hot u);
    # at K = 2 ATen's bmm is its own unfused triple loop (75 * 2 * 2 < 400), at K = 3 it is MKL's fused chain
    "zs_klk_K2_N3_i1": ("zs_klk", 2, 3, 1, 0, 2042, True),
    "zs_klk_K3_N2_i1": ("zs_klk", 3, 2, 1, 0, 2043, True),
    "zs_klk_K10_N4": ("zs_klk", 10, 4, 10, 0, 2020, True),
    "zs_klk_K37_N6": ("zs_klk", 37, 6, 10, 0, 2021, True),
    "zs_klk_K100_N4": ("zs_klk", 100, 4, 10, 0, 2022, True),
    "zs_klk_K397_N1": ("zs_klk", 397, 1, 10, 0, 2023, True),
    "zs_emgc_K2_N4": ("zs_emgc", 2, 4, 20, 0, 2051, True),
    "zs_emgc_K7_N4": ("zs_emgc", 7, 4, 20, 0, 2052, True),
    "zs_emgc_K10_N4": ("zs_emgc", 10, 4, 20, 0, 2020, True),
    "zs_emgc_K37_N6": ("zs_emgc", 37, 6, 20, 0, 2021, True),
    "zs_emgc_K100_N4": ("zs_emgc", 100, 4, 20, 0, 2022, True),
    "zs_emgc_K397_N1": ("zs_emgc", 397, 1, 20, 0, 2023, True),
    "zs_emg_K10_N4": ("zs_emg", 10, 4, 20, 0, 2020, True),
    "zs_emg_K37_N6": ("zs_emg", 37, 6, 20, 0, 2021, True),
    "zs_emg_K100_N4": ("zs_emg", 100, 4, 20, 0, 2022, True),
    "zs_emg_K397_N1": ("zs_emg", 397, 1, 20, 0, 2023, True),
    "fs_paddle_K10_N4_s4": ("fs_paddle", 10, 4, 20, 4, 2020, True),
    "fs_paddle_K37_N3_s2": ("fs_paddle", 37, 3, 20, 2, 2021, True),
    "fs_paddle_K100_N3_s1": ("fs_paddle", 100, 3, 20, 1, 2022, True),
    "fs_paddle_K397_N1_s1": ("fs_paddle", 397, 1, 20, 1, 2023, True),
}
LARGE = {
    "zs_hard_K397_N2": ("zs_hard", 397, 2, 10, 0, 2023, False),
    "zs_soft_K397_N1": ("zs_soft", 397, 1, 20, 0, 2024, False),
    "zs_hard_K1000_N1": ("zs_hard", 1000, 1, 10, 0, 2025, False),
    "zs_soft_K1000_N1": ("zs_soft", 1000, 1, 20, 0, 2026, False),
    # few-shot at sun397 / imagenet class counts (the reference's (N,S,K,K) temporary is 0.5 GB / 4 GB here)
    "fs_soft_K397_N1_s2": ("fs_soft", 397, 1, 20, 2, 2062, False),
    "fs_soft_K1000_N1_s1": ("fs_soft", 1000, 1, 20, 1, 2063, False),
    # three tasks coupled by the MM stop test at K = 1000: the reference's fp32 norm runs over 3e6 elements per checkpoint
    "zs_soft_K1000_N3": ("zs_soft", 1000, 3, 20, 0, 2064, False),
    # a batch of MORE than 16 384 (task, class) rows: the engine sums the stop test's row terms in two stages there
    # (k_mm_decide_partial), which is the path every batch of the K = 1000 bench takes.  The reference's (N,Q,K,K)
    # temporary is 510 MB.  Inputs from tests/helpers/intsynth.py (integer draws + one division: the test regenerates
    # them, the fixture holds their digest), outputs as digests + samples ("lean").
    "bigbatch_zs_soft_K100_N170": ("zs_soft", 100, 170, 20, 0, 2080, False),
    # the same two-stage path in the other two modes the bench runs it in (round 4):
    # * HARD zero-shot at sun397's class count - configs[2]'s kernels (32 lanes per row, 13 registers per lane): 16 674 rows,
    #   10 x 1000; the reference's (N,Q,K,K) temporary is 2.0 GB;
    # * FEW-SHOT (1 shot, S = 100 support rows per task) over 17 000 rows: the reference's (N,S,K,K) temporary is 680 MB
    #   (at K = 1000 a batch of more than 16 384 rows would need 68 GB of it, so configs[4]'s own class count is out of
    #   reach of the reference on this host; the mode, not the row length, is what this fixture adds).
    "bigbatch_zs_hard_K397_N42": ("zs_hard", 397, 42, 10, 0, 2081, False),
    "bigbatch_fs_soft_K100_N170_s1": ("fs_soft", 100, 170, 20, 1, 2082, False),
    # (round 5) the headline's own kernel combination, made by the reference: 17 tasks at K = 1000 are 17 000 rows, so the
    # engine runs k_mm_live<16,4,false,1,64,1000> + k_mm_split<16,64,1000> + the two-stage stop test (k_mm_decide_partial) -
    # what every batch of the K = 1000 bench runs.  The reference's (N,Q,K,K) temporary is 5.1 GB; full 20 x 1000 schedule.
    "bigbatch_zs_soft_K1000_N17": ("zs_soft", 1000, 17, 20, 0, 2083, False),
    # (round 5) configs[4]'s support size: ONE task at K = 1000 with 4 shots, S = 4000 support rows.  The reference's
    # (1,S,K,K) temporary is 16 GB (few_shot/em_dirichlet.py:196-200), once per outer iteration.
    "lean_fs_soft_K1000_N1_s4": ("fs_soft", 1000, 1, 20, 4, 2084, False),
}
INTSYNTH_LEAN = {"bigbatch_zs_soft_K100_N170", "bigbatch_zs_hard_K397_N42", "bigbatch_fs_soft_K100_N170_s1",
                 "bigbatch_zs_soft_K1000_N17", "lean_fs_soft_K1000_N1_s4"}
LEAN_BOOST = 64          # soft rows: the first outer iteration of the 170-task batch stops at MM iteration 151 (boost 4096: never)


def run_case(name, spec, classes):
    kind, K, N, iters, shots, seed, full = spec
    few = kind.startswith("fs")
    lean = name in INTSYNTH_LEAN
    if lean:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from helpers import intsynth
        sys.path.pop(0)
        if few:
            xq_np, yq_np, xs_np, ys_np = intsynth.make_tasks(seed, N, K, 75, shots=shots, boost=LEAN_BOOST)
        else:
            xq_np, yq_np = intsynth.make_tasks(seed, N, K, 75, boost=LEAN_BOOST)
        x_q, y_q = torch.from_numpy(xq_np), torch.from_numpy(yq_np).unsqueeze(2)
    else:
        x_q, y_q = synth.make_query_tasks(N, K, seed=seed, k_eff=(5 if few else None))
    task = {"x_q": x_q.clone(), "y_q": y_q.clone()}
    if few:
        if lean:
            x_s, y_s = torch.from_numpy(xs_np), torch.from_numpy(ys_np).unsqueeze(2)
        else:
            x_s, y_s = synth.make_support(N, K, shots, seed=seed)
        task["x_s"], task["y_s"] = x_s.clone(), y_s.clone()
    args = make_args(K, iters, shots=shots, lambd=PADDLE_LAMBD.get(name, 0.0))
    m = classes[kind](model=None, device=torch.device("cpu"), log_file=os.path.join("/tmp", "golden.log"),
                      args=args)

    trace = {"mm_iters": [], "argmax": [], "live": [], "stop_test": []}
    sqrt_calls = [0]
    real_sqrt = torch.sqrt

    def counting_sqrt(*a, **k):
        sqrt_calls[0] += 1
        return real_sqrt(*a, **k)

    # the MM stop test is the only caller of torch.norm without a `dim`: record both norms so
    # that tests can tell a borderline `crit < 1e-11` decision from a wrong one
    real_norm = torch.norm
    norm_vals = []

    def recording_norm(x, *a, **k):
        r = real_norm(x, *a, **k)
        if not a and not k:
            norm_vals.append(float(r))
        return r

    is_skm = kind in ("zs_skm", "zs_hkm", "fs_paddle", "zs_emg", "zs_klk", "zs_emgc")      # k-means family: no MM loop, the centroids stand in for alpha
    real_update_alpha = None if is_skm else m.update_alpha

    def traced_update_alpha(alpha_0, y_cst):
        sqrt_calls[0] = 0
        del norm_vals[:]
        trace["live"].append((m.u.sum(1) > m.eps).numpy().copy())
        real_update_alpha(alpha_0, y_cst)
        trace["mm_iters"].append(sqrt_calls[0])
        row = np.full((19, 2), np.nan, np.float64)     # (checkpoint, [||b'-b||, ||b||]) as fp32 values
        nv = np.asarray(norm_vals, np.float64).reshape(-1, 2)
        row[:len(nv)] = nv
        trace["stop_test"].append(row)

    if kind == "zs_klk":             # KL_KMEANS has no u_update: its assignment is the argmin of kl_divergence (kl_kmeans.py:172-173)
        real_kl = m.kl_divergence

        def traced_kl(P, Q):
            divs = real_kl(P, Q)
            trace["argmax"].append(divs.argmin(-1).to(torch.int16).numpy().copy())
            return divs
        m.kl_divergence = traced_kl
    else:
        real_u_update = m.u_update

        def traced_u_update(q):
            real_u_update(q)
            pick = m.u.argmin(2) if kind == "zs_hkm" else m.u.argmax(2)     # HARD_KMEANS assigns by argmin (hard_kmeans.py:193)
            trace["argmax"].append(pick.to(torch.int16).numpy().copy())
        m.u_update = traced_u_update

    if not is_skm:
        m.update_alpha = traced_update_alpha
    torch.sqrt = counting_sqrt
    torch.norm = recording_norm
    t0 = time.time()
    try:
        logs = m.run_task(task_dic=task, shot=shots) if few else m.run_task(task_dic=task)
    finally:
        torch.sqrt = real_sqrt
        torch.norm = real_norm
    dt = time.time() - t0

    alpha = m.w.numpy() if is_skm else m.alpha.numpy()      # soft k-means: the centroids
    out = {
        "kind": kind, "K": K, "N": N, "iters": iters, "iter_mm": 1000, "shots": shots, "seed": seed,
        "x_q": x_q.numpy(), "y_q": y_q.numpy(),
        "mm_iters": np.asarray(trace["mm_iters"], np.int32),
        "argmax": np.stack(trace["argmax"]),            # (iters, N, Q) int16
        "live": np.stack(trace["live"]) if trace["live"] else np.zeros(0),            # (iters, N, K) bool
        "stop_test": np.stack(trace["stop_test"]) if trace["stop_test"] else np.zeros(0),   # norms seen by the MM stop test
        "criterions": np.asarray(logs["criterions"], np.float32),
        "acc": np.asarray(logs["acc"], np.float32),
        "v": m.v.numpy() if hasattr(m, "v") and kind != "zs_skm" and kind != "zs_hkm" else np.zeros(0),
        "lambd": float(args.lambd),
        "torch_version": torch.__version__, "ref_seconds": dt,
    }
    if few:
        out["x_s"], out["y_s"] = x_s.numpy(), y_s.numpy()
    if kind == "zs_emgc":
        out["s"] = m.s.numpy()        # inverse diagonal covariances
    if lean:
        import hashlib
        sha = lambda a: hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()      # noqa: E731
        del out["x_q"]
        out["inputs"] = "intsynth"
        out["boost"] = LEAN_BOOST
        out["x_q_sha1"] = sha(x_q.numpy())
        if few:
            del out["x_s"]
            out["x_s_sha1"] = sha(x_s.numpy())
        out["u_sha1"] = sha(m.u.numpy())
        out["alpha_sha1"] = sha(alpha)
        rng = np.random.default_rng(seed)
        rows = np.stack([np.sort(rng.choice(K, size=(8 if N > 8 else 64), replace=False)) for _ in range(N)])
        out["alpha_rows_idx"] = rows.astype(np.int32)
        out["alpha_rows"] = np.stack([alpha[n, rows[n]] for n in range(N)])
        a64 = alpha.astype(np.float64)
        out["alpha_rowsum"] = a64.sum(-1)
        out["alpha_rowsumsq"] = (a64 * a64).sum(-1)
        if N <= 8:
            out["u"] = m.u.numpy()
    elif full:
        out["alpha"] = alpha
        out["u"] = m.u.numpy()
    else:
        # K>=397: full alpha is 0.6-4 MB per task; keep the responsibilities, 64 sampled rows
        # per task and float64 per-row checksums (sum and sum of squares) of every row.
        rng = np.random.default_rng(seed)
        rows = np.stack([np.sort(rng.choice(K, size=min(64, K), replace=False)) for _ in range(N)])
        out["u"] = m.u.numpy()
        out["alpha_rows_idx"] = rows.astype(np.int32)
        out["alpha_rows"] = np.stack([alpha[n, rows[n]] for n in range(N)])
        a64 = alpha.astype(np.float64)
        out["alpha_rowsum"] = a64.sum(-1)
        out["alpha_rowsumsq"] = (a64 * a64).sum(-1)
        import hashlib
        out["alpha_sha1"] = hashlib.sha1(np.ascontiguousarray(alpha).tobytes()).hexdigest()   # every bit of alpha
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {dt:.1f}s mm_iters={out['mm_iters'].tolist()} acc={out['acc'].ravel().round(3).tolist()} "
          f"-> {os.path.getsize(path) / 1e3:.0f} kB", flush=True)


def main():
    argv = sys.argv[1:]
    table = dict(SMALL)
    if "--large" in argv:
        argv.remove("--large")
        table = dict(LARGE)
    names = argv or list(table)
    classes = load_reference_classes()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    allc = {**SMALL, **LARGE}
    for n in names:
        run_case(n, allc[n], classes)


if __name__ == "__main__":
    main()
