#!/usr/bin/env python3
"""Generate tests/golden/objective/obj_*.npz by RUNNING the reference: the penalised objective of the EM-Dirichlet classes per
task and outer iteration.

The reference defines `objective_function` in its two HARD_EM_DIRICHLET classes and never calls it.  Here the reference's
classes run unchanged (imported through TCLIP_REFERENCE as in make_golden.py, never copied or edited) with
`record_convergence` wrapped: after every outer iteration the wrapper reads the object's own state and records

    terms      (iters, N, 4) f64  fit_q, fit_s, ent, part - summed in float64 from the reference's own fp32 get_logits output,
                                  u and alpha
    abs_sums   (iters, N, 4) f64  the sum of |summand| of each term
    fit_s_scale (iters, N)   f64  sum_s (|rowc[y_s]| + sum_d |alpha[y_s, d] - 1| * |log x_s[d]|), rowc the reference's fp32 l1 + l2
    ref_objective (iters, N) f32  the reference's own objective_function at that state

Calling conventions: zero-shot get_logits takes probabilities, few-shot get_logits the features the class has logged in place
(the task's own tensors after run_method has started); objective_function takes probabilities, and for the soft classes it is
called unbound from the hard class of the same setting; zero-shot passes an empty (N, 0, K) support.

The host's arithmetic.  The existing fixtures were made on a host whose torch takes MKL's AVX-512 vsLn / vsSqrt kernels for
torch.log / torch.sqrt; those bits are what the engine restates (tests/test_math_host.py).  MKL dispatches by CPU, and a host
where it takes another kernel returns other bits from the same reference (alpha 1e-4 apart after twenty iterations).  On such a
host `fixture_host_arithmetic` routes fp32 torch.log, Tensor.log_ and torch.sqrt through the restated kernels of
oracle/_mathcheck.so (mc_log, mc_sqrt_torch) while the reference runs; on the fixture host it changes nothing.  Either way a
case that shares its inputs with a fixture of make_golden.py (CHECK_AGAINST) must reproduce that fixture's final u, alpha, v and
criterions bit for bit, or nothing is written.

The files live in a directory of their own: conftest.golden_names() lists every .npz directly under tests/golden/ as a
method-level fixture of make_golden.py's schema, which these are not.

    TCLIP_REFERENCE=/path/to/reference python tests/golden/make_golden_objective.py [case ...]
"""
import contextlib
import ctypes
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)          # stubs clip / torchvision, checks TCLIP_REFERENCE, loads tclip_amd.synth by path

ROOT = os.path.dirname(os.path.dirname(HERE))
EPS = 1e-15
# cases that run a make_golden.py fixture's inputs for its number of iterations: their final state must be that fixture's
CHECK_AGAINST = {"obj_zs_soft_K10_N4": "zs_soft_K10_N4", "obj_zs_hard_K37_N6": "zs_hard_K37_N6",
                 "obj_fs_soft_K37_N3_s2": "fs_soft_K37_N3_s2", "obj_fs_hard_K10_N4_s4": "fs_hard_K10_N4_s4"}
# name: (kind, K, N, iters, shots, seed); the seeded inputs are those of make_golden.py's small fixtures of the same (K, seed)
CASES = {
    "obj_zs_soft_K10_N4": ("zs_soft", 10, 4, 20, 0, 2020),
    "obj_zs_hard_K37_N6": ("zs_hard", 37, 6, 10, 0, 2021),        # clusters die
    "obj_fs_soft_K37_N3_s2": ("fs_soft", 37, 3, 20, 2, 2021),
    "obj_fs_hard_K10_N4_s4": ("fs_hard", 10, 4, 10, 4, 2020),
    "obj_zs_soft_K100_N2": ("zs_soft", 100, 2, 5, 0, 2022),
    "obj_fs_soft_K100_N2_s1": ("fs_soft", 100, 2, 4, 1, 2060),
    "obj_zs_soft_K2_N3": ("zs_soft", 2, 3, 6, 0, 2031),
}


def _mathcheck():
    spec = importlib.util.spec_from_file_location("oracle_build", os.path.join(ROOT, "oracle", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build()[1])


@contextlib.contextmanager
def fixture_host_arithmetic():
    """fp32 torch.log / Tensor.log_ / torch.sqrt with the fixture host's bits (see the module's text); other dtypes and the
    float64 sums of this script keep torch's own functions"""
    lib = _mathcheck()

    def through(fn, x):
        a = np.ascontiguousarray(x.detach().numpy())
        y = np.empty_like(a)
        getattr(lib, fn)(a.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(a.size))
        return torch.from_numpy(y)

    probe = torch.exp(torch.linspace(-34.0, 11.0, 1 << 16))
    if all(torch.equal(through(fn, probe), real(probe)) for fn, real in (("mc_log", torch.log), ("mc_sqrt_torch", torch.sqrt))):
        print("this host's torch.log and torch.sqrt have the fixture host's bits: nothing is replaced", flush=True)
        yield
        return
    print("this host's MKL takes other vsLn / vsSqrt kernels: fp32 log and sqrt go through oracle/_mathcheck.so", flush=True)
    real_log, real_sqrt, real_log_ = torch.log, torch.sqrt, torch.Tensor.log_
    fp32 = lambda x: torch.is_tensor(x) and x.dtype == torch.float32 and x.device.type == "cpu"      # noqa: E731
    torch.log = lambda x, *a, **k: through("mc_log", x) if fp32(x) and not a and not k else real_log(x, *a, **k)
    torch.sqrt = lambda x, *a, **k: through("mc_sqrt_torch", x) if fp32(x) and not a and not k else real_sqrt(x, *a, **k)
    torch.Tensor.log_ = lambda self: self.copy_(through("mc_log", self)) if fp32(self) else real_log_(self)
    try:
        yield
    finally:
        torch.log, torch.sqrt, torch.Tensor.log_ = real_log, real_sqrt, real_log_


def run_case(name, spec, classes):
    kind, K, N, iters, shots, seed = spec
    few = kind.startswith("fs")
    x_q, y_q = mg.synth.make_query_tasks(N, K, seed=seed, k_eff=(5 if few else None))
    task = {"x_q": x_q.clone(), "y_q": y_q.clone()}
    if few:
        x_s, y_s = mg.synth.make_support(N, K, shots, seed=seed)
        task["x_s"], task["y_s"] = x_s.clone(), y_s.clone()
        onehot = torch.nn.functional.one_hot(y_s.long().squeeze(2), K).float()
        support_p = x_s.clone()
    else:
        onehot = torch.zeros(N, 0, K)
        support_p = torch.zeros(N, 0, K)
    m = classes[kind](model=None, device=torch.device("cpu"), log_file=os.path.join("/tmp", "golden.log"),
                      args=mg.make_args(K, iters, shots=shots))
    hard_cls = classes["fs_hard" if few else "zs_hard"]
    live_q, live_s = task["x_q"], task.get("x_s")        # few-shot: logged in place by run_method (cpu .to() is the identity)
    rec = {"terms": [], "abs_sums": [], "fit_s_scale": [], "ref_objective": []}
    real_record = m.record_convergence

    def recording(new_time, criterions):
        real_record(new_time=new_time, criterions=criterions)
        with torch.no_grad():
            u = m.u.double()
            lq = m.get_logits(live_q).double()                     # the reference's fp32 logits of the query rows
            logu = torch.log(u + EPS)
            p = u.sum(1) / u.shape[1]
            logp = torch.log(p + EPS)
            terms = [(u * lq).sum((1, 2)), torch.zeros(N, dtype=torch.float64), (u * logu).sum((1, 2)), (p * logp).sum(1)]
            sums = [(u * lq).abs().sum((1, 2)), torch.zeros(N, dtype=torch.float64), (u * logu).abs().sum((1, 2)),
                    (p * logp).abs().sum(1)]
            scale = torch.zeros(N, dtype=torch.float64)
            if few:
                ls = (m.get_logits(live_s).double() * onehot.double()).sum(-1)      # (N, S): logits[s, y_s]
                terms[1], sums[1] = ls.sum(1), ls.abs().sum(1)
                rowc = (torch.lgamma(m.alpha.sum(-1)) - torch.lgamma(m.alpha).sum(-1)).double()      # (N, K)
                a_y = torch.einsum("nsk,nkd->nsd", onehot.double(), m.alpha.double())                # alpha[y_s]
                scale = ((onehot.double() * rowc.unsqueeze(1)).sum(-1).abs()
                         + ((a_y - 1).abs() * live_s.double().abs()).sum(-1)).sum(1)
            rec["terms"].append(torch.stack(terms, 1).numpy())
            rec["abs_sums"].append(torch.stack(sums, 1).numpy())
            rec["fit_s_scale"].append(scale.numpy())
            rec["ref_objective"].append(hard_cls.objective_function(m, support_p, x_q, onehot).float().numpy())

    m.record_convergence = recording
    with fixture_host_arithmetic():
        logs = m.run_task(task_dic=task, shot=shots) if few else m.run_task(task_dic=task)
    out = {"kind": kind, "K": K, "N": N, "iters": iters, "iter_mm": 1000, "shots": shots, "seed": seed, "lambd": int(m.lambd),
           "x_q": x_q.numpy(), "y_q": y_q.numpy(), "u": m.u.numpy(), "alpha": m.alpha.numpy(), "v": m.v.numpy(),
           "criterions": np.asarray(logs["criterions"], np.float32), "torch_version": torch.__version__}
    out.update({k: np.stack(val) for k, val in rec.items()})
    if few:
        out["x_s"], out["y_s"] = x_s.numpy(), y_s.numpy()
    if name in CHECK_AGAINST:
        g = np.load(os.path.join(HERE, CHECK_AGAINST[name] + ".npz"))
        assert int(g["iters"]) == iters and np.array_equal(g["x_q"], out["x_q"]), "not the inputs of " + CHECK_AGAINST[name]
        for key in ("u", "alpha", "v", "criterions"):
            if not np.array_equal(g[key], out[key]):
                sys.exit(f"{name}: {key} differs from {CHECK_AGAINST[name]}.npz - this run is not on the fixture host's arithmetic")
    os.makedirs(os.path.join(HERE, "objective"), exist_ok=True)
    path = os.path.join(HERE, "objective", name + ".npz")
    np.savez_compressed(path, **out)
    obj = -0.5 * (out["terms"][..., 0] + out["terms"][..., 1]) + out["terms"][..., 2] - out["lambd"] * out["terms"][..., 3]
    print(f"{name}: objective of task 0 {obj[:, 0].round(3).tolist()} max |composed - reference| "
          f"{np.abs(obj - out['ref_objective']).max():.3g} -> {os.path.getsize(path) / 1e3:.0f} kB", flush=True)


def main():
    names = sys.argv[1:] or list(CASES)
    classes = mg.load_reference_classes()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for n in names:
        run_case(n, CASES[n], classes)


if __name__ == "__main__":
    main()
