"""GPU: the logs contract of every reference-named method class (what the evaluators and a reference checkout read):
the keys of run_task's dict, shape and dtype of `acc` and `criterions`, a finite `timestamps` scalar, how many wall-clock
entries the class records per call, and the banner of its first log line.  The values themselves are pinned by the
reference fixtures elsewhere; this file pins the bookkeeping around them, on synthetic tasks small enough for all fourteen
classes to take a few seconds together."""
import numpy as np
import pytest
import torch

from src.utils import CfgNode
from tclip_amd import synth

pytestmark = pytest.mark.gpu

K, N_TASK, N_QUERY, SHOTS, ITER = 5, 2, 75, 1, 2
F32, I64 = np.dtype(np.float32), np.dtype(np.int64)

# class: (module, name, banner text, entries of self.timestamps before get_logs, acc shape, criterions shape, criterions dtype)
ZERO_SHOT = [
    ("zero_shot.em_dirichlet", "EM_DIRICHLET", "EM-DIRICHLET", ITER, (N_TASK, 1), (ITER,), F32),
    ("zero_shot.hard_em_dirichlet", "HARD_EM_DIRICHLET", "HARD EM-DIRICHLET", ITER, (N_TASK, 1), (ITER,), F32),
    ("zero_shot.soft_kmeans", "SOFT_KMEANS", "SOFT K-MEANS", ITER, (N_TASK, 1), (ITER,), F32),
    ("zero_shot.hard_kmeans", "HARD_KMEANS", "HARD_KMEANS", 2 * ITER, (N_TASK, 1), (2 * ITER,), F32),
    ("zero_shot.kl_kmeans", "KL_KMEANS", "KL KMEANS", 2 * ITER, (N_TASK, 1), (2 * ITER,), F32),
    ("zero_shot.em_gaussian", "EM_GAUSSIAN", "EM_GAUSSIAN", ITER, (N_TASK, 1), (ITER,), F32),
    ("zero_shot.em_gaussian_cov", "EM_GAUSSIAN_COV", "EM_GAUSSIAN_COV", ITER, (N_TASK, 1), (ITER,), F32),
    ("zero_shot.inductive_clip", "CLIP", "CLIP", 1, (N_TASK, 1), (1,), F32),
]
FEW_SHOT = [
    ("few_shot.em_dirichlet", "EM_DIRICHLET", "EM-DIRICHLET", ITER, (N_TASK, 1), (ITER,), F32),
    ("few_shot.hard_em_dirichlet", "HARD_EM_DIRICHLET", "HARD EM-DIRICHLET", ITER, (N_TASK, 1), (ITER,), F32),
    ("few_shot.paddle", "PADDLE", "PADDLE", ITER, (N_TASK, 1), (ITER,), F32),
    ("few_shot.tim", "TIM_GD", "TIM", ITER, (N_TASK, 1), (ITER, N_TASK), F32),
    ("few_shot.tim", "ALPHA_TIM", "ALPHA_TIM", ITER, (N_TASK, 1), (ITER,), F32),
    ("few_shot.bdcspn", "BDCSPN", "BD-CSPN", 1, (N_TASK, 1), (1, 1), F32),
    ("few_shot.laplacian_shot", "LAPLACIAN_SHOT", "LAPLACIAN SHOT", N_TASK, (N_TASK, ITER), (N_TASK, 1), I64),
]


@pytest.fixture(scope="module")
def tasks():
    x_q, y_q = synth.make_query_tasks(N_TASK, K, seed=11, n_query=N_QUERY)
    x_f, y_f = synth.make_query_tasks(N_TASK, K, seed=12, n_query=N_QUERY, k_eff=K)
    x_s, y_s = synth.make_support(N_TASK, K, SHOTS, seed=12)
    return {"zero": {"x_q": x_q, "y_q": y_q}, "few": {"x_q": x_f, "y_q": y_f, "x_s": x_s, "y_s": y_s}}


def _args():
    return CfgNode(iter=ITER, iter_mm=60, num_classes_test=K, n_class=K, n_query=N_QUERY, k_eff=K, T=30,
                   use_softmax_feature=True, graph_matching=True, shots=SHOTS, batch_size=N_TASK, knn=3, lmd=0.7,
                   norm_type="L2N", temp=15.0, lambd=1.0, loss_weights=[1.0, 1.0, 1.0], lr_tim=1e-4, lr_alpha_tim=1e-4,
                   entropies=["Shannon", "Alpha", "Alpha"], alpha_value=7.0)


@pytest.mark.parametrize("module,name,banner,n_stamps,acc_shape,crit_shape,crit_dtype", ZERO_SHOT + FEW_SHOT,
                         ids=[f"{c[0]}.{c[1]}" for c in ZERO_SHOT + FEW_SHOT])
def test_logs_contract(tasks, module, name, banner, n_stamps, acc_shape, crit_shape, crit_dtype):
    few = module.startswith("few_shot")
    cls = getattr(__import__(f"src.methods.{module}", fromlist=[name]), name)
    m = cls(model=None, device=torch.device("cuda:0"), log_file=None, args=_args())
    lines, seen = [], {}
    info, get_logs = m.logger.info, m.get_logs

    def record_line(msg):
        lines.append(msg)
        info(msg)

    def count_then_get_logs():
        seen["stamps"] = len(m.timestamps)
        return get_logs()

    m.logger.info, m.get_logs = record_line, count_then_get_logs
    task = {k: v.clone() for k, v in tasks["few" if few else "zero"].items()}
    logs = m.run_task(task, SHOTS) if few else m.run_task(task)

    want_keys = {"timestamps", "criterions", "acc"} | ({"ent_energy"} if name == "LAPLACIAN_SHOT" else set())
    assert set(logs) == want_keys
    acc, crit = logs["acc"], logs["criterions"]
    assert isinstance(acc, np.ndarray) and acc.shape == acc_shape and acc.dtype == F32
    assert isinstance(crit, list if name == "LAPLACIAN_SHOT" else np.ndarray)
    crit = np.asarray(crit)
    print(name, "acc", acc.shape, acc.dtype, "criterions", crit.shape, crit.dtype, "timestamps", logs["timestamps"],
          "entries", seen.get("stamps"), "first line", lines[:1])
    assert crit.shape == crit_shape and crit.dtype == crit_dtype
    if name == "LAPLACIAN_SHOT":
        assert logs["ent_energy"].shape == (N_TASK, ITER)
    assert ((acc >= 0) & (acc <= 1)).all()
    stamp = logs["timestamps"]
    assert np.ndim(stamp) == 0 and np.isfinite(stamp) and stamp >= 0
    assert seen["stamps"] == n_stamps
    assert lines and "Executing" in lines[0] and banner in lines[0]
    if hasattr(cls, "BANNER"):
        assert cls.BANNER == banner
