"""Seeded inputs of the few-shot visual-feature fixtures (tests/golden/make_golden_visual_fs.py) and a torch-eager restatement
of the reference's op sequences on D-dim embeddings: one PADDLE iteration (src/methods/few_shot/paddle.py:94-158) and the
BD-CSPN pass (src/methods/few_shot/bdcspn.py:42-200).  The inputs are drawn by tests/helpers/visual.py (numpy's PCG64), so they
are the same bits on every machine."""
import hashlib

import numpy as np
import torch

from helpers import visual


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_tasks(N, K, D, shots, seed, n_query=75, k_eff=5, signal=0.35):
    """N few-shot tasks on visual features: the support set is every class x `shots` rows in class order with the labels
    unchanged (visual features are not relabelled), the queries come from min(k_eff, K) classes per task.
    Returns (x_s (N,K*shots,D), y_s (N,K*shots) int64, x_q (N,Q,D), y_q (N,Q) int64)."""
    text = visual.make_text(K, D, seed)
    rng = np.random.default_rng(seed + 1)
    y_q = np.stack([rng.choice(rng.choice(K, size=min(k_eff, K), replace=False), size=n_query) for _ in range(N)])
    y_s = np.stack([np.repeat(np.arange(K), shots) for _ in range(N)])
    x_q = visual.make_embeddings(text, y_q, seed + 2, signal=signal)
    x_s = visual.make_embeddings(text, y_s, seed + 3, signal=signal)
    return x_s, torch.from_numpy(y_s.astype(np.int64)), x_q, torch.from_numpy(y_q.astype(np.int64))


def make_tables(K, D, rows_per_class, seed, signal=0.35):
    """The train and the test table of an evaluator run on visual features:
    (feats_s (K*rows, D), labels_s, feats_q (K*rows, D), labels_q), labels int64 in class order."""
    text = visual.make_text(K, D, seed)
    labels = np.repeat(np.arange(K), rows_per_class)
    lab = torch.from_numpy(labels.astype(np.int64))
    return (visual.make_embeddings(text, labels, seed + 2, signal=signal), lab,
            visual.make_embeddings(text, labels, seed + 3, signal=signal), lab.clone())


def random_tasks(N, K, D, shots, seed, n_query=75, scale=1.0):
    """Unstructured tasks for the shape sweeps: normal rows, every class `shots` times in the support set in a seeded order
    (so that member rows are scattered over the cascade blocks)."""
    gen = torch.Generator().manual_seed(seed)
    S = K * shots
    x_s = torch.randn(N, S, D, generator=gen) * scale
    x_q = torch.randn(N, n_query, D, generator=gen) * scale
    y_s = torch.stack([torch.arange(K).repeat_interleave(shots)[torch.randperm(S, generator=gen)] for _ in range(N)])
    return x_s, y_s, x_q


def one_hot(y, K, dtype=torch.float32):
    return torch.zeros(y.shape + (K,), dtype=dtype).scatter_(-1, y.unsqueeze(-1), 1.0)


def support_sums(support, y_s, K):
    """(class sums (N,K,D), counts (N,K)) as init_w / w_update / proto_rectification build them"""
    h = one_hot(y_s, K)
    return (h.unsqueeze(-1) * support.unsqueeze(2)).sum(1), h.sum(1)


def paddle_step(support, query, y_s, K, lambd, w=None, v=None, eps=1e-15, log=torch.log):
    """One iteration of PADDLE's loop (u_update, v_update, w_update) from w and v, torch CPU; w=None: init_w first, v=None: zeros.
    Returns (u, v, w).  `log`: the logarithm of the v_update (helpers/restated.restated_log() is the reference host's on every
    host); float64 rows run the step in float64."""
    h = one_hot(y_s, K, query.dtype)
    if w is None:
        counts = h.sum(1).unsqueeze(-1)
        w = (h.unsqueeze(-1) * support.unsqueeze(2)).sum(1).div_(counts)
    if v is None:
        v = torch.zeros(query.shape[0], K, dtype=query.dtype)
    diff = w.unsqueeze(1) - query.unsqueeze(2)
    logits = -1 / 2 * diff.square_().sum(dim=-1)
    del diff
    u = (logits + lambd * v.unsqueeze(1) / query.size(1)).softmax(2)
    v = log(u.sum(1) / u.size(1) + eps) + 1
    num = (query.unsqueeze(2) * u.unsqueeze(3)).sum(1)
    den = u.sum(1)
    num.add_((support.unsqueeze(2) * h.unsqueeze(3)).sum(1))
    den.add_(h.sum(1))
    w = num.div_(den.unsqueeze(2))
    return u, v, w


def _get_logits(w, samples):
    w = w / w.norm(p=2, dim=-1, keepdim=True)
    samples = samples / samples.norm(p=2, dim=-1, keepdim=True)
    if len(w.shape) == 3:
        diff = w.unsqueeze(1) - samples.unsqueeze(2)
    else:
        diff = w.unsqueeze(0) - samples.unsqueeze(1)
    return -1 / 2 * diff.square_().sum(dim=-1)


def bdcspn_pass(support, query, y_s, K, temp, norm_type):
    """BD-CSPN's run_task from raw rows: normalisation, prototype rectification task by task, prediction.
    Returns (rectified prototypes (N,K,D), u (N,Q,K), preds (N,Q)); in float64 when the rows are."""
    mean = support.mean(1).unsqueeze(1)
    if norm_type == "CL2N":
        support = support - mean
        support = support / support.norm(p=2, dim=2, keepdim=True)
        query = query - mean
        query = query / query.norm(p=2, dim=2, keepdim=True)
    elif norm_type == "L2N":
        support = support / support.norm(p=2, dim=2, keepdim=True)
        query = query / query.norm(p=2, dim=2, keepdim=True)
    n_task, _, D = query.shape
    prototypes = torch.zeros(n_task, K, D, dtype=query.dtype)
    h = one_hot(y_s, K, query.dtype)
    counts = h.sum(1).unsqueeze(-1)
    init = (h.unsqueeze(-1) * support.unsqueeze(2)).sum(1).div_(counts)
    for j in range(n_task):
        eta = support[j].mean(0) - query[j].mean(0)
        aug = torch.cat((support[j], query[j] + eta), dim=0)
        u = (temp * _get_logits(init[j], aug)).softmax(-1)
        aug = aug / aug.norm(p=2, dim=-1, keepdim=True)
        cnt = u.sum(0).unsqueeze(-1)
        prototypes[j] = (u.unsqueeze(-1) * aug.unsqueeze(1)).sum(0).div_(cnt)
    u = (temp * _get_logits(prototypes, query)).softmax(-1)
    return prototypes, u, u.argmax(2)
