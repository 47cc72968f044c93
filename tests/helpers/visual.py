"""Seeded inputs of the visual-feature k-means fixtures (tests/golden/make_golden_visual.py) and a torch-eager restatement of
the reference's op sequence for one iteration of its loop (src/methods/zero_shot/{soft_kmeans,hard_kmeans,em_gaussian}.py,
use_softmax_feature == False).  numpy's PCG64 draws the inputs, so they are the same bits on every machine."""
import numpy as np
import torch


def make_text(K, D, seed):
    """(K, D) float32 unit-norm rows: the text features clip_weights returns."""
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.standard_normal((K, D)).astype(np.float32))
    return t / t.norm(dim=-1, keepdim=True)


def make_embeddings(text, labels, seed, scale=10.0, signal=0.35, common=0.5):
    """Raw image embeddings (..., D) float32 around their class's text direction: scale * (signal * text[label] + common *
    a shared direction + isotropic noise of unit expected norm), like CLIP's un-normalised visual features."""
    K, D = text.shape
    rng = np.random.default_rng(seed)
    shared = rng.standard_normal(D).astype(np.float32)
    shared /= np.linalg.norm(shared)
    lab = np.asarray(labels)
    noise = rng.standard_normal(lab.shape + (D,)).astype(np.float32) / np.float32(np.sqrt(D))
    x = scale * (signal * text.numpy()[lab] + common * shared + noise)
    return torch.from_numpy(x.astype(np.float32))


def make_tasks(N, K, D, seed, n_query=75, k_eff=5):
    """N zero-shot tasks of n_query queries drawn from min(k_eff, K) classes each: (x_q (N,Q,D), y_q (N,Q) int64, text (K,D))."""
    text = make_text(K, D, seed)
    rng = np.random.default_rng(seed + 1)
    labels = np.stack([rng.choice(rng.choice(K, size=min(k_eff, K), replace=False), size=n_query) for _ in range(N)])
    x_q = make_embeddings(text, labels, seed + 2)
    return x_q, torch.from_numpy(labels.astype(np.int64)), text


def make_table(K, D, rows_per_class, seed):
    """A visual feature table for the task-batch loop: (feats (K*rows, D) f32, labels (K*rows,) int64, text (K, D))."""
    text = make_text(K, D, seed)
    labels = np.repeat(np.arange(K), rows_per_class)
    return make_embeddings(text, labels, seed + 2), torch.from_numpy(labels.astype(np.int64)), text


def reference_init(x_q, text, T):
    """u0[t] = softmax_k(T * (x_q[t]/||x_q[t]|| @ text.T)), task by task as the reference loops (soft_kmeans.py:185-197)"""
    u = torch.zeros(x_q.shape[0], x_q.shape[1], text.shape[0])
    for t in range(x_q.shape[0]):
        f = x_q[t] / x_q[t].norm(dim=-1, keepdim=True)
        u[t] = (T * (f @ text.T)).softmax(dim=-1)
    return u


def reference_step(method, query, u, w=None, v=None, T=30.0, lambd=0, eps=1e-15, log=torch.log):
    """One iteration of the reference's loop from u (and the previous w / v), torch CPU: returns (u, w, v).  w=None: the w_init
    of SOFT_KMEANS / EM_GAUSSIAN first.  HARD_KMEANS returns u one-hot.  `log`: the logarithm of EM_GAUSSIAN's v_update
    (helpers/restated.restated_log() is the reference host's on every host); float64 inputs run the step in float64."""
    if method != "hard_kmeans" and w is None:
        num = (query.unsqueeze(2) * u.unsqueeze(3)).sum(1)
        den = u.sum(1).clamp(min=eps)
        w = num.div_(den.unsqueeze(2))
    num = (query.unsqueeze(2) * u.unsqueeze(3)).sum(1)
    den = u.sum(1).clamp(min=eps)
    nonzero = u.sum(1).unsqueeze(-1) > eps
    if method == "hard_kmeans":
        w = num.div_(den.unsqueeze(2)) * nonzero
    else:
        w = num.div_(den.unsqueeze(2)) * nonzero + (w * (1 - 1 * nonzero))
    diff = w.unsqueeze(1) - query.unsqueeze(2)
    logits = diff.square_().sum(dim=-1)
    if method == "hard_kmeans":
        u = logits.softmax(2)
        labels = torch.argmin(u, dim=-1)
        u.zero_()
        u.scatter_(2, labels.unsqueeze(-1), 1.0)
    elif method == "em_gaussian":
        if v is None:
            v = torch.zeros(u.shape[0], u.shape[2], dtype=u.dtype)
        u = (T * (-1 / 2 * logits) + lambd * v.unsqueeze(1) / query.size(1)).softmax(2)
        v = log(u.sum(1) / u.size(1) + eps) + 1
    else:
        u = (T * (-1 / 2 * logits)).softmax(2)
    return u, w, v
