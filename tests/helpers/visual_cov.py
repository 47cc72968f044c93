"""torch-CPU restatement of EM_GAUSSIAN_COV on visual features (rows of D elements, D independent of the class count K), written
from the method's formulas; tests/test_visual_cov.py pins it bit for bit to the reference-made fixtures full_vis_emgc_*, and the GPU
shape sweep compares the engine against it.

    w[t,k,:] = sum_q u[t,q,k] z[t,q,:] / max(sum_q u[t,q,k], eps)
    s[t,k,d] = sum_q u[t,q,k] / max(sum_q (w[t,k,d] - z[t,q,d])^2 u[t,q,k], eps)
    u[t,q,:] = softmax_k(-1/2 sum_d (w - z)^2 s + 1/2 sum_d log(s + eps) + lambd v / Q),    v = log(sum_q u / Q + eps) + 1
A cluster whose size sum_q u is <= eps keeps its w and s.

The logarithm is a parameter.  torch.log on the host is MKL's vsLn, whose kernel follows the host's CPU: on the machine the
fixtures were made on it is the one csrc/tclip_math.h restates (log_f32; tests/test_math_host.py pins the two to each other
there), on another CPU vendor it is a few ulp off on a fraction of the arguments, and two of the loop's steps go through it.
restated_log() (tests/helpers/restated.py, re-exported here) is that restatement's host build (oracle/mathcheck.cpp, mc_log):
the same bits on every host."""
import torch

from helpers.restated import restated_log      # noqa: F401

EPS = 1e-15


def _w_stats(query, u):
    num = (query.unsqueeze(2) * u.unsqueeze(3)).sum(1)
    return num.div_(u.sum(1).clamp(min=EPS).unsqueeze(2))


def _s_stats(query, u, w):
    d_q = (w.unsqueeze(1) - query.unsqueeze(2)).square_().mul_(u.unsqueeze(3)).sum(1)
    return u.sum(1).unsqueeze(2) / d_q.clamp(min=EPS)


def init(query, u0):
    """(w, s) of every cluster from the initial responsibilities."""
    w = _w_stats(query, u0)
    return w, _s_stats(query, u0, w)


def step(query, u, v, w, s, lambd, log=torch.log):
    """One iteration: (u, v, w, s) from the previous ones."""
    nonzero = u.sum(1).unsqueeze(-1) > EPS
    w = _w_stats(query, u) * nonzero + w * (1 - 1 * nonzero)
    s = _s_stats(query, u, w) * nonzero + s * (1 - 1 * nonzero)
    diff = w.unsqueeze(1) - query.unsqueeze(2)
    logits = -1 / 2 * diff.square_().mul_(s.unsqueeze(1)).sum(dim=-1)
    det = 1 / 2 * log(s + EPS).sum(-1).unsqueeze(1)
    u = (logits + det + lambd * v.unsqueeze(1) / query.size(1)).softmax(2)
    v = log(u.sum(1) / u.size(1) + EPS) + 1
    return u, v, w, s


def run(query, u0, iters, lambd, log=torch.log):
    """The whole loop from u0: (u, v, w, s, preds); in float64 when its inputs are."""
    u = u0.clone()
    v = torch.zeros(u0.shape[0], u0.shape[2], dtype=u0.dtype)
    w, s = init(query, u)
    for _ in range(iters):
        u, v, w, s = step(query, u, v, w, s, lambd, log)
    return u, v, w, s, u.argmax(2).int()
