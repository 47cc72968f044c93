"""A torch-autograd restatement of the reference's ALPHA_TIM (src/methods/few_shot/tim.py:203-322), written here from its op
sequence: what the GPU shape sweep compares against.  Rows have D elements, D independent of the class count; nothing is
normalised.  Also the loader and the bound check of the fs_vis_alpha_tim_* fixtures (tests/golden/make_golden_visual_alpha_tim.py)."""
import os

import numpy as np
import torch

from helpers import tim_gd, visual_fs

VISUAL = ["fs_vis_alpha_tim_D512_K10_S4_N3", "fs_vis_alpha_tim_D1024_K37_S2_N2", "fs_vis_alpha_tim_D768_K100_S1_N1"]


def loss(weights, support, query, hot, *, temp, alpha_value, loss_weights, entropies):
    """ALPHA_TIM's objective (:262-305), summed over the tasks -> (loss, logits_q)"""
    lw, a = list(loss_weights), alpha_value
    logits_s, logits_q = tim_gd.get_logits(weights, support, temp), tim_gd.get_logits(weights, query, temp)   # :203-217
    q_probs = logits_q.softmax(2)
    if entropies[0] == "Shannon":                                                      # :270-280
        ce = -(hot * torch.log(logits_s.softmax(2) + 1e-12)).sum(2).mean(1).sum(0)
    else:
        ce = torch.pow(hot, a) * torch.pow(logits_s.softmax(2) + 1e-12, 1 - a)
        ce = ((1 - ce.sum(2)) / (a - 1)).mean(1).sum(0)
    if entropies[1] == "Shannon":                                                      # :282-290
        q_ent = -(q_probs.mean(1) * torch.log(q_probs.mean(1))).sum(1).sum(0)
    else:
        q_ent = ((1 - (torch.pow(q_probs.mean(1), a)).sum(1)) / (a - 1)).sum(0)
    if entropies[2] == "Shannon":                                                      # :292-300
        q_cond_ent = -(q_probs * torch.log(q_probs + 1e-12)).sum(2).mean(1).sum(0)
    else:
        q_cond_ent = ((1 - (torch.pow(q_probs + 1e-12, a)).sum(2)) / (a - 1)).mean(1).sum(0)
    return lw[0] * ce - (lw[1] * q_ent - lw[2] * q_cond_ent), logits_q


def loss_gradient(x_q, x_s, y_s, *, n_class, temp, alpha_value, loss_weights=(1.0, 1.0, 1.0),
                  entropies=("Shannon", "Alpha", "Alpha"), dtype=torch.float64):
    """-> (w0 (N,K,D): the class means the loop starts from, d loss / d weights there, logits_q of that forward pass), one
    backward pass in `dtype`"""
    support, query, hot, w0 = tim_gd.setup(x_q, x_s, y_s, n_class, dtype)             # init_weights (:219-238)
    w0.requires_grad_()
    value, logits_q = loss(w0, support, query, hot, temp=temp, alpha_value=alpha_value, loss_weights=loss_weights,
                           entropies=entropies)
    value.backward()
    return w0.detach(), w0.grad.detach(), logits_q.detach()


def run_alpha_tim(x_q, x_s, y_s, *, n_class, iters, temp, lr, alpha_value, loss_weights=(1.0, 1.0, 1.0),
                  entropies=("Shannon", "Alpha", "Alpha"), dtype=torch.float32):
    """x_q (N,Q,D), x_s (N,S,D), y_s (N,S) or (N,S,1), all tasks one batch -> dict(weights (N,K,D), logits_q (N,Q,K) of the last
    iteration's forward pass, criterions (iters,): mean over tasks and classes of ||w_old - w|| per step, argmax (N,Q))."""
    support, query, hot, weights = tim_gd.setup(x_q, x_s, y_s, n_class, dtype)        # init_weights (:219-238)
    weights.requires_grad_()
    optimizer = torch.optim.Adam([weights], lr=lr)
    criterions, logits_q = [], None
    for _ in range(iters):
        weights_old = weights.detach().clone()
        value, logits_q = loss(weights, support, query, hot, temp=temp, alpha_value=alpha_value, loss_weights=loss_weights,
                               entropies=entropies)
        optimizer.zero_grad()
        value.backward()
        optimizer.step()
        criterions.append((weights_old - weights.detach()).norm(dim=-1).mean())        # one value per step (:313-314)
    logits_q = logits_q.detach()
    return {"weights": weights.detach(), "logits_q": logits_q, "criterions": torch.stack(criterions), "argmax": logits_q.argmax(2)}


def load_fixture(golden_dir, name):
    """a fixture as a dict of numpy arrays, its inputs regenerated from the seed and checked against the stored digests"""
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    x_s, _, x_q, _ = visual_fs.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"]), int(g["seed"]), signal=float(g["signal"]))
    g["x_s"], g["x_q"] = x_s.numpy(), x_q.numpy()
    assert visual_fs.sha(g["x_s"]) == str(g["x_s_sha1"]) and visual_fs.sha(g["x_q"]) == str(g["x_q_sha1"]), name
    return g


def params(g):
    return dict(iters=int(g["iters"]), temp=float(g["temp"]), lr=float(g["lr"]), alpha_value=float(g["alpha_value"]),
                loss_weights=[float(w) for w in g["loss_weights"]], entropies=[str(e) for e in g["entropies"]])
