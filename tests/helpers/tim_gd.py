"""A torch-autograd restatement of the reference's TIM_GD (src/methods/few_shot/tim.py:99-189), written here from its op
sequence: what the GPU shape sweep and the CPU fixture test compare against.  Rows have D elements, D independent of the
class count; nothing is normalised."""
import torch


def setup(x_q, x_s, y_s, n_class, dtype):
    """-> (support, query, hot (N,S,K), the class means of the support rows: init_weights, :115-131), all of `dtype`"""
    support, query = x_s.clone().to(dtype), x_q.clone().to(dtype)
    n_task = query.shape[0]
    y_s = y_s.long().view(n_task, -1)
    hot = torch.zeros(y_s.shape + (n_class,), dtype=dtype).scatter_(-1, y_s.unsqueeze(-1), 1.0)
    counts = hot.sum(1).view(n_task, -1, 1)
    return support, query, hot, hot.transpose(1, 2).matmul(support) / counts


def get_logits(weights, samples, temp):                                                # :99-113
    n_task = samples.shape[0]
    return temp * (samples.matmul(weights.transpose(1, 2)) - 1 / 2 * (weights ** 2).sum(2).view(n_task, 1, -1)
                   - 1 / 2 * (samples ** 2).sum(2).view(n_task, -1, 1))


def loss(weights, support, query, hot, *, temp, loss_weights):
    """TIM_GD's objective (:160-175), summed over the tasks -> (loss, logits_q)"""
    lw = list(loss_weights)
    logits_s, logits_q = get_logits(weights, support, temp), get_logits(weights, query, temp)
    ce = -(hot * torch.log(logits_s.softmax(2) + 1e-12)).sum(2).mean(1).sum(0)
    q_probs = logits_q.softmax(2)
    q_cond_ent = -(q_probs * torch.log(q_probs + 1e-12)).sum(2).mean(1).sum(0)
    q_ent = -(q_probs.mean(1) * torch.log(q_probs.mean(1) + 1e-12)).sum(1).sum(0)
    return lw[0] * ce - (lw[1] * q_ent - lw[2] * q_cond_ent), logits_q


def loss_gradient(x_q, x_s, y_s, *, n_class, temp, loss_weights=(1.0, 0.3, 1.0), dtype=torch.float64):
    """-> (w0 (N,K,D): the class means the loop starts from, d loss / d weights there, logits_q of that forward pass), one
    backward pass in `dtype`"""
    support, query, hot, w0 = setup(x_q, x_s, y_s, n_class, dtype)
    w0.requires_grad_()
    value, logits_q = loss(w0, support, query, hot, temp=temp, loss_weights=loss_weights)
    value.backward()
    return w0.detach(), w0.grad.detach(), logits_q.detach()


def run_tim_gd(x_q, x_s, y_s, *, n_class, iters, temp, lr, loss_weights=(1.0, 0.3, 1.0), dtype=torch.float32):
    """x_q (N,Q,D), x_s (N,S,D), y_s (N,S) or (N,S,1) -> dict(weights (N,K,D), logits_q (N,Q,K) of the last iteration's forward
    pass, criterions (iters, N): mean_class ||w_old - w|| per step and task, argmax (N,Q)).  dtype=torch.float64 runs the
    inputs, the weights and the whole loop in double."""
    support, query, hot, weights = setup(x_q, x_s, y_s, n_class, dtype)
    weights.requires_grad_()
    optimizer = torch.optim.Adam([weights], lr=lr)
    criterions, logits_q = [], None
    for _ in range(iters):
        weights_old = weights.detach().clone()
        value, logits_q = loss(weights, support, query, hot, temp=temp, loss_weights=loss_weights)
        optimizer.zero_grad()
        value.backward()
        optimizer.step()
        criterions.append((weights_old - weights.detach()).norm(dim=-1).mean(-1))      # one value per task (:181)
    logits_q = logits_q.detach()
    return {"weights": weights.detach(), "logits_q": logits_q, "criterions": torch.stack(criterions),
            "argmax": logits_q.argmax(2)}


PROB = ["fs_gd_tim_K5_N3_s2", "fs_gd_tim_K10_N4_s4", "fs_gd_tim_K37_N3_s2"]
VISUAL = ["fs_vis_gd_tim_D512_K10_S4_N3", "fs_vis_gd_tim_D1024_K37_S2_N2", "fs_vis_gd_tim_D768_K100_S1_N1"]


def load_fixture(golden_dir, name):
    """a fixture of tests/golden/make_golden_tim_gd.py as a dict of numpy arrays, the inputs of a visual one regenerated from
    its seed (helpers.visual_fs) and checked against the stored digests"""
    import os

    import numpy as np

    from helpers import visual_fs
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    if "x_q" not in g:
        x_s, _, x_q, _ = visual_fs.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"]), int(g["seed"]),
                                              signal=float(g["signal"]))
        g["x_s"], g["x_q"] = x_s.numpy(), x_q.numpy()
        assert visual_fs.sha(g["x_s"]) == str(g["x_s_sha1"]) and visual_fs.sha(g["x_q"]) == str(g["x_q_sha1"]), name
    return g


def params(g):
    return dict(iters=int(g["iters"]), temp=float(g["temp"]), lr=float(g["lr"]), loss_weights=[float(w) for w in g["loss_weights"]])


def check_within_bounds(weights, logits_q, crit, g):
    """the fixture's own three bounds (derived from the reference's fp32-against-fp64 gap when it was made); every figure is
    printed before it is asserted"""
    import numpy as np
    w_err = float(np.abs(weights - g["weights"]).max())
    l_err = float(np.abs(logits_q - g["logits_q"]).max())
    c_err = float(np.abs(crit / g["criterions"] - 1).max())
    print(f"deviation from the reference: weights {w_err:.3e} (bound {float(g['weights_abs']):.3e}), logits {l_err:.3e} "
          f"(bound {float(g['logits_abs']):.3e}), criterions {c_err:.3e} relative (bound {float(g['criterions_rel']):.3e})")
    assert w_err <= float(g["weights_abs"]), f"weights differ by {w_err} (bound {float(g['weights_abs'])})"
    assert l_err <= float(g["logits_abs"]), f"query logits differ by {l_err} (bound {float(g['logits_abs'])})"
    assert c_err <= float(g["criterions_rel"]), f"criterions differ by {c_err} relative (bound {float(g['criterions_rel'])})"
