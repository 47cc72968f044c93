"""The fs_vis_lshot_* fixtures (tests/golden/make_golden_visual_lshot.py) and the kNN margin of a set of LAPLACIAN_SHOT tasks:
what tells a comparison of neighbour lists apart from a coin toss."""
import os

import numpy as np

from helpers import visual_fs

VISUAL = ["fs_vis_lshot_D512_K10_S4_N3", "fs_vis_lshot_D1024_K37_S2_N2", "fs_vis_lshot_D768_K100_S1_N1_un"]


def load_fixture(golden_dir, name):
    """a fixture as a dict of numpy arrays, its inputs regenerated from the seed and checked against the stored digests"""
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    x_s, _, x_q, _ = visual_fs.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"]), int(g["seed"]), signal=float(g["signal"]))
    g["x_s"], g["x_q"] = x_s.numpy(), x_q.numpy()
    assert visual_fs.sha(g["x_s"]) == str(g["x_s_sha1"]) and visual_fs.sha(g["x_q"]) == str(g["x_q_sha1"]), name
    return g


def knn_margin(x_q, knn, norm_type):
    """x_q (N,Q,D) torch -> min over tasks and queries of the relative difference between the squared distances (fp64, rows
    normalised as the method normalises them) to the (knn-1)-th and the knn-th nearest other query"""
    z = x_q.double().numpy()
    if norm_type == "L2N":
        z = z / np.linalg.norm(z, axis=2, keepdims=True)
    worst = np.inf
    for zt in z:
        sq = (zt * zt).sum(1)
        d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * zt @ zt.T, 0.0) if zt.shape[1] > 256 else ((zt[:, None] - zt[None]) ** 2).sum(-1)
        np.fill_diagonal(d2, np.inf)
        s = np.sort(d2, axis=1)
        worst = min(worst, float(((s[:, knn - 1] - s[:, knn - 2]) / s[:, knn - 1]).min()))
    return worst
