"""Shapes, inputs, runners and conditions of tests/test_gpu_visual_method_shapes.py and tests/test_visual_method_shapes.py: the
six methods on visual features (zero-shot SOFT_KMEANS, HARD_KMEANS, EM_GAUSSIAN, EM_GAUSSIAN_COV from a given u0; few-shot
PADDLE and BD-CSPN) through tclip_amd.engine against the torch restatements of tests/helpers/visual.py, visual_cov.py and
visual_fs.py, away from the existing sweeps' Q = 75 and T <= 2.

A zero-shot shape is (D, K, Q, T): row length, class count, query rows per task, tasks.  A few-shot shape is (D, K, shots, Q, T);
shots = 0 stands for the unbalanced support set, class k with 1 + k % 3 members.  The largest torch temporary, T Q K D floats, is
2.9 M floats (33, 130, 76, 9), far under the 200 MB the sweep allows itself."""
import torch

from helpers import visual, visual_cov, visual_fs
from helpers.prob_shapes import CRIT_RTOL, bit_differences, criterion_gap, rel_err  # noqa: F401

ZERO_SHOT = ("skm", "hkm", "emg", "cov")
FEW_SHOT = ("paddle", "bdcspn")
# the `live` / `need` masks and the v term act from the second iteration on; the third sees what the second left
ITERS = {"skm": 3, "hkm": 3, "emg": 3, "cov": 3, "paddle": 2, "bdcspn": 1}
TEMPERATURE, PADDLE_LAMBD, BDCSPN_TEMP = 30.0, 7.5, 10.0
NORM_TYPES = ("L2N", "CL2N", "UN")
INTERIOR_MIN = 0.005             # of u after the first iteration, strictly between 1e-6 and 1 - 1e-6
DEAD_EPS = 1e-15

# k_vis_mstats takes kVisRows = 16 whole class rows per block and walks torch's cascade over Q in blocks of 16 rows, with a
# second level every 256 and a third every 4096; k_vis_dist deals the queries to 16 wavefronts.  K = 24: one 16-row group in
# k_vis_mstats and eight rows in k_vis_mstats_one.  Q: below, at and past one block (15, 16, 17), two blocks (31, 32, 33), the
# neighbours of the existing sweeps' 75, the second level (255, 256, 257) and a first-level dump behind it (272).
# 288: up to 272 rows a cascade without its second level adds the same numbers in an order that rounds the same - at 256, 257
# and 272 the sum is b17 + B, B the first 256 rows' and b17 the seventeenth block's, with or without the dump at 256 (tried: such
# a kernel passed those cases) -; with two blocks behind the dump it is (b17 + b18) + B against (B + b17) + b18.
# D = 7: K D = 168 columns end in eight 4-way row-sum columns, and k_vis_dist takes its D < 8 path.
ROW_QS = (1, 3, 15, 16, 17, 31, 32, 33, 74, 76, 255, 256, 257, 272, 288)
ZS_ROWS = [(d, 24, q, 2) for d in (40, 7) for q in ROW_QS]
# the cascade's third level: K D = 128 columns, all of them in the one group of k_vis_mstats
ZS_LEVEL3 = [(8, 16, q, 1) for q in (4096, 4097, 4112)]
# rows of more than one chunk of k_vis_dist (512 elements; 256 with covariances), where the barriers sit inside the query loop:
# one full group of 16 queries, and a last group with one working wavefront
ZS_CHUNKS = [(520, 72, 16, 2), (520, 72, 17, 2), (1024, 24, 17, 2)]
COV_CHUNKS = [(300, 24, 17, 2)]
# tasks: one, a full group of eight, a part-filled second and third one; K = 130: three k_vis_dist tiles, two classes in the last
ZS_TASKS = [(33, 72, 75, t) for t in (1, 8, 9, 17)] + [(33, 130, 76, 9)]
ZS_ALL = ZS_ROWS + ZS_LEVEL3 + ZS_CHUNKS + ZS_TASKS

PADDLE_SHAPES = ([(40, 24, 2, q, 2) for q in (1, 15, 16, 17, 76, 255, 256, 257, 272, 288)] + [(520, 24, 1, 17, 2), (8, 16, 1, 4097, 1)]
                 + [(33, 72, 1, 75, t) for t in (1, 9, 17)])
# S = 10: q = 246, 247 and 278 give 256, 257 and 288 augmented rows.  K = 5 has no group of 16 whole rows, so these run
# k_vis_mstats_one alone; (40, 24, 1, 264, 2), 288 augmented rows again, runs k_vis_mstats in mode 3 past its second level.
BDCSPN_SHAPES = [(40, 5, 2, q, 2) for q in (1, 17, 246, 247, 278)] + [(40, 24, 1, 264, 2), (33, 72, 1, 75, 9)]
# k_vis_support_stats replays the cascade's dumps between the members of a class: 1, 2 and 3 members in a shuffled order
UNBALANCED = [(40, 24, 0, 17, 2), (513, 24, 0, 17, 2)]
FS_CASES = ([("paddle", s) for s in PADDLE_SHAPES + UNBALANCED] + [("bdcspn", s) for s in BDCSPN_SHAPES + UNBALANCED])

# structured tasks whose u0 has the columns of classes 16..31 and 64..127 zeroed: a whole 16-row group of k_vis_mstats and a whole
# 64-class tile of k_vis_dist are dead from the start.  At (40, 130, 300, 2) and (7, 130, 75, 3) some planted class comes back to
# life in the restatement, so those are not used.
PLANTED = [(40, 130, 75, 2), (40, 130, 17, 2), (520, 130, 16, 2)]
PLANTED_DEAD = list(range(16, 32)) + list(range(64, 128))
PLANTED_METHODS = ("skm", "emg", "cov")

# HARD_KMEANS must leave a cluster dead after the first iteration (mode 1's `r * 0.0f` rows).  At D = 40, K = 24, Q >= 74 the stated
# inputs leave none: every centroid is the mean of three or more points of norm about 2, each point is nearer to its own
# cluster's mean (about 4 (1 - 1/n) squared) than to any other (4 + 4/n), and neither another seed nor another scale of x
# (k-means does not see it) or of u0 (8, 4, 2, 1 probed: no dead cluster at Q >= 255) changes that.  There HARD_KMEANS, and it
# alone, starts from the same u0 with two columns zeroed and the rows renormalised - one class of k_vis_mstats's 16-row group, one
# of k_vis_mstats_one's rows: their centroids are written as 0 in the first iteration (4 from every point) and win no query.
HKM_ZEROED_COLUMNS = (5, 20)
HKM_ZEROED_AT = [(40, 24, q, 2) for q in (74, 76, 255, 256, 257, 272, 288)]


def shape_id(shape):
    if len(shape) == 4:
        return "D{}_K{}_Q{}_T{}".format(*shape)
    return "D{}_K{}_s{}_Q{}_T{}".format(shape[0], shape[1], shape[2] or "123", shape[3], shape[4])


def case_id(case):
    return case[0] + "-" + shape_id(case[1])


def norm_type_of(case):
    """BD-CSPN's three normalisations, cycled over its cases"""
    return NORM_TYPES[[c for c in FS_CASES if c[0] == "bdcspn"].index(case) % 3]


def lambd_of(shape):
    return int(shape[1] / 5) * shape[2]


def make_inputs(shape):
    """zero-shot -> dict(x_q (T,Q,D), u0 (T,Q,K)); few-shot -> dict(x_q, x_s (T,S,D), y_s (T,S) int64); CPU tensors, the seed
    from the shape.  Rows are randn * 2 / sqrt(D): squared distances of a few units, so that the responsibilities are not all 0
    and 1 (with randn * 3 they are, from D of a few hundred on)."""
    if len(shape) == 4:
        D, K, Q, T = shape
        gen = torch.Generator().manual_seed(((D * 1031 + K) * 131 + Q) * 7 + T)
        x_q = torch.randn(T, Q, D, generator=gen) * (2.0 / D ** 0.5)
        return {"x_q": x_q, "u0": (torch.randn(T, Q, K, generator=gen) * 8).softmax(-1)}
    D, K, shots, Q, T = shape
    seed = (((D * 1031 + K) * 131 + Q) * 7 + T) * 5 + shots
    scale = 2.0 / D ** 0.5
    if shots:
        x_s, y_s, x_q = visual_fs.random_tasks(T, K, D, shots, seed, n_query=Q, scale=scale)
    else:
        gen = torch.Generator().manual_seed(seed)
        members = torch.cat([torch.full((1 + k % 3,), k) for k in range(K)])
        S = members.numel()
        x_s = torch.randn(T, S, D, generator=gen) * scale
        x_q = torch.randn(T, Q, D, generator=gen) * scale
        y_s = torch.stack([members[torch.randperm(S, generator=gen)] for _ in range(T)])
    return {"x_q": x_q, "x_s": x_s, "y_s": y_s}


def make_planted(shape):
    """-> dict(x_q, u0): visual.make_tasks's structured tasks, the text-prompt u0 with the planted columns zeroed and the rows
    renormalised"""
    D, K, Q, T = shape
    x_q, _, text = visual.make_tasks(T, K, D, 7 * K + Q, n_query=Q)
    u0 = visual.reference_init(x_q, text, 30)
    u0[:, :, PLANTED_DEAD] = 0.0
    return {"x_q": x_q, "u0": u0 / u0.sum(-1, keepdim=True)}


def u0_of(method, shape, inp):
    """the method's initial responsibilities: the shape's u0, but for HARD_KMEANS at HKM_ZEROED_AT"""
    if method != "hkm" or shape not in HKM_ZEROED_AT:
        return inp["u0"]
    u0 = inp["u0"].clone()
    u0[:, :, list(HKM_ZEROED_COLUMNS)] = 0.0
    return u0 / u0.sum(-1, keepdim=True)


def bdcspn_rows(inp):
    """off-centre, so that eta and the CL2N mean are not noise around zero"""
    return inp["x_s"] + 0.5, inp["x_q"] + 0.25


def run_engine(method, shape, inp, iters=None, n_batches=1, norm_type="L2N"):
    """-> dict of CPU tensors, named as run_reference names them"""
    from tclip_amd import engine
    it = ITERS[method] if iters is None else iters
    dev = "cuda:0"
    K = shape[1]
    if method in ZERO_SHOT:
        x, u0 = inp["x_q"].to(dev), u0_of(method, shape, inp).to(dev)
    if method == "skm":
        out = dict(zip(("u", "w", "preds"), engine.run_soft_kmeans_visual(x, u0, iters=it, temperature=TEMPERATURE)))
    elif method == "hkm":
        out = dict(zip(("u", "w", "preds", "criterions"), engine.run_hard_kmeans_visual(x, u0, iters=it, n_batches=n_batches)))
    elif method == "emg":
        out = dict(zip(("u", "v", "w", "preds"),
                       engine.run_em_gaussian_visual(x, u0, iters=it, temperature=TEMPERATURE, lambd=lambd_of(shape))))
    elif method == "cov":
        out = dict(zip(("u", "v", "w", "s", "preds"), engine.run_em_gaussian_cov_visual(x, u0, iters=it, lambd=lambd_of(shape))))
    elif method == "paddle":
        out = dict(zip(("u", "v", "w", "preds"), engine.run_paddle_visual(inp["x_q"].to(dev), inp["x_s"].to(dev), inp["y_s"].to(dev),
                                                                          n_class=K, iters=it, lambd=PADDLE_LAMBD)))
    else:
        x_s, x_q = bdcspn_rows(inp)
        out = dict(zip(("w", "u", "preds"), engine.run_bdcspn_visual(x_q.to(dev), x_s.to(dev), inp["y_s"].to(dev), n_class=K,
                                                                     temp=BDCSPN_TEMP, norm_type=norm_type)))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def run_reference(method, shape, inp, iters=None, log=torch.log, dtype=torch.float32, norm_type="L2N", trail=None):
    """the torch restatement in `dtype`; BD-CSPN's rectified prototypes go by the name `w` like every other method's centroids;
    HARD_KMEANS's criterions (1, iters) as the engine lays one batch out.  `trail`: a list that receives u after every iteration."""
    K = shape[1]
    it = ITERS[method] if iters is None else iters
    trail = [] if trail is None else trail
    if method in ZERO_SHOT:
        x, u = inp["x_q"].to(dtype), u0_of(method, shape, inp).to(dtype)
    if method == "skm":
        w = None
        for _ in range(it):
            u, w, _ = visual.reference_step("soft_kmeans", x, u, w=w, T=TEMPERATURE)
            trail.append(u)
        out = {"u": u, "w": w, "preds": u.argmax(2)}
    elif method == "hkm":
        crit = []
        for _ in range(it):
            u_old = u
            u, w, _ = visual.reference_step("hard_kmeans", x, u.clone())
            crit.append((u_old - u).norm(dim=(1, 2)).mean(0))
            trail.append(u)
        out = {"u": u, "w": w, "preds": u.argmax(2), "criterions": torch.stack(crit).view(1, -1)}
    elif method == "emg":
        w = v = None
        for _ in range(it):
            u, w, v = visual.reference_step("em_gaussian", x, u, w=w, v=v, T=TEMPERATURE, lambd=lambd_of(shape), log=log)
            trail.append(u)
        out = {"u": u, "v": v, "w": w, "preds": u.argmax(2)}
    elif method == "cov":
        v = torch.zeros(u.shape[0], K, dtype=dtype)
        w, s = visual_cov.init(x, u)
        for _ in range(it):
            u, v, w, s = visual_cov.step(x, u, v, w, s, lambd_of(shape), log)
            trail.append(u)
        out = {"u": u, "v": v, "w": w, "s": s, "preds": u.argmax(2)}
    elif method == "paddle":
        w = v = None
        for _ in range(it):
            u, v, w = visual_fs.paddle_step(inp["x_s"].to(dtype), inp["x_q"].to(dtype), inp["y_s"], K, PADDLE_LAMBD, w=w, v=v, log=log)
            trail.append(u)
        out = {"u": u, "v": v, "w": w, "preds": u.argmax(2)}
    else:
        x_s, x_q = bdcspn_rows(inp)
        p, u, preds = visual_fs.bdcspn_pass(x_s.to(dtype), x_q.to(dtype), inp["y_s"], K, BDCSPN_TEMP, norm_type)
        trail.append(u)
        out = {"w": p, "u": u, "preds": preds}
    return out


def interior_fraction(u):
    return float(((u > 1e-6) & (u < 1 - 1e-6)).double().mean())


def unmet_conditions(method, shape, out, trail, planted=False):
    """what keeps a comparison with this restatement's run from passing vacuously -> the list of the conditions it misses (empty:
    none); prints the figures.  Every output finite; SOFT_KMEANS, EM_GAUSSIAN, PADDLE: at least INTERIOR_MIN of u after the first
    iteration is neither 0 nor 1; HARD_KMEANS at K >= 24: a dead cluster for mode 1's `r * 0.0f` rows and at least two live ones,
    counted over the call's (task, cluster) pairs; planted cases: the planted classes are dead after every iteration."""
    name = f"{method} {shape_id(shape)}"
    missed = [f"{name}: {k} is not finite" for k, a in out.items() if a.is_floating_point() and not bool(torch.isfinite(a).all())]
    if method in ("skm", "emg", "paddle") and not planted:
        frac = interior_fraction(trail[0])
        print(f"{name}: {100 * frac:.2f} % of u is interior after the first iteration")
        if not frac >= INTERIOR_MIN:
            missed.append(f"{name}: {100 * frac:.3f} % of u is interior after the first iteration")
    if method == "hkm" and shape[1] >= 24:
        sizes = trail[0].sum(1)
        dead, live = int((sizes == 0).sum()), int((sizes > 0).sum())
        print(f"{name}: {live} live and {dead} dead clusters after the first iteration")
        if dead < 1 or live < 2:
            missed.append(f"{name}: {live} live and {dead} dead clusters after the first iteration")
    if planted:
        sizes = [float(u[:, :, PLANTED_DEAD].sum(1).max()) for u in trail]
        print(f"{name}: the largest planted cluster after every iteration: {sizes}")
        if not all(s <= DEAD_EPS for s in sizes):
            missed.append(f"{name}: a planted cluster came to life: {sizes}")
        alive = [k for k in range(shape[1]) if k not in PLANTED_DEAD]
        if not all(bool((u[:, :, alive].sum(1) > DEAD_EPS).any()) for u in trail):
            missed.append(f"{name}: no live cluster is left")
    return missed


# the outputs that are continuous functions of the inputs after ONE iteration; one-hot u and predictions are not
CONTINUOUS = {"skm": ("w", "u"), "hkm": ("w",), "emg": ("w", "u", "v"), "cov": ("w", "s", "u", "v"), "paddle": ("w", "u", "v"),
              "bdcspn": ("w", "u")}
