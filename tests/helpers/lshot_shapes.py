"""LAPLACIAN_SHOT over a sweep of Q, K, T and knn: the shape table with its seeds, the inputs, a dense float64 restatement of the
bound-update loop for a GIVEN unary term and neighbour lists (so that k_lshot_task's loop is judged apart from the distance
kernels), and the margins that tell a determined comparison from a coin toss.  Nothing here touches the GPU; the conditions
every case must meet are asserted by tests/test_lshot_shapes.py, so that tests/test_gpu_lshot_shapes.py never skips.

What the shapes reach in csrc/tclip_lshot.inc:
  k_lshot_task       a lane keeps ceil(Q / 64) distances in registers (1, a full one, 2, 3, 5, all 16 at kLshotMaxQ = 1024);
                     rows go to 8 wavefronts (Q = 2, 3 leave most idle); the K loops stride by 64 (3, 5 and 16 strides, ragged
                     and full); knn = Q; neighbour lists of 19 and 39; the longest list under the 60 000-byte LDS check
  k_lshot_pairdist   32-row tiles: Q = 31, 32, 33
  k_lshot_normalize  four rows per block: T Q = 325 and T S = 7 * 6 leave the last block part-filled
  probability entry  the distances inside k_lshot_task, serially over D = K up to 1000 and 1024"""
import functools
from collections import namedtuple

import numpy as np
import torch

from helpers import visual_fs, visual_lshot
from oracle import ref_torch

ITERS, LMD = 15, 0.7
NORMS = ("L2N", "UN")
FREEZE_RTOL = 1e-6                   # laplacian_shot.py:165
KNN_MARGIN = 1e-6                    # the threshold of tests/test_gpu_visual_lshot.py, asserted here instead of skipping
MAX_LEFT_OUT = 0.02                  # share of (task, update, query) elements whose logit gap is below tau
BOUND_FACTOR = 4.0                   # tau = 4 s_L, energy bound = 4 s_E + floor

Case = namedtuple("Case", "entry D K shots Q T knn norm iters seed")

# (D, K, shots, Q, T, knn, seed).  The seed is D 1019 + K 7 + Q unless a condition of tests/test_lshot_shapes.py asked for
# another one (marked).  The two smallest tasks: with 65253 and 65254 ref_torch's own energies are 1e-6 and 5e-6 from those of
# the correctly rounded float64 unary term (reference_energy_error), more than the end-to-end comparison allows in all; with two
# or three queries that is the rule (one seed in five meets a quarter of 1e-6 at Q = 2, one in four hundred at Q = 3).
VISUAL = [
    (64, 5, 1, 2, 3, 2, 565253),           # the smallest task: one neighbour, fewer rows than wavefronts (marked: see below)
    (64, 5, 1, 3, 3, 3, 40465254),         # knn = Q (marked: see below)
    (40, 7, 2, 31, 2, 4, 40840),           # k_lshot_pairdist's 32-row tile edge
    (40, 7, 2, 32, 2, 4, 40841),
    (40, 7, 2, 33, 2, 4, 40842),
    (40, 7, 2, 63, 2, 3, 40872),           # one distance register
    (40, 7, 2, 64, 2, 3, 40873),           # a full one
    (40, 7, 2, 65, 5, 3, 40874),           # one lane in the second; T Q = 325
    (96, 10, 1, 128, 2, 5, 98022),         # two full registers
    (96, 10, 1, 129, 2, 5, 98023),         # three
    (33, 130, 1, 75, 2, 3, 34612),         # K in three strides of 64, ragged
    (130, 257, 1, 76, 1, 3, 134345),       # five, ragged
    (64, 1000, 1, 74, 1, 3, 72290),        # sixteen, ragged
    (1024, 1024, 1, 40, 1, 3, 1050664),    # sixteen, full; both limits at once
    (16, 4, 2, 1024, 1, 3, 17356),         # Q at kLshotMaxQ
    (16, 4, 2, 1024, 1, 13, 17356),        # 1024 * 12 * 4 + 8192 = 57 344 bytes of LDS
    (32, 6, 1, 20, 7, 20, 32670),          # knn = Q with 19 neighbours, T = 7
    (8, 3, 1, 300, 1, 40, 8473),           # 39 neighbours over five registers
]
# (K, shots, Q, T, knn, seed), D = K.  The seed is K 31 + Q unless marked.
PROB = [
    (2, 1, 75, 3, 3, 137),
    (63, 1, 40, 2, 3, 1993),
    (64, 2, 65, 2, 3, 102049),             # marked: at 2049 the L2N kNN margin is 2.2e-7
    (65, 1, 75, 2, 5, 102090),             # marked: at 2090 the L2N kNN margin is 2.8e-7
    (129, 1, 128, 2, 3, 4127),
    (512, 1, 76, 1, 3, 15948),
    (1000, 1, 75, 2, 3, 31075),
    (1024, 1, 33, 1, 4, 31777),
]
SHORT = (40, 7, 2, 33, 2, 4, 40842)      # the visual shape that is also run at iters = 1, 2, 3, where `it > 1` decides


def _cases():
    out = [Case("visual", D, K, s, Q, T, knn, norm, ITERS, seed) for D, K, s, Q, T, knn, seed in VISUAL for norm in NORMS]
    out += [Case("prob", K, K, s, Q, T, knn, norm, ITERS, seed) for K, s, Q, T, knn, seed in PROB for norm in NORMS]
    return out


SWEEP = _cases()
SHORT_ITERS = [Case("visual", *SHORT[:6], "L2N", iters, SHORT[6]) for iters in (1, 2, 3)]
ALL = SWEEP + SHORT_ITERS


def case_id(c):
    return f"{c.entry}-D{c.D}-K{c.K}-s{c.shots}-Q{c.Q}-T{c.T}-knn{c.knn}-{c.norm}" + (f"-it{c.iters}" if c.iters != ITERS else "")


def amplifying(c):
    """lmd (knn - 1) > 2.8: a last-place change of Y0 grows from update to update, so an end-to-end comparison with another
    host's fp32 start decides nothing; such a case is judged through the loop in isolation alone"""
    return LMD * (c.knn - 1) > 2.8 + 1e-12


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """(x_q (T,Q,D), x_s (T,S,D), y_s (T,S) int64), torch on the host"""
    if c.entry == "visual":
        x_s, y_s, x_q = visual_fs.random_tasks(c.T, c.K, c.D, c.shots, c.seed, n_query=c.Q, scale=c.D ** -0.5)
        return x_q, x_s, y_s
    from tclip_amd import synth
    x_q, _ = synth.make_query_tasks(c.T, c.K, c.seed, n_query=c.Q, k_eff=min(4, c.K))
    x_s, y_s = synth.make_support(c.T, c.K, c.shots, c.seed)
    return x_q, x_s, y_s.squeeze(2)


def params(c):
    return dict(iters=c.iters, knn=c.knn, lmd=LMD, norm_type=c.norm)


@functools.lru_cache(maxsize=None)
def run_reference(c):
    """oracle/ref_torch.py's restatement of the reference, computed once per case and never written to"""
    x_q, x_s, y_s = make_inputs(c)
    t = ref_torch.run_laplacian_shot(x_q, x_s, y_s, torch.zeros(c.T, c.Q, dtype=torch.long), n_class=c.K, **params(c))
    for v in t.values():
        v.setflags(write=False)
    return t


def run_engine(c):
    """the engine's (unary, neighbours, preds_iter, energies) as numpy arrays"""
    from tclip_amd import engine
    x_q, x_s, y_s = (a.cuda() for a in make_inputs(c))
    if c.entry == "visual":
        out = engine.run_laplacian_shot_visual(x_q, x_s, y_s, n_class=c.K, **params(c))
    else:
        out = engine.run_laplacian_shot(x_q, x_s, y_s, **params(c))
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


# ---- the loop, restated -------------------------------------------------------------------------------------------------

def _softmax(a):
    a = a - a.max(axis=1)[:, None]
    e = np.exp(a)
    return e / e.sum(axis=1)[:, None]


def _jitter(y32, seed):
    """every element one fp32 place up or down, the direction from a seeded coin"""
    up = np.random.default_rng(seed).integers(0, 2, y32.shape).astype(bool)
    return np.where(up, np.nextafter(y32, np.float32(2)), np.nextafter(y32, np.float32(-1))).astype(np.float32)


STARTS = ("numpy32", "float64", "numpy32~1", "numpy32~2", "float64~1", "float64~2")


def start_y(unary32, start):
    """Y0 (Q,K) fp32: 'numpy32' = numpy's fp32 normalize(-unary) as the reference computes it (laplacian_shot.py:145),
    'float64' = the float64 softmax rounded to fp32, '<base>~<seed>' = that base moved one fp32 place per element"""
    base, _, seed = start.partition("~")
    if base == "numpy32":
        # the reference's unary term is a transposed view (laplacian_shot.py:242), so numpy sums its rows element by element
        y = np.ascontiguousarray(_softmax(np.asfortranarray(-np.asarray(unary32, dtype=np.float32))))
        assert y.dtype == np.float32
    elif base == "float64":
        y = _softmax(-np.asarray(unary32, dtype=np.float64)).astype(np.float32)
    else:
        raise ValueError(start)
    return _jitter(y, int(seed)) if seed else y


def restated_loop(unary32, neighbours, lmd, iters, start="numpy32", freeze=True):
    """laplacian_shot.py:142-171 for one task in dense float64 numpy, from a GIVEN unary term (Q,K) fp32 and neighbour lists
    (Q,nn): Y <- softmax(-unary + lmd W Y), E = sum Y log max(Y, 1e-20) + unary Y - lmd (W Y) Y with the new Y on both sides of
    W, the break once |E - E_old| <= 1e-6 |E_old| after the third update, the last values repeated from then on.
    `start`: see start_y.  freeze=False runs every update (what the sensitivities compare).
    Returns dict(energies (iters,), preds_iter (iters,Q), frozen_at, logits (iters,Q,K): -unary + lmd W Y_old of every update,
    gaps (iters,Q): the distance between a query's two largest logits, abs_terms (iters,): the sum of the absolute values of the
    energy's Q K terms)."""
    u = np.asarray(unary32, dtype=np.float64)
    nbr = np.asarray(neighbours, dtype=np.int64)
    Q, K = u.shape
    y = start_y(unary32, start).astype(np.float64)
    out = {"energies": [], "preds_iter": [], "logits": [], "gaps": [], "abs_terms": []}
    old_e, frozen_at = np.inf, -1
    for it in range(iters):
        logits = -u + lmd * y[nbr].sum(axis=1)
        y = _softmax(logits)
        terms = y * np.log(np.maximum(y, 1e-20)) + u * y - lmd * y[nbr].sum(axis=1) * y
        e = terms.sum()
        top = np.partition(logits, K - 2, axis=1)[:, K - 2:]
        out["energies"].append(e)
        out["preds_iter"].append(np.argmax(logits, axis=1))
        out["logits"].append(logits)
        out["gaps"].append(top[:, 1] - top[:, 0])
        out["abs_terms"].append(np.abs(terms).sum())
        if freeze and it > 1 and abs(e - old_e) <= FREEZE_RTOL * abs(old_e):
            frozen_at = it
            for v in out.values():
                v.extend([v[-1]] * (iters - it - 1))
            break
        old_e = e
    out = {k: np.asarray(v) for k, v in out.items()}
    out["frozen_at"] = frozen_at
    return out


def frozen_from_energies(e):
    """the first update from which the values of e (iters,) repeat, -1 if that is the last one (a break taken in the last
    update writes what no break writes)"""
    e = np.asarray(e)
    f = len(e) - 1
    while f > 0 and e[f - 1] == e[-1]:
        f -= 1
    return -1 if f == len(e) - 1 else f


def freeze_margins(energies, frozen_at):
    """(iters,): | |E - E_old| / |E_old| - 1e-6 | at the updates 2 .. freeze, how far the break's comparison is from tipping
    there; inf at the updates where nothing is compared"""
    e = np.asarray(energies, dtype=np.float64)
    last = frozen_at if frozen_at >= 0 else len(e) - 1
    out = np.full(len(e), np.inf)
    for i in range(2, last + 1):
        out[i] = abs(abs(e[i] - e[i - 1]) / abs(e[i - 1]) - FREEZE_RTOL)
    return out


Judged = namedtuple("Judged", "loop s_e s_l tau floor bound bound_it freeze_margin freeze_slack left_out")


def judge_task(unary32, neighbours, lmd, iters):
    """the restated loop of one task from the reference's start, and what a last-place change of that start does to it:
    s_e   largest relative energy difference, s_l largest absolute logit difference between the 'numpy32' run and every other
          start of STARTS, all run without the break and compared over the updates up to the break of the 'numpy32' run
    tau   4 s_l: below that gap between its two largest logits a query's assignment is not determined
    floor (iters,) Q K 2^-53 sum|terms| / |E|: the fp64 reordering bound of a sum of Q K terms
    bound max over the updates of 4 s_e + floor: what the engine's energies are held to
    bound_it  (iters,) the same with the sensitivity of update `it` alone.  Where lmd (knn - 1) >> 1 a last-place change of Y0
          grows over the first updates and dies out as the iteration settles (at knn = Q = 20: 2e-6 at update 3, 2e-10 at
          update 5), and the break is taken after it has: the comparison of update `it` reads E[it] and E[it-1] only
    freeze_margin  min over the updates 2 .. freeze of | |E - E_old| / |E_old| - 1e-6 |
    freeze_slack   min over those updates of that margin / (4 max(bound_it[it], bound_it[it-1])): at 1 and above the break of
          an engine whose energies are within twice bound_it of these is the one taken here
    left_out  (iters,Q) bool: gap < tau"""
    loop = restated_loop(unary32, neighbours, lmd, iters)
    base = restated_loop(unary32, neighbours, lmd, iters, freeze=False)
    upto = (loop["frozen_at"] if loop["frozen_at"] >= 0 else iters - 1) + 1
    s_e_it, s_l = np.zeros(iters), 0.0
    for start in STARTS[1:]:
        other = restated_loop(unary32, neighbours, lmd, iters, start, freeze=False)
        s_e_it[:upto] = np.maximum(s_e_it[:upto], np.abs(other["energies"][:upto] / base["energies"][:upto] - 1))
        s_l = max(s_l, float(np.abs(other["logits"][:upto] - base["logits"][:upto]).max()))
    s_e = float(s_e_it.max())
    Q, K = np.asarray(unary32).shape
    floor = Q * K * 2.0 ** -53 * loop["abs_terms"] / np.abs(loop["energies"])
    tau = BOUND_FACTOR * s_l
    bound_it = BOUND_FACTOR * s_e_it + floor
    margins = freeze_margins(loop["energies"], loop["frozen_at"])
    slack = min((margins[i] / (4 * max(bound_it[i], bound_it[i - 1])) for i in range(2, upto)), default=np.inf)
    return Judged(loop, s_e, s_l, tau, floor, float((BOUND_FACTOR * s_e + floor).max()), bound_it, float(margins.min()), float(slack),
                  loop["gaps"] < tau)


# ---- the distance side, restated in float64 -------------------------------------------------------------------------------

def normalised64(x, norm):
    z = x.double().numpy()
    return z / np.sqrt((z * z).sum(axis=2, keepdims=True)) if norm == "L2N" else z


def scale2(c):
    """max |row|^2 over the rows the distances are taken between: 1 after L2N"""
    x_q, x_s, _ = make_inputs(c)
    return 1.0 if c.norm == "L2N" else float(torch.cat([x_s, x_q], 1).double().square().sum(2).max())


def unary64(c):
    """normalisation, class means and squared distances in float64 numpy from the fp32 inputs -> (T,Q,K) float64"""
    x_q, x_s, y_s = make_inputs(c)
    z_q, z_s = normalised64(x_q, c.norm), normalised64(x_s, c.norm)
    out = np.empty((c.T, c.Q, c.K))
    for t in range(c.T):
        proto = np.zeros((c.K, c.D))
        np.add.at(proto, y_s[t].numpy(), z_s[t])
        proto /= np.bincount(y_s[t].numpy(), minlength=c.K)[:, None]
        for q in range(c.Q):
            d = proto - z_q[t, q]
            out[t, q] = (d * d).sum(axis=1)
    return out


END_TO_END_RTOL = 1e-6               # energies against ref_torch, the bound of tests/test_laplacian_shot.py


def reference_energy_error(c):
    """max relative distance of ref_torch's energies from those of the float64 loop run on the float64 unary term rounded to
    fp32 (ref_torch's own neighbour lists): what the fp32 roundings of the reference's unary term alone do to the energies.
    With two or three queries nothing averages out and this alone can pass END_TO_END_RTOL; an end-to-end comparison judges
    the engine only where it leaves room."""
    t, u = run_reference(c), unary64(c).astype(np.float32)
    return max(float(np.abs(restated_loop(u[k], t["neighbours"][k], LMD, c.iters)["energies"] / t["ent_energy"][k] - 1).max())
               for k in range(c.T))


def knn_margin(c):
    """visual_lshot.knn_margin; with knn = Q every other query is a neighbour and there is nothing to tell apart"""
    return np.inf if c.knn == c.Q else visual_lshot.knn_margin(make_inputs(c)[0], c.knn, c.norm)


def neighbours64(c):
    """(T,Q,knn-1) sorted: the nearest other queries by float64 distances of rows normalised in float64 and rounded to fp32 -
    rows that differ from numpy's fp32-normalised ones (and from the engine's) in the last place"""
    z = normalised64(make_inputs(c)[0], c.norm).astype(np.float32).astype(np.float64)
    out = np.empty((c.T, c.Q, c.knn - 1), dtype=np.int64)
    for t in range(c.T):
        d2 = np.stack([((z[t] - z[t, q]) ** 2).sum(axis=1) for q in range(c.Q)])
        np.fill_diagonal(d2, np.inf)
        out[t] = np.sort(np.argsort(d2, axis=1, kind="stable")[:, :c.knn - 1], axis=1)
    return out
