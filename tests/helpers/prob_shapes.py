"""Shapes, inputs, runners and the two comparisons of tests/test_gpu_prob_method_shapes.py: the seven methods on probability
features (SOFT_KMEANS, HARD_KMEANS, KL_KMEANS, EM_GAUSSIAN, EM_GAUSSIAN_COV, PADDLE, BD-CSPN) through tclip_amd.engine against
the torch restatements of oracle/ref_torch.py, away from the fixtures' K <= 397, Q = 75 and T <= 6.

A shape is (K, Q, T, shots): class count = row length, query rows per task, tasks, support rows per class (S = K * shots)."""
import numpy as np
import torch

from oracle import ref_torch

ZERO_SHOT = ("skm", "hkm", "klk", "emg", "cov")
FEW_SHOT = ("paddle", "bdcspn")
METHODS = ZERO_SHOT + FEW_SHOT
# the `live` / `need` masks and the v term only take effect from the second iteration on, and the two Gaussian methods are the
# ones that lose clusters: three iterations for them, two for the rest (BD-CSPN is one pass)
ITERS = {"skm": 2, "hkm": 2, "klk": 2, "emg": 3, "cov": 3, "paddle": 2, "bdcspn": 1}
TEMPERATURE, PADDLE_LAMBD, BDCSPN_TEMP, CRIT_RTOL = 30, 2.5, 30.0, 5e-6

# Both sides of the LDS-tile kernels' limit (K <= 511) and both ends of every dispatch_E bucket of ceil(K / 32) registers behind
# it (16 | 17..20 | 21..24 | 25..28 | 29..32), with a ragged last register at 1000 and 1023.
CLASS_SWEEP = [(k, 75, 1, 1) for k in (511, 512, 513, 640, 641, 768, 769, 896, 897, 1000, 1023, 1024)]
# Off the special-cased 75 rows: its neighbours 74 and 76, the cascade's dump after every 16 rows (15, 16, 17), below the
# eight-row groups (1, 3), past one hundred.  K = 7: the one-row statistics kernel alone and rows below the tile kernels' 32
# elements; 40: eight-row groups only; 100: both, with two 64-class tiles; 600: past the tile kernels (T = 2 there, too).
ROW_SWEEP = [(k, q, 2, 1) for k in (7, 40, 100) for q in (1, 3, 15, 16, 17, 74, 76, 128)] + [(600, q, 2, 1) for q in (3, 76)]
# An augmented set S + Q of exactly 75 rows: the 75-row kernels in BD-CSPN's PlainQuotient mode.  PADDLE and BD-CSPN only.
AUG75 = [(10, 55, 2, 2), (5, 60, 3, 3), (37, 38, 2, 1)]
# Blocks are dealt to tasks in groups of eight: a full group, a part-filled second and third one.  K = 72: two 64-column
# tiles with a partial last one; K = 8: the smallest K of the column kernel.
TASK_SWEEP = [(72, 75, t, 1) for t in (1, 8, 9, 17)] + [(8, 75, 9, 1)]
ALL_SEVEN = CLASS_SWEEP + ROW_SWEEP + TASK_SWEEP


def shape_id(shape):
    return "K{}_Q{}_T{}_s{}".format(*shape)


def make_inputs(shape):
    """-> dict(x_q for the zero-shot methods; xf_q, x_s, y_s for the few-shot pair), CPU tensors, the seed from the shape"""
    from tclip_amd import synth
    K, Q, T, shots = shape
    seed = ((K * 1031 + Q) * 131 + T) * 7 + shots
    x_q, _ = synth.make_query_tasks(T, K, seed=seed, n_query=Q)
    xf_q, _ = synth.make_query_tasks(T, K, seed=seed + 1, n_query=Q, k_eff=min(4, K))
    x_s, y_s = synth.make_support(T, K, shots, seed=seed)
    return {"x_q": x_q, "xf_q": xf_q, "x_s": x_s, "y_s": y_s}


def lambd_of(shape):
    return int(shape[0] / 5) * shape[1]


def run_engine(method, shape, inp, iters=None, n_batches=1):
    """-> dict of CPU tensors, named as run_reference names them"""
    from tclip_amd import engine
    it = ITERS[method] if iters is None else iters
    dev = "cuda:0"
    if method in ZERO_SHOT:
        x = inp["x_q"].to(dev)
    else:
        x, xs, ys = inp["xf_q"].to(dev), inp["x_s"].to(dev), inp["y_s"].squeeze(2).to(dev)
    if method == "skm":
        out = dict(zip(("u", "w", "preds"), engine.run_soft_kmeans(x, iters=it, temperature=TEMPERATURE)))
    elif method == "hkm":
        out = dict(zip(("u", "w", "preds", "criterions"), engine.run_hard_kmeans(x, iters=it, n_batches=n_batches)))
    elif method == "klk":
        out = dict(zip(("u", "w", "preds", "criterions"), engine.run_kl_kmeans(x, iters=it, n_batches=n_batches)))
    elif method == "emg":
        out = dict(zip(("u", "v", "w", "preds"), engine.run_em_gaussian(x, iters=it, temperature=TEMPERATURE, lambd=lambd_of(shape))))
    elif method == "cov":
        out = dict(zip(("u", "v", "w", "s", "preds"), engine.run_em_gaussian_cov(x, iters=it, lambd=lambd_of(shape))))
    elif method == "paddle":
        out = dict(zip(("u", "v", "w", "preds"), engine.run_paddle(x, xs, ys, iters=it, lambd=PADDLE_LAMBD)))
    else:
        out = dict(zip(("w", "u", "preds"), engine.run_bdcspn(x, xs, ys, temp=BDCSPN_TEMP, norm_type="L2N")))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def run_reference(method, shape, inp, iters=None, log=torch.log, bmm=None, dtype=torch.float32):
    """the torch restatement; BD-CSPN's rectified prototypes go by the name `w` like every other method's centroids;
    criterions (1, iters) as the engine lays one batch out"""
    K = shape[0]
    it = ITERS[method] if iters is None else iters
    kw = {"n_class": K, "dtype": dtype}
    if method == "skm":
        t = ref_torch.run_soft_kmeans(inp["x_q"], iters=it, temperature=TEMPERATURE, **kw)
        out = {"u": t["u"], "w": t["w"], "preds": t["u"].argmax(2)}
    elif method in ("hkm", "klk"):
        t = (ref_torch.run_hard_kmeans(inp["x_q"], iters=it, **kw) if method == "hkm" else
             ref_torch.run_kl_kmeans(inp["x_q"], iters=it, log=log, bmm=bmm, **kw))
        out = {"u": t["u"], "w": t["w"], "preds": t["labels"][-1], "criterions": t["criterions"].view(1, -1)}
    elif method == "emg":
        t = ref_torch.run_em_gaussian(inp["x_q"], iters=it, temperature=TEMPERATURE, lambd=lambd_of(shape), log=log, **kw)
        out = {"u": t["u"], "v": t["v"], "w": t["w"], "preds": t["argmax"][-1]}
    elif method == "cov":
        t = ref_torch.run_em_gaussian_cov(inp["x_q"], iters=it, lambd=lambd_of(shape), log=log, **kw)
        out = {"u": t["u"], "v": t["v"], "w": t["w"], "s": t["s"], "preds": t["argmax"][-1]}
    elif method == "paddle":
        t = ref_torch.run_paddle(inp["xf_q"], inp["x_s"], inp["y_s"], iters=it, lambd=PADDLE_LAMBD, log=log, **kw)
        out = {"u": t["u"], "v": t["v"], "w": t["w"], "preds": t["argmax"][-1]}
    else:
        t = ref_torch.run_bdcspn(inp["xf_q"], inp["x_s"], inp["y_s"], temp=BDCSPN_TEMP, norm_type="L2N", **kw)
        out = {"w": t["prototypes"], "u": t["u"], "preds": t["preds"]}
    return out


def bit_differences(got, want):
    """-> {tensor: number of elements whose bits differ} over the float tensors and the predictions (criterions apart)"""
    bad = {}
    for k, b in want.items():
        if k == "criterions":
            continue
        a = got[k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if k == "preds":
            bad[k] = int((a.long() != b.long()).sum())
        else:
            assert a.dtype == b.dtype == torch.float32, (k, a.dtype, b.dtype)
            bad[k] = int((a.numpy().view(np.int32) != b.numpy().view(np.int32)).sum())
    return bad


def criterion_gap(got, want):
    """largest relative deviation of the engine's criterions (fp64 accumulation) from the restatement's (fp32)"""
    a, b = got["criterions"].double(), want["criterions"].double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(((a - b).abs() / b.abs().clamp(min=torch.finfo(torch.float32).tiny)).max())


# the outputs that are continuous functions of the inputs after ONE iteration; one-hot u and predictions are not
CONTINUOUS = {"skm": ("w", "u"), "hkm": ("w",), "klk": ("w",), "emg": ("w", "u", "v"), "cov": ("w", "s", "u", "v"),
              "paddle": ("w", "u", "v"), "bdcspn": ("w", "u")}
TINY = float(torch.finfo(torch.float32).tiny)


def rel_err(a, ref64):
    """e(a) = max over the elements of |a - ref64| / max(|ref64|, tiny), tiny the smallest normal float32"""
    return float(((a.double() - ref64).abs() / ref64.abs().clamp(min=TINY)).max())
