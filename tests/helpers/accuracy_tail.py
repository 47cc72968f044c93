"""Shapes, inputs, restatements and runners of tests/test_accuracy_tail.py, tests/test_gpu_accuracy_tail.py and
tests/test_gpu_front_end.py: the accuracy tail's prototype kernels (tclip_cluster_prototypes: k_one_hot, k_cluster_sizes,
launch_mstats mode 0, k_gather_prototypes; tclip_cluster_prototypes_visual: k_vis_prototypes) and the two instantiations of
k_probability_features (tclip_probability_features, tclip_visual_init), each against a plain torch restatement of the
reference's op sequence in fp32 and in float64.  numpy's PCG64 draws every input: the same bits on every machine."""
import ctypes
import functools

import numpy as np
import torch

EPS = 1e-15                       # the reference's clamp of the cluster sizes
SENTINEL = -123456.0              # what run_prototypes leaves in rows the kernels must not write
TINY = float(torch.finfo(torch.float32).tiny)
PATTERNS = ("random_all", "full", "full_reversed", "single", "three_spread", "alone_but_two")

# ---- shape tables ------------------------------------------------------------------------------------------------------
# Probability features, (K, Q, T).  K at Q = 75: below and at the column kernel's smallest K (7, 8), both sides of a 64-class
# tile, of the LDS-tile limit (511 .. 513) and the largest K (1000 ragged, 1024).  Q at K = 7, 40, 100: the cascade's dump
# after every 16 rows (15 .. 17) and at 256 rows (255 .. 257), the neighbours of the special-cased 75, Q < K and Q > K.
# (1024, 1100): Q > K = Cmax, every slot of k_gather_prototypes's ids array in LDS taken (one task: the restatement's
# (Q, K, K) temporary is 4.6 GB in fp32 and is summed in ranges of classes).  T at K = 72: tasks are dealt to
# blocks in groups of eight.
PROB_K = (2, 5, 7, 8, 64, 65, 100, 511, 512, 513, 1000, 1024)
PROB_Q = (1, 3, 15, 16, 17, 74, 76, 128, 255, 256, 257, 300)
PROB_SHAPES = ([(k, 75, 7) for k in PROB_K] + [(k, q, 7) for k in (7, 40, 100) for q in PROB_Q] + [(1024, 1100, 1)] +
               [(72, 75, t) for t in (1, 8, 9, 17)])
# Visual features, (K, D, Q, T).  D at K = 5: K*D is a multiple of 32 only at D = 512 and 1024, so the last columns take
# the 4-way row sum everywhere else, and D = 1 gives fewer than 8 columns.  K at D = 33; the largest case; Q at (7, 40) and
# Q = 257 at a K*D that is no multiple of 32.
VIS_D = (1, 3, 7, 8, 9, 31, 33, 255, 511, 512, 513, 1000, 1023, 1024)
VIS_K = (2, 64, 65, 130, 1000)
VIS_Q = (1, 15, 16, 17, 255, 256, 257, 300)
VIS_SHAPES = ([(5, d, 75, 7) for d in VIS_D] + [(k, 33, 75, 7) for k in VIS_K] + [(1000, 1024, 75, 7)] +
              [(7, 40, q, 7) for q in VIS_Q] + [(65, 513, 257, 7)])
# engine.clustering_accuracy / clustering_accuracy_visual: Q < K, Q > K, Q != 75 and the special-cased 75
COMPOSE_PROB = [(7, 3, 7), (100, 17, 7), (7, 300, 7), (40, 257, 7), (65, 75, 7)]
COMPOSE_VIS = [(7, 40, 1, 7), (130, 33, 75, 7), (7, 40, 300, 7), (65, 513, 257, 7), (5, 3, 16, 7)]
COMPOSE_T = 5.0
# The front end, (n, D, K, T): D at K = 37 (the 16-byte loads need D % 4 == 0; 64-product blocks), K at D = 512 (a block
# has 256 threads: with K < 64 three wavefronts own no class, K > 256 gives a thread a second class), one row and 65 rows,
# and the three temperatures at three (D, K).
FRONT_D = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 1000, 1023, 1024)
FRONT_K = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1024)
FRONT_SHAPES = ([(65, d, 37, 30) for d in FRONT_D] + [(65, 512, k, 30) for k in FRONT_K] + [(1, 512, 37, 30), (1, 5, 2, 30)] +
                [(n, d, k, t) for (d, k) in ((512, 100), (1024, 1000), (1000, 397)) for t in (10, 30, 100)
                 for n in ((65,) if t != 100 else (1, 65))])
FRONT_KINDS = ("random", "structured")
# Where the two scale orders are told apart: T = 100 is no power of two, so T * f rounds in every element.  On dense rows that
# rounding is a tenth of what the summation order moves, and no distance separates the two formulas; on "sparse" rows (one
# element of size 1 .. 2, one of 1/64, zeros elsewhere) every partial sum but one is exact in any order and the scale order
# is what is left.  D = 128: the 16-byte loads; 129: the scalar loop.
SWAP_CASES = [(65, 128, 37, 100), (65, 129, 37, 100)]
MIN_PROB = 1e-32


def prob_id(s):
    return "K{}_Q{}_T{}".format(*s)


def vis_id(s):
    return "K{}_D{}_Q{}_T{}".format(*s)


def front_id(s):
    return "n{}_D{}_K{}_T{}".format(*s)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def make_preds(T, Q, K, seed):
    """(T, Q) int64 predictions in 0..K-1, task t after PATTERNS[t % 6] - a single task after "full", the pattern with the
    most clusters; -> (preds, the pattern names)"""
    rng = np.random.default_rng(seed)
    out = np.empty((T, Q), np.int64)
    names = ["full"] if T == 1 else [PATTERNS[t % len(PATTERNS)] for t in range(T)]
    for t in range(T):
        p = names[t]
        if p == "random_all":
            out[t] = rng.integers(0, K, size=Q)
        elif p == "full":                                 # n_clusters = min(Q, K) exactly
            out[t] = np.arange(Q) % K
        elif p == "full_reversed":                        # class K-1 first: first appearance is not sorted order
            out[t] = (K - 1) - np.arange(Q) % K
        elif p == "single":
            out[t] = rng.integers(0, K)
        elif p == "three_spread":
            out[t] = np.array([0, K // 2, K - 1])[rng.integers(0, 3, size=Q)]
        else:                                             # every query alone in its cluster except two
            classes = rng.permutation(K)[:max(1, min(Q - 1, K))]
            row = classes[np.arange(max(Q - 1, 1)) % len(classes)]
            out[t] = np.concatenate([row, row[rng.integers(0, len(row), size=1)]])[:Q] if Q > 1 else row[:1]
    return out, names


def make_prob_rows(T, Q, K, seed):
    """(T, Q, K) float32 rows on the simplex"""
    rng = np.random.default_rng(seed)
    e = np.exp(3.0 * rng.standard_normal((T, Q, K)))
    return torch.from_numpy((e / e.sum(-1, keepdims=True)).astype(np.float32))


def make_visual_rows(T, Q, D, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((3.0 * rng.standard_normal((T, Q, D))).astype(np.float32))


def make_text(K, D, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((K, D))
    return torch.from_numpy((t / np.linalg.norm(t, axis=-1, keepdims=True)).astype(np.float32))


def make_front_rows(kind, n, text, seed):
    """random: 3 * randn; sparse: see SWAP_CASES; structured: 2 * text[label] + noise of expected norm 4 -> ((n, D) float32, labels or None)"""
    K, D = text.shape
    rng = np.random.default_rng(seed)
    if kind == "random":
        return torch.from_numpy((3.0 * rng.standard_normal((n, D))).astype(np.float32)), None
    if kind == "sparse":
        f = np.zeros((n, D), np.float32)
        for r in range(n):
            i, j = rng.choice(D, size=2, replace=False)
            f[r, i] = (1.0 + rng.random()) * (1.0 if rng.random() < 0.5 else -1.0)
            f[r, j] = rng.standard_normal() / 64.0
        return torch.from_numpy(f), None
    labels = rng.integers(0, K, size=n)
    noise = rng.standard_normal((n, D)) * (4.0 / np.sqrt(D))
    return torch.from_numpy((2.0 * text.numpy()[labels] + noise).astype(np.float32)), labels


# ---- restatements ------------------------------------------------------------------------------------------------------
def first_appearance(preds, K):
    """-> (n_clusters (T,) int32, the classes present in preds[t] in the order of their first appearance, padded with -1 to
    Cmax = min(Q, K): (T, Cmax) int32), in plain Python (src/utils.py:387-394)"""
    preds = np.asarray(preds)
    T, Q = preds.shape
    ncl = np.zeros(T, np.int32)
    ids = -np.ones((T, min(Q, K)), np.int32)
    for t in range(T):
        order = []
        for c in preds[t].tolist():
            if c not in order:
                order.append(c)
        ncl[t] = len(order)
        ids[t, :len(order)] = order
    return ncl, ids


def _column_chunks(K, W, Q, itemsize, limit):
    """class ranges [k0, k1) whose (Q, k1 - k0, W) temporaries stay under `limit` bytes and whose columns are a multiple of 32
    in every range but the last: torch's outer sum then sends each column down the path it takes in the whole (Q, K*W) sum"""
    if Q * K * W * itemsize <= limit or K * W < 64:
        return [(0, K)]
    step = max(1, limit // (Q * W * itemsize))
    while (step * W) % 32:
        step += 1
    return [(k0, min(K, k0 + step)) for k0 in range(0, K, step)]


def prototypes_reference(preds, z, K, dtype, limit=1 << 29):
    """The reference's op sequence (soft_kmeans.py:36-44, em_dirichlet.py:61-70) in `dtype`:
        (one_hot(preds).unsqueeze(-1) * z.unsqueeze(2)).sum(1) / one_hot(preds).sum(1).clamp(min=EPS).unsqueeze(-1)
    and of that the rows of the clusters present, in first-appearance order: (T, Cmax, W), rows from n_clusters[t] on zero.
    z (T, Q, W): W = K on probability features, D on visual ones.  One task at a time, and a task whose (Q, K, W) temporary
    would pass `limit` bytes in ranges of classes (_column_chunks): tests/test_accuracy_tail.py holds both to the bits of
    the one-piece formula."""
    preds = torch.as_tensor(np.asarray(preds)).long()
    T, Q = preds.shape
    W = z.shape[2]
    ncl, ids = first_appearance(preds.numpy(), K)
    eye = torch.eye(K, dtype=dtype)
    out = torch.zeros(T, ids.shape[1], W, dtype=dtype)
    for t in range(T):
        hot, zt = eye[preds[t]], z[t].to(dtype)                               # (Q, K), (Q, W)
        sizes = hot.unsqueeze(0).sum(1).clamp(min=EPS).squeeze(0)             # (K,)
        full = torch.cat([(hot[:, k0:k1].unsqueeze(-1) * zt.unsqueeze(1)).unsqueeze(0).sum(1).squeeze(0)
                          for k0, k1 in _column_chunks(K, W, Q, zt.element_size(), limit)])
        protos = full / sizes.unsqueeze(-1)
        out[t, :ncl[t]] = protos[torch.from_numpy(ids[t, :ncl[t]]).long()]
    return out


def prototypes_reference_one_piece(preds, z, K, dtype):
    """the formula as the reference writes it, over all tasks at once -> the dense (T, K, W) prototypes"""
    hot = torch.eye(K, dtype=dtype)[torch.as_tensor(np.asarray(preds)).long()]
    return (hot.unsqueeze(-1) * z.to(dtype).unsqueeze(2)).sum(1) / hot.sum(1).clamp(min=EPS).unsqueeze(-1)


def front_end_reference(f, text, T, scale_after, dtype):
    """scale_after False: softmax(T * normalize(f) @ text.T), the front end (src/utils.py:287-290);
    True: softmax(T * (normalize(f) @ text.T)), the visual initialisation (soft_kmeans.py:185-197)"""
    f, text = f.to(dtype), text.to(dtype)
    fn = f / f.norm(dim=-1, keepdim=True)
    return (T * (fn @ text.T)).softmax(-1) if scale_after else (T * fn @ text.T).softmax(-1)


def match_reference(preds, ncl, ids, rows, y, graph_matching):
    """clusters to classes as compute_acc_clustering does it (src/utils.py:380-417): scipy's assignment on -rows of the
    clusters present, or each cluster's argmax -> (new_preds (T, Q) int32, acc (T,) float32)"""
    from scipy.optimize import linear_sum_assignment
    preds, y = np.asarray(preds), np.asarray(y)
    T, Q = preds.shape
    new = np.empty((T, Q), np.int32)
    for t in range(T):
        c = int(ncl[t])
        r = rows[t, :c].numpy()
        cls = linear_sum_assignment(-r.astype(np.float64), maximize=False)[1] if graph_matching else r.argmax(-1)
        lut = {int(ids[t, i]): int(cls[i]) for i in range(c)}
        new[t] = [lut[int(p)] for p in preds[t]]
    acc = torch.from_numpy(new == y).float().mean(1).numpy()
    return new, acc


def rel_err(a, ref64, rows=None):
    """prob_shapes.rel_err over the rows [0, rows[t]) of every task (all rows: None)"""
    d = (a.double() - ref64).abs() / ref64.abs().clamp(min=TINY)
    if rows is not None:
        d = torch.cat([d[t, :int(n)].reshape(-1) for t, n in enumerate(rows)])
    return float(d.max())


def bit_differences(a, b, rows):
    """number of elements of the rows [0, rows[t]) whose bits differ"""
    a, b = np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32)
    return int(sum((a[t, :int(n)] != b[t, :int(n)]).sum() for t, n in enumerate(rows)))


# ---- cases -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prototype_case(shape, visual):
    """inputs and both restatements of one shape, computed once: dict(K, W, preds, patterns, z, ncl, ids, ref32, ref64)"""
    if visual:
        K, W, Q, T = shape
    else:
        (K, Q, T), W = shape, shape[0]
    seed = ((K * 1031 + W) * 1031 + Q) * 31 + T
    preds, patterns = make_preds(T, Q, K, seed)
    z = make_visual_rows(T, Q, W, seed + 1) if visual else make_prob_rows(T, Q, K, seed + 1)
    ncl, ids = first_appearance(preds, K)
    return {"K": K, "W": W, "preds": preds, "patterns": patterns, "z": z, "ncl": ncl, "ids": ids,
            "ref32": prototypes_reference(preds, z, K, torch.float32), "ref64": prototypes_reference(preds, z, K, torch.float64)}


def check_prototype_inputs(case, shape):
    """what a case must hold for its checks to mean what they say"""
    K, preds, ncl, ids = case["K"], case["preds"], case["ncl"], case["ids"]
    T, Q = preds.shape
    assert preds.min() >= 0 and preds.max() < K, shape
    cmax = min(Q, K)
    assert ids.shape == (T, cmax)
    for t, p in enumerate(case["patterns"]):
        if p in ("full", "full_reversed"):
            assert ncl[t] == cmax, (shape, p)
        if p == "full_reversed":
            assert ids[t, 0] == K - 1 and (cmax == 1 or ids[t, 1] < ids[t, 0]), shape
        if p == "single":
            assert ncl[t] == 1, shape
        if p == "three_spread":
            assert set(ids[t, :ncl[t]].tolist()) <= {0, K // 2, K - 1}, shape
        if p == "alone_but_two" and 2 <= Q <= K + 1:
            assert ncl[t] == Q - 1, shape
    assert torch.isfinite(case["ref64"]).all()
    # every prototype row that is compared is a mean of at least one row: it has a non-zero element
    for t in range(T):
        assert (case["ref64"][t, :ncl[t]].abs().amax(-1) > 0).all(), shape


@functools.lru_cache(maxsize=None)
def front_case(shape, kind):
    """dict(f, text, T, ref32/ref64 per scale order) of one front-end shape; asserts the input condition"""
    n, D, K, T = shape
    seed = ((n * 1031 + D) * 1031 + K) * 131 + T
    text = make_text(K, D, seed)
    f, labels = make_front_rows(kind, n, text, seed + 1)
    case = {"f": f, "text": text, "T": float(T), "labels": labels}
    for after in (False, True):
        case["ref32", after] = front_end_reference(f, text, float(T), after, torch.float32)
        case["ref64", after] = front_end_reference(f, text, float(T), after, torch.float64)
    check_front_inputs(case, shape)
    return case


def check_front_inputs(case, shape):
    for after in (False, True):
        r64 = case["ref64", after]
        assert float(r64.min()) >= MIN_PROB, (shape, after, float(r64.min()))       # every fp32 value is then normal
        assert float(case["ref32", after].min()) >= TINY, (shape, after)


def front_distance(a, b, ref64):
    """root mean square of (a - b) / ref64: relative on every probability, so on the logits' scale"""
    return float((((a.double() - b.double()) / ref64) ** 2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def compose_case(shape, visual):
    """Separated inputs for the composition: x_q = 2 * text[y] + noise (probability path: their fp32 front-end rows), the
    predictions a noisy relabelling of y.  Holds, per graph_matching value, the restated (new_preds, acc) - asserted to be the
    same from fp32 and from float64 prototypes, so that no rounding of the engine's can legitimately move an assignment."""
    if visual:
        K, D, Q, T = shape
    else:
        (K, Q, T), D = shape, 48
    seed = ((K * 1031 + D) * 1031 + Q) * 31 + T + 7
    rng = np.random.default_rng(seed)
    text = make_text(K, D, seed + 1)
    y = np.stack([rng.choice(rng.choice(K, size=min(5, K), replace=False), size=Q) for _ in range(T)]).astype(np.int64)
    noise = rng.standard_normal((T, Q, D)) * (1.0 / np.sqrt(D))
    emb = torch.from_numpy((2.0 * text.numpy()[y] + noise).astype(np.float32))
    relabel = np.stack([rng.permutation(K) for _ in range(T)])
    preds = np.take_along_axis(relabel, y, 1)
    flip = rng.random((T, Q)) < 0.1
    preds = np.where(flip, rng.integers(0, K, size=(T, Q)), preds).astype(np.int64)
    x_q = emb if visual else front_end_reference(emb.reshape(T * Q, D), text, COMPOSE_T, False, torch.float32).reshape(T, Q, K)
    ncl, ids = first_appearance(preds, K)
    case = {"K": K, "x_q": x_q, "y": y, "preds": preds, "text": text, "ncl": ncl, "ids": ids}
    for graph in (True, False):
        got = {}
        for dtype in (torch.float32, torch.float64):
            rows = prototypes_reference(preds, x_q, K, dtype)
            if visual:                                     # the tail scores the prototypes with the front-end formula
                rows = front_end_reference(rows.reshape(-1, D), text, COMPOSE_T, False, dtype).reshape(T, -1, K)
            got[dtype] = match_reference(preds, ncl, ids, rows, y, graph)
        assert np.array_equal(got[torch.float32][0], got[torch.float64][0]), (shape, graph, "fp32 and float64 assign differently")
        assert np.array_equal(got[torch.float32][1], got[torch.float64][1]), (shape, graph)
        case["want", graph] = got[torch.float32]
    return case


# ---- runners (GPU) -----------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_prototypes(preds, z, K, visual):
    """tclip_cluster_prototypes / tclip_cluster_prototypes_visual through tclip_amd._capi, `prototypes` filled with SENTINEL
    beforehand -> the raw arrays (n_clusters (T,) int32, cluster_ids (T, Cmax) int32, prototypes (T, Cmax, W) float32), numpy"""
    from tclip_amd import _capi
    lib = _capi.lib()
    dev = "cuda:0"
    zd = z.to(dev).contiguous().float()
    T, Q, W = zd.shape
    pd = torch.as_tensor(np.asarray(preds)).to(dev).int().contiguous()
    cmax = min(Q, K)
    ncl = torch.full((T,), -7, dtype=torch.int32, device=dev)
    ids = torch.full((T, cmax), -7, dtype=torch.int32, device=dev)
    protos = torch.full((T, cmax, W), SENTINEL, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if visual:
        rc = lib.tclip_cluster_prototypes_visual(T, Q, K, W, _ptr(zd), _ptr(pd), _ptr(ncl), _ptr(ids), _ptr(protos), stream)
        _capi.check(rc, "tclip_cluster_prototypes_visual")
    else:
        assert W == K
        ws_bytes = lib.tclip_prototype_workspace_bytes(T, Q, K)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 256
        rc = lib.tclip_cluster_prototypes(T, Q, K, _ptr(zd), _ptr(pd), _ptr(ncl), _ptr(ids), _ptr(protos),
                                          ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, stream)
        _capi.check(rc, "tclip_cluster_prototypes")
    torch.cuda.synchronize()
    return ncl.cpu().numpy(), ids.cpu().numpy(), protos.cpu().numpy()


def run_front_end(f, text, T, scale_after):
    """features.probability_features (scale before the product) or engine.visual_init (after) -> (n, K) float32, cpu"""
    from tclip_amd import engine, features
    fn = engine.visual_init if scale_after else features.probability_features
    out = fn(f.cuda(), text.cuda(), T)
    torch.cuda.synchronize()
    return out.cpu()
