"""GPU: no k-means or few-shot entry touches a byte outside the workspace its query returns.  engine._Call.launch is replaced
by a copy that puts a workspace of exactly the queried size between two 4 KiB bands of a byte pattern inside one allocation and
checks both bands after a synchronise; every call form of every method (dense, visual, from the tables, visual from the
tables, value sweep) runs once that way and must return the bits it returns through the unpatched launch.

Shapes: 2 batches x 2 tasks, Q = 7, K = 5, one shot (S = 5), 3 iterations, knn = 3, three sweep values; D = 9 and D = 16 on
visual features - S D = 45 and 80 against (S + Q) K = 60 take both sides of BD-CSPN's max(T R K, T S D) region for table
input - and no region of any layout is a multiple of 256 bytes.  Two zero-shot calls at K = 37, Q = 75 take the tile kernels'
route through kmeans_loop and kl_kmeans_loop."""
import ctypes
import functools

import pytest
import torch

from tclip_amd import _capi, engine, synth

pytestmark = pytest.mark.gpu
T, Q, K, S, ITERS, KNN, VALUES = 4, 7, 5, 5, 3, 3, (0.5, 2.0, 3.0)
BAND, PATTERN = 4096, 0xA5


def _guarded_launch(self, entry, args):
    with torch.cuda.device(self.dev):
        buf = torch.full((self.ws_bytes + 2 * BAND + 256,), PATTERN, dtype=torch.uint8, device=self.dev)
        lo = (-buf.data_ptr()) % 256
        ws, hi = lo + BAND, lo + BAND + self.ws_bytes
        rc = getattr(self.lib, entry)(ctypes.byref(self.p), *args(ctypes.c_void_p(buf.data_ptr() + ws), self.ws_bytes, engine._stream()))
        _capi.check(rc, entry)
        torch.cuda.synchronize()
        assert bool((buf[lo:ws] == PATTERN).all()), f"{entry} wrote below its workspace"
        assert bool((buf[hi:hi + BAND] == PATTERN).all()), f"{entry} wrote beyond the {self.ws_bytes} bytes of its workspace query"


@functools.lru_cache(maxsize=None)
def _inputs(D):
    """D = 0: probability features of K columns; otherwise raw rows of D elements.  -> dense (x_q, x_s, y_s), tables
    (table_q, q_idx, table_s, s_idx, y_s) and, for the visual k-means, u0"""
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5 + D)
    if D == 0:
        x_q, _ = synth.make_query_tasks(T, K, seed=3, n_query=Q, k_eff=3)
        x_s, y_s = synth.make_support(T, K, 1, seed=3)
        table, labels = synth.make_feature_table(K, 6, seed=3)
    else:
        x_q, x_s = torch.randn(T, Q, D, generator=gen), torch.randn(T, S, D, generator=gen)
        y_s = torch.arange(K).repeat(T, 1)
        table, labels = torch.randn(K * 6, D, generator=gen), torch.arange(K).repeat_interleave(6)
    q_idx = torch.randint(K * 6, (T, Q), generator=gen)
    s_idx = torch.arange(K).repeat(T, 1) * 6 + torch.randint(6, (T, S), generator=gen)
    u0 = torch.softmax(torch.randn(T, Q, K, generator=gen), -1)
    dense = (x_q.to(dev), x_s.to(dev), y_s.reshape(T, S).to(dev))
    tables = (table.to(dev), q_idx, table.to(dev), s_idx, labels[s_idx].to(dev))
    return dense, tables, u0.to(dev)


def _cases():
    tim = dict(iters=ITERS, temp=15.0, lr=1e-3)
    few = {"paddle": (dict(iters=ITERS), dict(lambd=2.0)), "bdcspn": (dict(norm_type="CL2N"), dict(temp=2.0)),
           "alpha_tim": (dict(tim, n_batches=2), dict(alpha_value=2.0)), "laplacian_shot": (dict(iters=ITERS, knn=KNN), dict(lmd=2.0))}
    out = []
    zs = {"soft_kmeans": dict(iters=ITERS, temperature=5.0), "em_gaussian": dict(iters=ITERS, temperature=5.0, lambd=10),
          "em_gaussian_cov": dict(iters=ITERS, lambd=10), "hard_kmeans": dict(iters=ITERS, n_batches=2)}
    for m, kw in zs.items():
        out.append((f"run_{m}", "x_q", 0, kw))
        out.append((f"run_{m}_visual", "x_q+u0", 9, kw))
    out.append(("run_kl_kmeans", "x_q", 0, dict(iters=ITERS, n_batches=2)))
    out.append(("run_soft_kmeans", "k37", 0, dict(iters=ITERS, temperature=5.0)))
    out.append(("run_kl_kmeans", "k37", 0, dict(iters=ITERS, n_batches=2)))
    for m, (kw, scalar) in few.items():
        out.append((f"run_{m}", "dense", 0, dict(kw, **scalar)))
        out.append((f"run_{m}_tasks", "tables", 0, dict(kw, **scalar)))
        out.append((f"sweep_{m}_tasks", "tables", 0, dict(kw, values=VALUES)))
        for D in (9, 16):
            out.append((f"run_{m}_visual", "dense", D, dict(kw, n_class=K, **scalar)))
            out.append((f"run_{m}_visual_tasks", "tables", D, dict(kw, n_class=K, **scalar)))
        out.append((f"sweep_{m}_tasks", "tables", 9, dict(kw, n_class=K, values=VALUES)))
    for D in (9, 16):
        out.append(("run_tim_gd", "dense", D, dict(tim, n_class=K, n_batches=2)))
    out.append(("run_tim_gd_tasks", "tables", 9, dict(tim, n_class=K, n_batches=2)))
    return out


def _positional(rows, D):
    if rows == "k37":
        return (synth.make_query_tasks(T, 37, seed=4, n_query=75)[0].to(torch.device("cuda", 0)),)
    dense, tables, u0 = _inputs(D)
    return {"x_q": dense[:1], "x_q+u0": (dense[0], u0), "dense": dense, "tables": tables}[rows]


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32 if t.element_size() == 4 else torch.uint8)


@pytest.mark.parametrize("fn,rows,D,kw", _cases(), ids=lambda v: v if isinstance(v, str) else str(v) if isinstance(v, int) else "")
def test_no_entry_leaves_its_workspace(fn, rows, D, kw, monkeypatch):
    pos = _positional(rows, D)
    want = getattr(engine, fn)(*pos, **kw)
    torch.cuda.synchronize()
    monkeypatch.setattr(engine._Call, "launch", _guarded_launch)
    got = getattr(engine, fn)(*pos, **kw)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(_bits(g), _bits(w)), fn


def test_the_cases_cover_every_form_of_every_method():
    names = {c[0] for c in _cases()}
    few = {k % m for m in ("paddle", "bdcspn", "alpha_tim", "laplacian_shot")
           for k in ("run_%s", "run_%s_visual", "run_%s_tasks", "run_%s_visual_tasks", "sweep_%s_tasks")}
    zero = {f"run_{m}{v}" for m in ("soft_kmeans", "em_gaussian", "em_gaussian_cov", "hard_kmeans") for v in ("", "_visual")}
    assert names == few | zero | {"run_kl_kmeans", "run_tim_gd", "run_tim_gd_tasks"}
