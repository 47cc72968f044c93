"""GPU: scoring with a fitted EM-Dirichlet model (tclip_amd.score, tclip_em_dirichlet_score[_tasks]).

1. The reference's fixtures, without a fit: its loop ends with the dead-row revert, v_update and u_update(query), so the u it
   returns is a fresh E-step of the alpha, v and x_q it returns - scoring them must give the fixture's u and last argmax, bit
   for bit (soft) / as one-hot (hard).
2. Larger K through the engine's own fit, which the fixtures pin to the reference.
3. Row independence: the bits of a row do not depend on what shares the call, on its position or on the outputs asked for.
4. The table route against the dense entry on the gathered rows.
5. logits against a float64 restatement, bounded by twice the error of the same expression in torch fp32 on the CPU.
6. The four drop-in classes: score_rows / score_table_rows on the state a run leaves.

Measured on the MI355X (test 5 prints the figures): e(gpu) / e(ref32) = 1.0000 for the logits at every K of the sweep (e from
0.014 at K = 2 to 4.1 at K = 1000), although some logits differ from torch's fp32 ones in the last place on these wide-range
models; u carries torch's bits at every K but 2.  See DESIGN.md 8q."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SOFT = ["zs_soft_K2_N4", "zs_soft_K5_N2_borderline", "zs_soft_K7_N4", "zs_soft_K8_N2_borderline", "zs_soft_K10_N4", "zs_soft_K37_N6",
        "zs_soft_K47_N3", "zs_soft_K100_N4", "zs_soft_K102_N2", "fs_soft_K6_N3_s2", "fs_soft_K10_N4_s4", "fs_soft_K37_N3_s2",
        "fs_soft_K100_N4_s4"]
HARD = ["zs_hard_K5_N4", "zs_hard_K10_N4", "zs_hard_K37_N6", "zs_hard_K100_N4", "zs_hard_K196_N2", "fs_hard_K10_N4_s4",
        "fs_hard_K37_N3_s3", "fs_hard_K47_N3_s2", "fs_hard_K100_N3_s4"]
KS = [2, 15, 16, 17, 32, 33, 100, 129, 417, 1000, 1024]      # either side of every dispatch_E size in reach and of the K < 16 softmax
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """bit for bit, NaN payloads and signed zeros included"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _score(x, alpha, v, **kw):
    from tclip_amd import score
    return score.score_em_dirichlet(x, alpha, v, **kw)


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOFT + HARD)
def test_scoring_a_reference_fit_returns_its_u(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K, hard = int(g["K"]), name in HARD
    assert str(g["kind"]).endswith("hard") == hard and g["x_q"].shape[1] == 75
    x, alpha, v = (torch.from_numpy(g[k]).to(DEV) for k in ("x_q", "alpha", "v"))
    res = _score(x, alpha, v, lambd=int(K / 5) * 75, n_query=75, hard=hard)
    u, ref_u = res.u.cpu().numpy(), g["u"]
    assert not np.isnan(ref_u).any()
    if hard:
        assert ((ref_u == 0) | (ref_u == 1)).all() and (ref_u.sum(-1) == 1).all()
    assert np.array_equal(u.view(np.int32), ref_u.view(np.int32)), f"u differs from the reference's in {(u != ref_u).sum()} places"
    assert np.array_equal(res.preds.cpu().numpy(), g["argmax"][-1].astype(np.int32))


# ---- 2. larger K through the engine's own fit --------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,shots,hard", [(397, 2, 0, False), (1000, 2, 0, False), (1024, 1, 0, False), (100, 3, 2, True)])
def test_scoring_an_engine_fit_returns_its_u(K, N, shots, hard):
    from tclip_amd import engine, synth
    x_q, _ = synth.make_query_tasks(N, K, seed=31 + K, k_eff=5 if shots else None)
    x_q = x_q.to(DEV)
    x_s = y_s = None
    if shots:
        x_s, y_s = synth.make_support(N, K, shots, seed=31 + K)
        x_s, y_s = x_s.to(DEV), y_s.squeeze(2).to(DEV)
    lambd = int(K / 5) * 75
    fit = engine.run_em_dirichlet(x_q, x_s, y_s, iters=2, iter_mm=60, lambd=lambd, hard=hard)
    res = _score(x_q, fit.alpha, fit.v, lambd=lambd, n_query=75, hard=hard)
    assert _same(res.u, fit.u) and _same(res.preds, fit.preds)
    assert not torch.isnan(fit.u).any()


# ---- 3. / 5. seeded random models ----------------------------------------------------------------------------------------------
def _model(K, T, R, seed):
    """alpha log-uniform in [1e-2, 1e4] with a few rows of exact ones, v = log(p) + 1 of a random simplex point, simplex rows
    with some exact zeros"""
    gen = torch.Generator().manual_seed(seed)
    alpha = torch.exp(torch.rand(T, K, K, generator=gen) * np.log(1e6) + np.log(1e-2)).float()
    for t in range(T):
        alpha[t, torch.randperm(K, generator=gen)[:max(1, K // 8)]] = 1.0
    p = torch.softmax(torch.randn(T, K, generator=gen), -1)
    v = torch.log(p) + 1
    x = torch.softmax(3 * torch.randn(T, R, K, generator=gen), -1)
    x = x * (torch.rand(T, R, K, generator=gen) > 0.2)
    x[..., 0] += (x.sum(-1) == 0)                      # no all-zero row
    x = x / x.sum(-1, keepdim=True)
    assert (x == 0).any() and (alpha == 1).all(-1).any()
    return x.contiguous(), alpha.contiguous(), v.contiguous()


KW = dict(lambd=7 * 75, n_query=75)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_a_row_does_not_depend_on_what_shares_the_call(K, T):
    R = 257 if K < 1000 else 76
    x, alpha, v = (a.to(DEV) for a in _model(K, T, R, seed=1000 * T + K))
    full = _score(x, alpha, v, want_logits=True, **KW)
    assert not torch.isnan(full.logits).any()
    for piece in (1, 7, 75, 76):
        for a in range(0, R, piece):
            part = _score(x[:, a:a + piece], alpha, v, want_logits=True, **KW)
            for name in ("u", "preds", "logits"):
                assert _same(getattr(part, name), getattr(full, name)[:, a:a + piece]), (name, piece, a)
    rev = _score(x.flip(1), alpha, v, want_logits=True, **KW)
    first = _score(x[:1], alpha[:1], v[:1], want_logits=True, **KW)
    flat = _score(x[0], alpha[:1], v[:1], want_logits=True, **KW)
    for name in ("u", "preds", "logits"):
        assert _same(getattr(rev, name).flip(1), getattr(full, name)), name
        assert _same(getattr(first, name), getattr(full, name)[:1]), name
        assert _same(getattr(flat, name), getattr(full, name)[0]), name
    # the outputs asked for change nothing
    labels = _score(x, alpha, v, want_u=False, **KW)
    plain = _score(x, alpha, v, **KW)
    assert labels.u is None and labels.logits is None and plain.logits is None
    assert _same(labels.preds, full.preds) and _same(plain.preds, full.preds) and _same(plain.u, full.u)
    # hard: the one-hot of the same predictions
    hard = _score(x, alpha, v, hard=True, **KW)
    assert _same(hard.preds, full.preds)
    assert _same(hard.u, torch.nn.functional.one_hot(full.preds.long(), K).float())


def test_more_tiles_than_blocks():
    """beyond 65 536 tiles the blocks stride over the tiles (K = 2: 32 rows per tile): the rows of a late tile, of the ragged
    last one and of the first have the bits they have in a small call"""
    K, T = 2, 1
    R = 32 * 65536 + 32 + 5
    gen = torch.Generator().manual_seed(12)
    alpha = torch.exp(torch.rand(T, K, K, generator=gen) * np.log(1e3) + np.log(1e-1)).float().to(DEV)
    v = (torch.log(torch.softmax(torch.randn(T, K, generator=gen), -1)) + 1).to(DEV)
    x = torch.softmax(3 * torch.randn(T, R, K, generator=gen), -1).to(DEV)
    full = _score(x, alpha, v, want_logits=True, **KW)
    for a, b in ((0, 70), (32 * 65536 - 40, 32 * 65536 + 20), (R - 50, R)):
        part = _score(x[:, a:b], alpha, v, want_logits=True, **KW)
        for name in ("u", "preds", "logits"):
            assert _same(getattr(part, name), getattr(full, name)[:, a:b]), (name, a, b)
    # every row, against the same rows scored as two calls of half the size
    half = R // 2
    for a, b in ((0, half), (half, R)):
        part = _score(x[:, a:b], alpha, v, **KW)
        assert _same(part.u, full.u[:, a:b]) and _same(part.preds, full.preds[:, a:b])


# ---- 4. the table route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T,R", [(17, 3, 40), (100, 2, 77), (417, 2, 19)])
def test_table_rows_equal_the_dense_entry_on_the_gathered_rows(K, T, R):
    from tclip_amd import engine, score
    x, alpha, v = (a.to(DEV) for a in _model(K, T, 3 * R, seed=77 + K))
    table = x.reshape(-1, K)[:2 * R + 5].contiguous()
    gen = torch.Generator().manual_seed(K)
    idx = torch.randint(0, table.shape[0], (T, R), generator=gen)
    idx[:, 1] = idx[:, 0]                                           # repeats
    idx[-1, -3:] = table.shape[0] - 1
    cols = torch.stack([torch.arange(K - 1, -1, -1)] + [torch.randperm(K, generator=gen) for _ in range(T - 1)]).int()
    for c in (None, cols, cols.to(DEV)):
        for i in (idx, idx.to(DEV)):
            dense = _score(engine.gather_task_rows(table, i, c), alpha, v, want_logits=True, **KW)
            res = score.score_em_dirichlet_tasks(table, i, alpha, v, c, want_logits=True, **KW)
            for name in ("u", "preds", "logits"):
                assert _same(getattr(res, name), getattr(dense, name)), name
    for bad in (table.shape[0], -1):
        for i in (idx, idx.to(DEV)):
            i = i.clone()
            i[0, 2] = bad
            with pytest.raises(IndexError, match="idx"):
                score.score_em_dirichlet_tasks(table, i, alpha, v, **KW)
    badc = cols.clone()
    badc[0, 0] = K
    for c in (badc, badc.to(DEV)):
        with pytest.raises(IndexError):
            score.score_em_dirichlet_tasks(table, idx, alpha, v, c, **KW)


# ---- 5. logits against float64 -----------------------------------------------------------------------------------------------
def _restate(x, alpha, v, lambd, n_query, dtype):
    """get_logits and u_update of the reference (em_dirichlet.py:35-39, 141-143) on the CPU in `dtype`, task by task"""
    logits, u = [], []
    for t in range(x.shape[0]):
        a, z = alpha[t].to(dtype), x[t].to(dtype)
        l1 = torch.lgamma(a.sum(-1)).unsqueeze(0)
        l2 = -torch.lgamma(a).sum(-1).unsqueeze(0)
        l3 = ((a.unsqueeze(0) - 1) * torch.log(z + 1e-15).unsqueeze(1)).sum(-1)
        lg = l1 + l2 + l3
        logits.append(lg)
        u.append((lg if v is None else lg + lambd * v[t].to(dtype).unsqueeze(0) / n_query).softmax(1))
    return torch.stack(logits), torch.stack(u)


@pytest.mark.parametrize("K", KS)
def test_logits_against_float64(K):
    T, R = 3, (24 if K <= 129 else 8)
    x, alpha, v = _model(K, T, 257 if K < 1000 else 76, seed=3000 + K)      # test 3's models (T = 3), their first rows
    x = x[:, :R].contiguous()
    for vv in (v, None):
        l64, u64 = _restate(x, alpha, vv, KW["lambd"], 75, torch.float64)
        l32, u32 = _restate(x, alpha, vv, KW["lambd"], 75, torch.float32)
        res = _score(x.to(DEV), alpha.to(DEV), None if vv is None else vv.to(DEV), want_logits=True, **KW)
        e = lambda a, ref: float((a.double() - ref).abs().max())      # noqa: E731
        e_gpu, e_ref = e(res.logits.cpu(), l64), e(l32, l64)
        eu_gpu, eu_ref = e(res.u.cpu(), u64), e(u32, u64)
        print(f"K={K} v={'given' if vv is not None else 'None'}: logits e(gpu)={e_gpu:.4g} e(ref32)={e_ref:.4g} "
              f"ratio={e_gpu / e_ref if e_ref else float('nan'):.4f} bits_equal={_same(res.logits.cpu(), l32)}; "
              f"u e(gpu)={eu_gpu:.4g} e(ref32)={eu_ref:.4g} bits_equal={_same(res.u.cpu(), u32)}")
        assert e_gpu <= 2 * e_ref, (K, e_gpu, e_ref)
        if vv is None:              # the softmax of the logits alone, by the same rule
            assert eu_gpu <= 2 * eu_ref, (K, eu_gpu, eu_ref)


# ---- 6. the classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("few", [False, True], ids=["zero_shot", "few_shot"])
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_classes_score_with_the_state_a_run_leaves(few, hard):
    import importlib
    from src.utils import CfgNode
    from tclip_amd import engine, synth
    K, N, shots = 10, 3, 2
    mod = importlib.import_module("src.methods.{}.{}em_dirichlet".format("few_shot" if few else "zero_shot", "hard_" if hard else ""))
    cls = getattr(mod, "HARD_EM_DIRICHLET" if hard else "EM_DIRICHLET")
    args = CfgNode(iter=3, iter_mm=60, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30, use_softmax_feature=True,
                   graph_matching=True, shots=shots, batch_size=N)
    m = cls(model=None, device=torch.device(DEV), log_file=None, args=args)
    x_q, y_q = synth.make_query_tasks(N, K, seed=5, k_eff=5 if few else None)
    task = {"x_q": x_q.clone(), "y_q": y_q.clone()}
    if few:
        task["x_s"], task["y_s"] = synth.make_support(N, K, shots, seed=5)
    logs = m.run_task(task, shots) if few else m.run_task(task)
    assert set(logs) == {"timestamps", "criterions", "acc"}
    state = set(vars(m))
    res = m.score_rows(x_q)
    assert res.logits is None and _same(res.u, m.u) and _same(res.preds, m.preds)
    assert _same(m.score_rows(x_q, hard=not hard).preds, m.preds)
    # rows that were not queries of the fit, through the table
    table, _ = synth.make_feature_table(K, 6, seed=9)
    gen = torch.Generator().manual_seed(3)
    idx = torch.randint(0, table.shape[0], (N, 11), generator=gen)
    cols = torch.stack([torch.randperm(K, generator=gen) for _ in range(N)]).int()
    for c in (None, cols):
        a = m.score_table_rows(table, idx, c)
        b = m.score_rows(engine.gather_task_rows(table.to(DEV), idx, c))
        assert _same(a.u, b.u) and _same(a.preds, b.preds) and a.u.shape == (N, 11, K)
    assert set(vars(m)) == state, "scoring keeps nothing on the object"
