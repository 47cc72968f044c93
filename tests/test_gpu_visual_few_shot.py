"""GPU: few-shot PADDLE and BDCSPN on visual features (use_softmax_feature == False).

Pinned bit for bit to reference-made fixtures (tests/golden/make_golden_visual_fs.py), to a torch-CPU restatement of the
reference's op sequences over a sweep of feature lengths D, class counts K and support sizes S (tests/helpers/visual_fs.py), and
to the probability-feature entries at D = K.  Nothing here skips: a missing fixture fails."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG
from helpers import visual_fs

pytestmark = pytest.mark.gpu

PADDLE_FIX = ["fs_vis_paddle_D512_K10_S4_N3", "fs_vis_paddle_D1024_K37_S2_N2", "fs_vis_paddle_D768_K100_S1_N1"]
BDCSPN_FIX = ["fs_vis_bdcspn_D512_K10_S4_N3", "fs_vis_bdcspn_D1024_K37_S2_N2", "fs_vis_bdcspn_D768_K100_S1_N1"]
LEAN = ["lean_fs_vis_paddle_D1024_K1000_S1_N1", "lean_fs_vis_bdcspn_D1024_K1000_S1_N1"]


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def load(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_s, y_s, x_q, y_q = visual_fs.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["shots"]), int(g["seed"]),
                                              signal=float(g["signal"]))
    for k, a in (("x_s", x_s), ("x_q", x_q), ("y_s", y_s), ("y_q", y_q)):
        assert visual_fs.sha(a.numpy()) == str(g[k + "_sha1"]), k
    return g, x_s, y_s, x_q, y_q


def accuracy(preds, y_q):
    return (preds.long().cpu() == y_q).float().mean(1).numpy()


def _args(method, K, **kw):
    from src.utils import CfgNode
    a = CfgNode(iter=20, num_classes_test=K, n_class=K, n_query=75, k_eff=5, T=30.0, use_softmax_feature=False,
                name_method=method, lambd=0.0, temp=15.0, norm_type="L2N")
    a.update(kw)
    return a


# ---- 1. reference fixtures, bit for bit -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PADDLE_FIX)
def test_paddle_fixture_c_entry(name):
    from tclip_amd import engine
    g, x_s, y_s, x_q, y_q = load(name)
    u, v, w, preds = engine.run_paddle_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_class=int(g["K"]), iters=int(g["iters"]),
                                              lambd=float(g["lambd"]))
    print(name, "max |du|", float(np.abs(u.cpu().numpy() - g["u"]).max()), "max |dw|", float(np.abs(w.cpu().numpy() - g["w"]).max()),
          "max |dv|", float(np.abs(v.cpu().numpy() - g["v"]).max()))
    assert np.array_equal(preds.cpu().numpy(), g["preds"])
    assert np.array_equal(accuracy(preds, y_q), g["acc"])
    assert same(w, g["w"])
    assert same(u, g["u"])
    assert same(v, g["v"])
    assert ((g["u"] > 1e-6) & (g["u"] < 1 - 1e-6)).any() and any(0 < a < 1 for a in g["acc"])


@pytest.mark.parametrize("name", PADDLE_FIX)
def test_paddle_fixture_drop_in(name):
    from src.methods.few_shot.paddle import PADDLE
    g, x_s, y_s, x_q, y_q = load(name)
    a = _args("PADDLE", int(g["K"]), iter=int(g["iters"]), lambd=float(g["lambd"]))
    assert not hasattr(a, "text_features")
    m = PADDLE(model=None, device="cuda", log_file=None, args=a)
    logs = m.run_task({"x_s": x_s, "x_q": x_q, "y_s": y_s.unsqueeze(2), "y_q": y_q.unsqueeze(2)}, int(g["shots"]))
    assert set(logs) == {"timestamps", "criterions", "acc"}
    assert np.array_equal(logs["acc"][:, -1], g["acc"])
    assert len(logs["criterions"]) == int(g["iters"]) and not np.any(logs["criterions"])
    assert same(m.u, g["u"]) and same(m.v, g["v"]) and same(m.w, g["w"])
    assert np.array_equal(m.preds.cpu().numpy(), g["preds"])


@pytest.mark.parametrize("name", BDCSPN_FIX)
def test_bdcspn_fixture_c_entry(name):
    from tclip_amd import engine
    g, x_s, y_s, x_q, y_q = load(name)
    protos, u, preds = engine.run_bdcspn_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_class=int(g["K"]), temp=float(g["temp"]),
                                                norm_type=str(g["norm_type"]))
    print(name, "max |du|", float(np.abs(u.cpu().numpy() - g["u"]).max()),
          "max |dp|", float(np.abs(protos.cpu().numpy() - g["prototypes"]).max()))
    assert np.array_equal(preds.cpu().numpy(), g["preds"])
    assert np.array_equal(accuracy(preds, y_q), g["acc"])
    assert same(protos, g["prototypes"])
    assert same(u, g["u"])
    assert ((g["u"] > 1e-6) & (g["u"] < 1 - 1e-6)).any() and any(0 < a < 1 for a in g["acc"])


@pytest.mark.parametrize("name", BDCSPN_FIX)
def test_bdcspn_fixture_drop_in(name):
    from src.methods.few_shot.bdcspn import BDCSPN
    g, x_s, y_s, x_q, y_q = load(name)
    a = _args("BDCSPN", int(g["K"]), temp=float(g["temp"]), norm_type=str(g["norm_type"]))
    m = BDCSPN(model=None, device="cuda", log_file=None, args=a)
    logs = m.run_task({"x_s": x_s, "x_q": x_q, "y_s": y_s.unsqueeze(2), "y_q": y_q.unsqueeze(2)}, int(g["shots"]))
    assert np.array_equal(logs["acc"][:, -1], g["acc"])
    assert same(m.prototypes, g["prototypes"]) and same(m.u, g["u"])
    assert np.array_equal(m.preds.cpu().numpy(), g["preds"])


@pytest.mark.parametrize("name", LEAN)
def test_lean_case_digests(name):
    from tclip_amd import engine
    g, x_s, y_s, x_q, y_q = load(name)
    K = int(g["K"])
    if str(g["method"]) == "paddle":
        u, v, w, preds = engine.run_paddle_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_class=K, iters=int(g["iters"]),
                                                  lambd=float(g["lambd"]))
        got = {"u": u, "v": v, "w": w}
    else:
        protos, u, preds = engine.run_bdcspn_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_class=K, temp=float(g["temp"]),
                                                    norm_type=str(g["norm_type"]))
        got = {"prototypes": protos, "u": u}
    assert np.array_equal(preds.cpu().numpy(), g["preds"])
    assert np.array_equal(accuracy(preds, y_q), g["acc"]) and 0 < float(g["acc"][0]) < 1
    for k, a in got.items():
        assert visual_fs.sha(a.cpu().numpy()) == str(g[k + "_sha1"]), k


# ---- 2. one PADDLE iteration and the BD-CSPN pass against torch's CPU op sequence ---------------------------------------
# (D, K, shots).  Every D of the sweep with S below 16 (K = 5, 2 shots) and with K = 37; every K of the sweep; S between 256 and
# 4096 (65 x 4, 100 x 4, 397 x 4, 1000 x 1, 1000 x 4); S + 75 = 4171 > 4096 (K = 1024, 4 shots, D = 7); K*D not a multiple of 32
# (most of them: 5 x 7, 37 x 33, 397 x 7, 65 x 255 ...).  The largest torch temporary, S x K x D floats, is 0.65 GB
# (397 x 397 x 1024), under 2 GB everywhere.
DS = (1, 7, 8, 31, 33, 255, 256, 511, 512, 513, 768, 1000, 1024)
SWEEP = [(d, 5, 2) for d in DS] + [(d, 37, 1) for d in DS]
SWEEP += [(33, 2, 3), (256, 2, 1), (513, 64, 1), (1000, 64, 2), (255, 65, 4), (768, 65, 2), (31, 100, 4), (512, 100, 4),
          (7, 397, 1), (33, 397, 4), (1024, 397, 1), (8, 1000, 1), (31, 1000, 4), (7, 1024, 4)]


def test_sweep_covers_what_it_claims():
    assert {d for d, _, _ in SWEEP} == set(DS) and {2, 5, 37, 64, 65, 100, 397, 1000} <= {k for _, k, _ in SWEEP}
    sizes = [k * s for _, k, s in SWEEP]
    assert min(sizes) < 16 and any(256 < s < 4096 for s in sizes) and any(s + 75 > 4096 for s in sizes)
    assert any((k * d) % 32 for d, k, _ in SWEEP)
    assert max(k * s * k * d for d, k, s in SWEEP) * 4 < 2 << 30


@pytest.mark.parametrize("D,K,shots", SWEEP)
def test_paddle_iterations_match_torch(D, K, shots):
    from tclip_amd import engine
    N = 2 if K * shots * K * D < 50_000_000 else 1
    x_s, y_s, x_q = visual_fs.random_tasks(N, K, D, shots, seed=D * 1009 + K, scale=2.0 / D ** 0.5)
    lambd = 7.5
    u1, v1, w1 = visual_fs.paddle_step(x_s, x_q, y_s, K, lambd)
    gu, gv, gw, gp = engine.run_paddle_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_class=K, iters=1, lambd=lambd)
    assert same(gu, u1)
    assert same(gw, w1)
    assert np.array_equal(gp.cpu().numpy(), u1.argmax(2).int().numpy())
    # v = log(...) + 1 of the host's torch, whose SLEEF variant follows the host CPU's vector ISA: a few ulp (the fixtures, made
    # on the reference's side, pin v bit for bit).  The second iteration therefore starts from the engine's own v.
    np.testing.assert_allclose(gv.cpu().numpy(), v1.numpy(), rtol=1e-6, atol=5e-7)
    u2, _, w2 = visual_fs.paddle_step(x_s, x_q, y_s, K, lambd, w=w1, v=gv.cpu())
    gu2, _, gw2, _ = engine.run_paddle_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_class=K, iters=2, lambd=lambd)
    assert same(gu2, u2)
    assert same(gw2, w2)


@pytest.mark.parametrize("D,K,shots", SWEEP)
def test_bdcspn_pass_matches_torch(D, K, shots):
    from tclip_amd import engine
    x_s, y_s, x_q = visual_fs.random_tasks(1 if K * shots * K * D > 50_000_000 else 2, K, D, shots, seed=D * 1013 + K)
    x_s, x_q = x_s + 0.5, x_q + 0.25          # off-centre, so that eta and the CL2N mean are not noise around zero
    for norm_type in ("L2N", "CL2N", "UN") if K * shots * K * D < 50_000_000 else (("L2N", "CL2N", "UN")[(D + K) % 3],):
        rp, ru, rpred = visual_fs.bdcspn_pass(x_s, x_q, y_s, K, 10.0, norm_type)
        gp, gu, gpred = engine.run_bdcspn_visual(x_q.cuda(), x_s.cuda(), y_s.cuda(), n_class=K, temp=10.0, norm_type=norm_type)
        assert same(gp, rp), norm_type
        assert same(gu, ru), norm_type
        assert np.array_equal(gpred.cpu().numpy(), rpred.int().numpy()), norm_type


# ---- 3. D = K: the same bits as the probability-feature entries ------------------------------------------------------

@pytest.mark.parametrize("K,shots", [(10, 4), (37, 2), (100, 1), (64, 5)])
def test_width_equal_to_class_count_matches_probability_entries(K, shots):
    from tclip_amd import engine
    gen = torch.Generator().manual_seed(K)
    x_s = (torch.randn(3, K * shots, K, generator=gen) * 3).softmax(-1).cuda()
    x_q = (torch.randn(3, 75, K, generator=gen) * 3).softmax(-1).cuda()
    y_s = torch.arange(K).repeat_interleave(shots).repeat(3, 1).cuda()
    a = engine.run_paddle(x_q, x_s, y_s, iters=5, lambd=3.0)
    b = engine.run_paddle_visual(x_q, x_s, y_s, n_class=K, iters=5, lambd=3.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for norm_type in ("UN", "L2N", "CL2N"):
        a = engine.run_bdcspn(x_q, x_s, y_s, temp=15.0, norm_type=norm_type)
        b = engine.run_bdcspn_visual(x_q, x_s, y_s, n_class=K, temp=15.0, norm_type=norm_type)
        for x, y in zip(a, b):
            assert torch.equal(x, y), norm_type


# ---- 4. end to end ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["PADDLE", "BDCSPN"])
def test_evaluator_on_visual_tables(method):
    from src.eval_few_shot import Evaluator_few_shot
    g = np.load(os.path.join(GOLDEN, f"eval_fs_vis_{method.lower()}_D512_K10.npz"))
    K, D = int(g["K"]), int(g["D"])
    feats_s, labels_s, feats_q, labels_q = visual_fs.make_tables(K, D, int(g["rows_per_class"]), int(g["seed"]),
                                                                 signal=float(g["signal"]))
    a = _args(method, K, number_tasks=int(g["number_tasks"]), batch_size=int(g["batch_size"]), used_test_set="test",
              dataset="synthetic", shots=int(g["shots"]), iter=int(g["iters"]), lambd=float(g["lambd"]), temp=float(g["temp"]),
              norm_type=str(g["norm_type"]), tunable=False)
    ev = Evaluator_few_shot(device=torch.device("cuda", 0), args=a, log_file=None)
    acc, _ = ev.evaluate_tasks(None, feats_s, labels_s, feats_q, labels_q,
                               indices=(torch.from_numpy(g["support_idx"]), torch.from_numpy(g["query_idx"])))
    assert np.array_equal(ev.last_task_accuracies.astype(np.float32), g["task_accuracy"])
    assert abs(float(acc) - float(g["mean_accuracy"])) < 1e-7
    assert 0 < float(g["mean_accuracy"]) < 1


@pytest.mark.parametrize("method,param", [("paddle", "lambd"), ("bdcspn", "temp")])
def test_main_features_visual_plk(method, param, tmp_path):
    """main_features on visual .plk files in the reference's layout, no text features anywhere: two validation runs write the
    sweep file <METHOD>_visual_s2.txt, the test run reads its parameter back and reproduces the reference's mean accuracy."""
    from tclip_amd import features
    sys.path.insert(0, PKG)
    import main_features
    g = np.load(os.path.join(GOLDEN, f"eval_fs_vis_{method}_D512_K10.npz"))
    feats_s, labels_s, feats_q, labels_q = visual_fs.make_tables(int(g["K"]), int(g["D"]), int(g["rows_per_class"]), int(g["seed"]),
                                                                 signal=float(g["signal"]))
    d = tmp_path / "data" / "synthetic" / "saved_features"
    d.mkdir(parents=True)
    features.save_features(str(d / "train_visual_RN50.plk"), feats_s, labels_s)
    for split in ("val", "test"):
        features.save_features(str(d / f"{split}_visual_RN50.plk"), feats_q, labels_q)
    value = str(float(g[param]))
    common = ["--results-root", str(tmp_path), "--opts", "method", method, "use_softmax_feature", "False", "shots",
              str(int(g["shots"])), "number_tasks", "20", "batch_size", "10", "dataset", "synthetic", "seed", str(int(g["seed"])),
              param, value]
    for _ in range(2):            # the reader of the sweep file skips its first two lines
        _, _, sweep = main_features.main(common + ["used_test_set", "val"])
    assert sweep.endswith(os.path.join("results_few_shot", "val", "synthetic", f"{method.upper()}_visual_s2.txt"))
    rows = open(sweep).read().splitlines()
    assert rows[0] == "val_param\tacc" and [r.split("\t")[0] for r in rows[1:]] == [value, value]
    acc, t, path = main_features.main(common)
    assert abs(float(acc) - float(g["mean_accuracy"])) < 1e-7
    assert path.endswith(os.path.join("results_few_shot", "test", "synthetic", f"{method.upper()}_visual_s2.txt"))
    assert open(path).read().splitlines()[-1].split("\t")[:4] == ["2", "75", "5", str(round(100 * float(g["mean_accuracy"]), 1))]


# ---- 5. argument errors ----------------------------------------------------------------------------------------------

def test_argument_errors():
    from tclip_amd import _capi, engine
    lib = _capi.lib()
    p = _capi.Problem(1, 1, 75, 10, 20, 1, 1, 0, 0)
    for query in (lib.tclip_paddle_visual_workspace_bytes, lib.tclip_bdcspn_visual_workspace_bytes):
        assert query(ctypes.byref(p), 512) > 0
        for dim in (0, 1025):
            assert query(ctypes.byref(p), dim) == 0 and b"dim" in lib.tclip_last_error()
        assert query(ctypes.byref(_capi.Problem(1, 1, 75, 10, 0, 1, 1, 0, 0)), 512) == 0
        assert b"n_support" in lib.tclip_last_error()
        assert query(ctypes.byref(_capi.Problem(1, 1, 75, 1025, 20, 1, 1, 0, 0)), 512) == 0
    x_q, x_s = torch.randn(1, 75, 512).cuda(), torch.randn(1, 20, 512).cuda()
    y_s = torch.arange(10).repeat_interleave(2).view(1, 20).cuda()
    u, v, w = torch.empty(1, 75, 10).cuda(), torch.empty(1, 10).cuda(), torch.empty(1, 10, 512).cuda()
    preds = torch.empty(1, 75, dtype=torch.int32).cuda()
    ws = torch.empty(1 << 22, dtype=torch.uint8).cuda()
    off = (-ws.data_ptr()) % 256
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    wsp = ctypes.c_void_p(ws.data_ptr() + off)

    def paddle(problem, dim, ws_bytes):
        return lib.tclip_paddle_visual_run(ctypes.byref(problem), dim, P(x_q), P(x_s), P(y_s), ctypes.c_float(1.0), P(u), P(v), P(w),
                                           P(preds), wsp, ws_bytes, None)

    def bdcspn(problem, dim, ws_bytes):
        return lib.tclip_bdcspn_visual_run(ctypes.byref(problem), dim, P(x_q), P(x_s), P(y_s), ctypes.c_float(1.0), 1, P(w), P(u),
                                           P(preds), wsp, ws_bytes, None)
    for run, query in ((paddle, lib.tclip_paddle_visual_workspace_bytes), (bdcspn, lib.tclip_bdcspn_visual_workspace_bytes)):
        need = query(ctypes.byref(p), 512)
        assert 0 < need < (1 << 22) - 256
        assert run(p, 0, need) == 1 and run(p, 1025, need) == 1                       # TCLIP_ERR_ARG
        assert run(_capi.Problem(1, 1, 75, 10, 0, 1, 1, 0, 0), 512, need) == 1
        assert run(p, 512, need - 1) != 0 and b"workspace" in lib.tclip_last_error()
        assert run(p, 512, need) == 0
    torch.cuda.synchronize()
    assert lib.tclip_bdcspn_visual_run(ctypes.byref(p), 512, P(x_q), P(x_s), P(y_s), ctypes.c_float(1.0), 3, P(w), P(u), P(preds), wsp,
                                       1 << 21, None) == 1
    for bad in (-1, 10):
        y_bad = y_s.clone()
        y_bad[0, 3] = bad
        with pytest.raises(ValueError, match="label"):
            engine.run_paddle_visual(x_q, x_s, y_bad, n_class=10, iters=1, lambd=0.0)
        with pytest.raises(ValueError, match="label"):
            engine.run_bdcspn_visual(x_q, x_s, y_bad, n_class=10, temp=1.0)
    with pytest.raises(ValueError):
        engine.run_paddle_visual(x_q, x_s[:, :, :100].contiguous(), y_s, n_class=10, iters=1, lambd=0.0)
    with pytest.raises(ValueError):
        engine.run_bdcspn_visual(x_q, x_s, y_s, n_class=1025, temp=1.0)
    torch.cuda.synchronize()
