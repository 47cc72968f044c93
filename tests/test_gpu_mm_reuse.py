"""GPU: k_mm_reuse, the live rows' MM kernel for chunks 1.. of the first outer iteration.

digamma and lgamma are evaluated at fl(a + 1); the kernel keeps both values of every element in two LDS planes and
evaluates only the elements whose fl(a + 1) the previous MM iteration changed (csrc/tclip_kernels.hip, k_mm_reuse).
`tclip_debug_set_mm_reuse`: 0 = k_mm_live for the whole first outer iteration, 1 = the default, 2 = the default with
a 64-entry index queue (every iteration with more than 64 dirty elements takes the overflow path).  Results never
depend on the mode: every comparison here is bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("alpha", "u", "v", "preds", "mm_iters", "criterions")


def _set_reuse(mode):
    from tclip_amd import _capi
    _capi.check(_capi.lib().tclip_debug_set_mm_reuse(mode), "tclip_debug_set_mm_reuse")


def _last_reuse():
    """(entries evaluated, element-updates executed) by k_mm_reuse in the last collected profile"""
    from tclip_amd import _capi
    out = (ctypes.c_uint64 * 2)()
    _capi.check(_capi.lib().tclip_profile_last_mm_reuse(out), "tclip_profile_last_mm_reuse")
    return int(out[0]), int(out[1])


def _mm_launch_names(fn):
    """kernel names of the launches `fn` makes, from torch's profiler: which MM kernel a test really ran"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if "k_mm_" in e.name}


def _run_modes(modes, x_q, x_s=None, y_s=None, **kw):
    from tclip_amd import engine
    res = {}
    try:
        for mode in modes:
            _set_reuse(mode)
            res[mode] = engine.run_em_dirichlet(x_q, x_s, y_s, **kw)
            torch.cuda.synchronize()
    finally:
        _set_reuse(1)
    return res


# (K, N, few-shot, hard): 16 lanes per row (65, 100, 196), 32 (300, 397, 620, 750), 64 (1000, 1024)
@pytest.mark.parametrize("K,N,few,hard", [(65, 6, False, False), (100, 6, False, False), (100, 3, True, False), (196, 3, False, False),
                                           (300, 3, False, False), (397, 3, False, True), (620, 2, False, False), (750, 2, False, False),
                                           (1000, 2, False, False), (1024, 2, True, False)])
def test_reuse_kernel_is_invisible(K, N, few, hard):
    """Modes 1 and 2 against mode 0 in every lane layout, two batches, iter_mm = 151: the first outer iteration has chunks
    0 (k_mm_live), 1 and 2 (k_mm_reuse, each starting with a full iteration)."""
    from tclip_amd import synth
    B = 2
    x_q, _ = synth.make_query_tasks(B * N, K, seed=8600 + K, k_eff=(min(4, K) if few else None))
    x_s = y_s = None
    if few:
        x_s, y_s = synth.make_support(B * N, K, 1, seed=8700 + K)
        x_s, y_s = x_s.to(DEV), y_s.squeeze(2).to(DEV)
    res = _run_modes((1, 2, 0), x_q.to(DEV), x_s, y_s, n_batches=B, iters=2, iter_mm=151, lambd=max(1, int(K / 5)) * 75, hard=hard)
    for mode in (1, 2):
        for name in FIELDS:
            assert torch.equal(getattr(res[mode], name), getattr(res[0], name)), (mode, name)
    assert torch.isfinite(res[0].alpha).all()


@pytest.mark.parametrize("K,N", [(100, 4), (1000, 2)])
def test_reuse_kernel_ran_and_skipped(K, N):
    """The profiler's kernel names: k_mm_reuse in modes 1 and 2, not in mode 0; and the kernel's own counters in mode 1:
    it evaluated some entries and fewer than the element-updates it executed.  The ratio is printed, not asserted (it is
    a property of the data)."""
    from tclip_amd import engine, synth
    x_q, _ = synth.make_query_tasks(N, K, seed=8800 + K)
    x = x_q.to(DEV)
    kw = dict(n_batches=1, iters=2, iter_mm=151, lambd=int(K / 5) * 75, hard=False)
    names = {}
    try:
        for mode in (0, 1, 2):
            _set_reuse(mode)
            names[mode] = _mm_launch_names(lambda: engine.run_em_dirichlet(x, **kw))
        _set_reuse(1)
        engine.profile_enable(True)
        try:
            engine.profile_collect()
            engine.run_em_dirichlet(x, **kw)
            _, _, _, total = engine.profile_collect()
            kernels = engine.profile_last_kernels()
            evaluated, updates = _last_reuse()
        finally:
            engine.profile_enable(False)
    finally:
        _set_reuse(1)
    for mode in (1, 2):
        assert any("k_mm_reuse" in n for n in names[mode]), (mode, names[mode])
    assert not any("k_mm_reuse" in n for n in names[0]), names[0]
    assert any("k_mm_live" in n for n in names[1]), "chunk 0 stays on k_mm_live"
    print(f"K={K}: k_mm_reuse evaluated {evaluated} of {updates} element-updates ({evaluated / max(updates, 1):.3f})")
    assert 0 < evaluated < updates
    # the kernel's updates are booked under k_mm_live (the first outer iteration), and the total counts every executed update
    assert set(kernels) == {"k_mm_live", "k_mm_split"}
    assert updates < kernels["k_mm_live"][3] and kernels["k_mm_live"][3] + kernels["k_mm_split"][3] == total


def test_reuse_kernel_equals_oracle():
    """K = 100, three tasks, iter_mm = 230 (chunks 1 .. 4 of the first outer iteration in k_mm_reuse) against the C++ oracle."""
    from oracle import c_oracle
    from tclip_amd import engine, synth
    K, N = 100, 3
    kw = dict(iters=2, iter_mm=230, lambd=int(K / 5) * 75)
    x_q, _ = synth.make_query_tasks(N, K, seed=8900)
    _set_reuse(1)
    res = engine.run_em_dirichlet(x_q.to(DEV), n_batches=1, hard=False, **kw)
    torch.cuda.synchronize()
    ref = c_oracle.run(x_q.numpy(), **kw)
    assert np.array_equal(res.mm_iters[0].cpu().numpy(), ref["mm_iters"])
    assert np.array_equal(res.alpha.cpu().numpy(), ref["alpha"]), "alpha differs from the oracle's"
    assert np.array_equal(res.u.cpu().numpy(), ref["u"]) and np.array_equal(res.v.cpu().numpy(), ref["v"])
    assert np.array_equal(res.criterions[0].cpu().numpy(), ref["criterions"])


@pytest.mark.parametrize("K,N", [(100, 4), (397, 2), (1000, 2)])
def test_reuse_kernel_with_nan_and_stopped_batches(K, N):
    """A NaN feature (the wavefront's generic path, after which the kernel evaluates everything anew) and a batch that stops
    while the other runs on (rows of a stopped batch are skipped): mode 1 against mode 0."""
    from tclip_amd import engine, synth
    B, iter_mm = 2, 400
    x_q, _ = synth.make_query_tasks(B * N, K, seed=8300 + K)
    x_q[N:] = torch.softmax(torch.log(x_q[N:]) * 0.02, -1)      # nearly flat: its MM loop never converges within iter_mm
    x_bad = x_q.clone()
    x_bad[1, 3, 5] = float("nan")
    kw = dict(n_batches=B, iters=3, iter_mm=iter_mm, lambd=int(K / 5) * 75, hard=False)
    out = {}
    try:
        for mode in (0, 1):
            _set_reuse(mode)
            out[mode] = (engine.run_em_dirichlet(x_q.to(DEV), **kw), engine.run_em_dirichlet(x_bad.to(DEV), **kw))
            torch.cuda.synchronize()
    finally:
        _set_reuse(1)
    clean = out[0][0].mm_iters.cpu().numpy()
    assert ((clean[0] < iter_mm) & (clean[1] == iter_mm)).any(), f"one batch should stop while the other runs on: {clean.tolist()}"
    assert torch.isnan(out[0][1].alpha[1]).any(), "the NaN feature must reach alpha (the generic path ran)"
    for a, b in zip(out[0], out[1]):
        for name in ("alpha", "u", "v", "preds", "mm_iters"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0)), name


def test_reuse_kernel_with_small_parameters_and_stop_test():
    """Few-shot, K = 100, one shot, sharpened features (the smallest parameters a finite input gives), iter_mm = 101: the
    measuring iteration (100) is the last one of a k_mm_reuse launch.  Mode 1 against mode 0.

    The smallest parameter is printed.  It does NOT reach 1e-11, the threshold of the curvature's constant branch (phase C's
    kTiny form): the features enter as log(x + 1e-15) >= -34.5, so y >= -34.5 and the fixed point digamma(a) - digamma(s) = y
    keeps a above ~1/35 (seen: 0.030 here, 0.032 with half of every feature row set to 0, 0.052 unsharpened).  No input
    through the engine's entry points was found that takes a live row's in-domain parameter to 1e-11; the kTiny form of
    this kernel is the one k_mm_split uses (pk_mm_update_stage1_given<true>), with the same arguments."""
    from tclip_amd import synth
    K, N, B = 100, 3, 2
    x_q, _ = synth.make_query_tasks(B * N, K, seed=9300, k_eff=4)
    x_s, y_s = synth.make_support(B * N, K, 1, seed=9400)
    x_q = torch.softmax(torch.log(x_q) * 6.0, -1)
    x_s = torch.softmax(torch.log(x_s) * 6.0, -1)
    kw = dict(n_batches=B, iters=2, iter_mm=101, lambd=int(K / 5) * 75, hard=False)
    res = _run_modes((1, 0), x_q.to(DEV), x_s.to(DEV), y_s.squeeze(2).to(DEV), **kw)
    print(f"smallest parameter: {res[0].alpha.min().item():.3e}")
    for name in FIELDS:
        assert torch.equal(getattr(res[1], name), getattr(res[0], name)), name
    assert torch.isfinite(res[0].alpha).all()
