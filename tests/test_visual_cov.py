"""CPU: the host side of EM_GAUSSIAN_COV on visual features at the engine level - the two C entries in the header, the binding
and the library, their argument checks (no device needed: every check comes before the first launch), the engine function's
validation, and the torch restatement the GPU sweep compares against (tests/helpers/visual_cov.py), pinned bit for bit to the
reference-made fixtures of tests/golden/make_golden_visual_cov.py by running the whole loop from their u0."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden_names
from helpers import visual, visual_cov

ENTRIES = ("tclip_em_gaussian_cov_visual_workspace_bytes", "tclip_em_gaussian_cov_visual_run")
FULL = ["full_vis_emgc_D512_K10_N3", "full_vis_emgc_D1024_K37_N2", "full_vis_emgc_D768_K100_N1", "full_vis_emgc_D5_K4_N2"]
LEAN = "lean_vis_emc_D1024_K1000_N1"
ERR_ARG, ERR_WORKSPACE = 1, 2


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_entries_in_header_and_binding():
    from tclip_amd import _capi
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _capi.EXPORTS
    assert "#define TCLIP_ABI_VERSION 5" in header


def test_entries_exported_by_the_library():
    from tclip_amd import _capi
    assert os.path.exists(_capi.LIB_PATH), "libtclip.so is missing: run build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert _capi.lib().tclip_abi_version() == 5


def test_argument_checks_come_before_any_launch():
    from tclip_amd import _capi
    lib = _capi.lib()
    zs = _capi.Problem(1, 4, 75, 10, 0, 5, 1, 150, 0)
    fs = _capi.Problem(1, 4, 75, 10, 1, 5, 1, 150, 0)
    P = ctypes.c_void_p(4096)          # 256-byte aligned, never dereferenced: the checks fail first
    ref = ctypes.byref
    run, query = lib.tclip_em_gaussian_cov_visual_run, lib.tclip_em_gaussian_cov_visual_workspace_bytes
    need = query(ref(zs), 512)
    assert need > 0 and need % 256 == 0
    assert need == query(ref(zs), 1) == query(ref(zs), 1024)          # no region holds feature rows
    assert need > lib.tclip_visual_workspace_bytes(ref(zs), 512)       # the half log-determinants [T, K]
    # the workspace query returns 0 on bad input
    for p, dim in ((zs, 0), (zs, 1025), (fs, 512), (_capi.Problem(1, 4, 75, 1025, 0, 5, 1, 150, 0), 512),
                   (_capi.Problem(1, 4, 75, 1, 0, 5, 1, 150, 0), 512)):
        assert query(ref(p), dim) == 0
    assert query(None, 512) == 0
    # null pointers, each in turn
    for i in range(8):
        args = [P] * 8
        args[i] = None
        assert run(ref(zs), 512, *args, 1 << 30, None) == ERR_ARG and b"null" in lib.tclip_last_error()
    assert run(None, 512, *([P] * 8), 1 << 30, None) == ERR_ARG
    for dim in (0, 1025):
        assert run(ref(zs), dim, *([P] * 8), 1 << 30, None) == ERR_ARG and b"dim" in lib.tclip_last_error()
    assert run(ref(fs), 512, *([P] * 8), 1 << 30, None) == ERR_ARG and b"zero-shot" in lib.tclip_last_error()
    # one byte short, and misaligned
    assert run(ref(zs), 512, *([P] * 7), P, need - 1, None) == ERR_WORKSPACE and b"workspace" in lib.tclip_last_error()
    assert run(ref(zs), 512, *([P] * 7), ctypes.c_void_p(4096 + 4), need, None) == ERR_WORKSPACE


def test_engine_validates_before_any_launch():
    """shapes first, then the device: all of it without a GPU"""
    from tclip_amd import engine
    x = torch.randn(2, 75, 16)
    with pytest.raises(ValueError, match="cuda"):
        engine.run_em_gaussian_cov_visual(x, torch.rand(2, 75, 4).softmax(-1), iters=3, lambd=0)
    for bad in (torch.rand(2, 74, 4), torch.rand(3, 75, 4), torch.rand(150, 4)):
        with pytest.raises(ValueError, match="u0"):
            engine.run_em_gaussian_cov_visual(x, bad, iters=3, lambd=0)
    with pytest.raises(ValueError, match="1024"):
        engine.run_em_gaussian_cov_visual(torch.randn(1, 75, 1025), torch.rand(1, 75, 4), iters=3, lambd=0)


def test_fixture_names_stay_out_of_the_other_lists():
    for n in FULL + [LEAN]:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 1 << 20
        assert not n.startswith("vis_") and n not in golden_names("") and n not in golden_names("zs_emgc_")


def test_fixtures_satisfy_their_conditions():
    """what the generator asserted, from what it stored: finite outputs, empty clusters at the start of an iteration >= 1 at
    K = 37 and K = 100 (and so rows of w and s that were kept), s at the sum u / eps clamp"""
    s_max = []
    for n in FULL + [LEAN]:
        g = np.load(os.path.join(GOLDEN, n + ".npz"))
        assert str(g["method"]) == "em_gaussian_cov" and int(g["iters"]) == 20 and float(g["T"]) == 30.0
        assert int(g["lambd"]) == int(int(g["K"]) / 5) * 75
        for k in ("u0", "u", "v", "w", "s"):
            if k in g:
                assert np.isfinite(g[k]).all(), (n, k)
        if int(g["K"]) in (37, 100):
            assert int(g["dead_clusters"]) > 0
        s_max.append(float(g["s_max"]))
    assert max(s_max) >= 1e14
    g = np.load(os.path.join(GOLDEN, LEAN + ".npz"))
    x_q, _, _ = visual.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["seed"]))
    assert sha(x_q.numpy()) == str(g["x_q_sha1"])


@pytest.mark.parametrize("name", FULL)
def test_restatement_reproduces_the_reference(name):
    """the whole loop from the fixture's u0: u, v, w, s bit for bit (w and s by digest where the fixture keeps only that); the
    logarithm is the restated one, so that the test asks the same on every host"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x_q, y_q, text = visual.make_tasks(int(g["N"]), int(g["K"]), int(g["D"]), int(g["seed"]))
    assert torch.equal(x_q, torch.from_numpy(g["x_q"]))
    u, v, w, s, preds = visual_cov.run(x_q, torch.from_numpy(g["u0"]), int(g["iters"]), int(g["lambd"]), log=visual_cov.restated_log())
    assert torch.equal(u, torch.from_numpy(g["u"])) and torch.equal(v, torch.from_numpy(g["v"]))
    for k, a in (("w", w), ("s", s)):
        if k in g:
            assert torch.equal(a, torch.from_numpy(g[k])), k
        else:
            assert sha(a.numpy()) == str(g[k + "_sha1"]), k
    assert np.array_equal(preds.numpy(), g["preds"])
