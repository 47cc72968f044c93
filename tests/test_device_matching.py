"""CPU: the device matching of clusters to classes (tclip_match_clusters) is declared, exported and bound, checks its
arguments before it touches a device, and is an opt-in of the engine, the drop-in classes and main_features.py."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from tclip_amd import _capi, engine

ENTRIES = ("tclip_match_clusters_workspace_bytes", "tclip_match_clusters")


def _header():
    return open(os.path.join(ROOT, "include", "tclip.h")).read()


def test_entries_are_declared_listed_and_bound():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    later = text[text.index("later, without a new number"):text.index("(every entry point of an earlier version")]
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/tclip.h"
        assert re.search(r"\b%s\b" % name, later), f"{name} is missing from the header's list of later additions"
        assert name in _capi.EXPORTS
    assert re.search(r"#define\s+TCLIP_ABI_VERSION\s+5\b", text)
    assert _capi.lib().tclip_abi_version() == 5


def test_built_library_exports_the_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in ENTRIES:
        assert name in symbols, f"{name} is not exported by libtclip.so"


def test_argument_checks_need_no_device():
    lib = _capi.lib()
    P = ctypes.c_void_p(4096)          # never dereferenced: the checks fail first
    ok = dict(T=4, Q=75, K=10, graph=1, c_stride=10)

    def call(T, Q, K, graph, c_stride, ptr=P):
        return lib.tclip_match_clusters(T, Q, K, ptr, ptr, ptr, ptr, ptr, graph, c_stride, ptr, ptr, ptr, None, 0, None)

    assert call(**ok, ptr=None) == 1
    assert b"null pointer" in lib.tclip_last_error()
    for hole in range(8):              # each pointer on its own
        ptrs = [P] * 8
        ptrs[hole] = None
        assert lib.tclip_match_clusters(4, 75, 10, *ptrs[:5], 1, 10, *ptrs[5:], None, 0, None) == 1
    assert call(**dict(ok, K=1, c_stride=1)) == 1
    assert b"n_class" in lib.tclip_last_error()
    assert call(**dict(ok, K=1025)) == 1
    assert call(**dict(ok, c_stride=11)) == 1          # min(Q, K) = K = 10
    assert b"c_stride" in lib.tclip_last_error()
    assert call(**dict(ok, Q=6, c_stride=7)) == 1      # min(Q, K) = Q = 6
    assert call(**dict(ok, c_stride=0)) == 1
    assert call(**dict(ok, T=0)) == 1
    assert call(**dict(ok, Q=0)) == 1
    # the kernel keeps a task in LDS: no global workspace
    assert lib.tclip_match_clusters_workspace_bytes(1250, 75, 1000, 75) == 0


def test_matching_is_a_keyword_only_opt_in():
    for fn in (engine.clustering_accuracy, engine.clustering_accuracy_visual):
        p = inspect.signature(fn).parameters["matching"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "host"
    x, preds, y = torch.rand(2, 75, 10), torch.zeros(2, 75, dtype=torch.int32), torch.zeros(2, 75, dtype=torch.int64)
    with pytest.raises(ValueError, match="matching"):
        engine.clustering_accuracy(x, preds, y, matching="bogus")
    with pytest.raises(ValueError, match="matching"):
        engine.clustering_accuracy_visual(torch.rand(2, 75, 16), preds, y, torch.rand(10, 16), 30.0, matching="bogus")
    with pytest.raises(RuntimeError, match="must live on the GPU"):         # a valid value goes on to the device check
        engine.clustering_accuracy(x, preds, y, matching="device")


def test_match_status_ok_names_the_failed_tasks():
    good = torch.tensor([0.5, 1.0, 0.0])
    assert torch.equal(engine.match_status_ok(good), good)
    with pytest.raises(RuntimeError, match=r"\[1, 3\]"):
        engine.match_status_ok(torch.tensor([0.5, float("nan"), 0.25, float("nan")]))
    with pytest.raises(RuntimeError, match=r"\[2\]"):                      # the (T, 1) columns the method classes keep
        engine.match_status_ok(torch.tensor([[0.5], [0.1], [float("nan")]]))


def test_drop_in_classes_and_cli_carry_the_flag():
    import main_features
    from src.methods.zero_shot.soft_kmeans import SOFT_KMEANS
    from src.utils import CfgNode
    _, cfg = main_features.parse_args(["--opts", "device_matching", "True", "method", "soft_kmeans"])
    assert cfg.device_matching is True
    _, cfg = main_features.parse_args(["--opts", "method", "soft_kmeans"])
    assert getattr(cfg, "device_matching", False) is False
    assert "device_matching" not in main_features.MAIN_DEFAULTS
    a = CfgNode(iter=2, num_classes_test=10, n_class=10, n_query=75, k_eff=5, T=30, use_softmax_feature=True, graph_matching=True)
    m = SOFT_KMEANS(model=None, device=torch.device("cpu"), log_file=None, args=a)
    assert m._matching() == "host"
    a.device_matching = True
    assert m._matching() == "device"


def test_flag_is_optional_for_dict_style_args():
    """a caller's args may be a dict with attribute access, whose missing key is a KeyError and not an AttributeError"""
    from src.methods.zero_shot.soft_kmeans import SOFT_KMEANS

    class Args(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    a = Args(iter=2, iter_mm=0, num_classes_test=10, n_class=10, n_query=75, k_eff=5, T=30, use_softmax_feature=True,
             graph_matching=True)
    m = SOFT_KMEANS(model=None, device=torch.device("cpu"), log_file=None, args=a)
    assert m._matching() == "host"
    a.device_matching = True
    assert m._matching() == "device"
    a.device_matching = False
    assert m._matching() == "host"
