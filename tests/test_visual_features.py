"""CPU: the host side of the zero-shot methods on visual features - fixture names, where the text features come from,
the --text-features option, and the methods that still refuse visual features."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, golden_names


def test_visual_fixture_names_stay_out_of_the_existing_lists():
    vis = [f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and "vis_" in f]
    assert len(vis) >= 14
    for prefix in ("", "zs_skm_", "zs_hkm_", "zs_emg_", "zs_"):
        assert not any("vis" in n for n in golden_names(prefix))
    for f in vis:
        assert os.path.getsize(os.path.join(GOLDEN, f + ".npz")) < 1 << 20


def _args(**kw):
    from src.utils import CfgNode
    a = CfgNode(num_classes_test=4, classnames=["a", "b", "c", "d"], template=["a photo of a {}."])
    a.update(kw)
    return a


def test_text_features_from_args_tensor_and_files(tmp_path):
    from src.methods._visual import text_features
    t = torch.randn(4, 16)
    assert torch.equal(text_features(None, _args(text_features=t), "cpu"), t)
    np.save(tmp_path / "t.npy", t.numpy())
    torch.save(t, str(tmp_path / "t.pt"))
    assert torch.equal(text_features(None, _args(text_features=str(tmp_path / "t.npy")), "cpu"), t)
    assert torch.equal(text_features(None, _args(text_features=str(tmp_path / "t.pt")), "cpu"), t)
    with pytest.raises(ValueError, match="num_classes_test"):
        text_features(None, _args(text_features=torch.randn(5, 16)), "cpu")
    with pytest.raises(ValueError, match=r"\.pt"):
        text_features(None, _args(text_features=str(tmp_path / "t.txt")), "cpu")


def test_text_features_fall_back_to_clip_weights_then_fail(monkeypatch):
    import src.utils
    from src.methods._visual import text_features
    assert not hasattr(src.utils, "clip_weights")          # the package's own src.utils: no CLIP model here
    with pytest.raises(ValueError, match="text_features"):
        text_features(None, _args(), "cpu")
    seen = {}

    def clip_weights(model, classnames, template, device):   # a reference checkout's src.utils (Level 1)
        seen.update(model=model, classnames=classnames, template=template, device=device)
        return torch.ones(4, 8, dtype=torch.float16)
    monkeypatch.setattr(src.utils, "clip_weights", clip_weights, raising=False)
    model = object()
    got = text_features(model, _args(), "cpu")
    assert got.dtype == torch.float32 and got.shape == (4, 8)
    assert seen == {"model": model, "classnames": ["a", "b", "c", "d"], "template": ["a photo of a {}."], "device": "cpu"}
    # args.text_features wins over clip_weights
    assert torch.equal(text_features(model, _args(text_features=torch.zeros(4, 3)), "cpu"), torch.zeros(4, 3))


def test_text_features_option():
    sys.path.insert(0, PKG)
    import main_features
    _, cfg = main_features.parse_args(["--text-features", "/x/text.npy", "--opts", "method", "soft_kmeans",
                                       "use_softmax_feature", "False"])
    assert cfg.text_features == "/x/text.npy" and cfg.use_softmax_feature is False
    _, cfg = main_features.parse_args(["--opts", "method", "soft_kmeans"])
    assert getattr(cfg, "text_features", None) is None


@pytest.mark.parametrize("module,cls", [("kl_kmeans", "KL_KMEANS"), ("em_gaussian_cov", "EM_GAUSSIAN_COV")])
def test_kl_kmeans_and_em_gaussian_cov_still_refuse_visual_features(module, cls):
    from src.utils import CfgNode
    mod = __import__(f"src.methods.zero_shot.{module}", fromlist=[cls])
    a = CfgNode(iter=5, num_classes_test=4, n_class=4, n_query=75, k_eff=5, T=30, use_softmax_feature=False,
                graph_matching=True, text_features=torch.randn(4, 8))
    m = getattr(mod, cls)(model=None, device="cuda", log_file=None, args=a)
    with pytest.raises(NotImplementedError):
        m.run_method(torch.randn(1, 75, 8), torch.zeros(1, 75, dtype=torch.long))
