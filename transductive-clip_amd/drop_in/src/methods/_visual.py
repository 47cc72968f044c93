"""Text features for the zero-shot methods on VISUAL features (use_softmax_feature == False).

The reference builds them with clip_weights(model, classnames, template, device) (src/utils.py:363-377): one unit-norm text
embedding per class.  Resolution order here:
  1. args.text_features: a (K, D) tensor, or the path of a .pt / .npy file holding one;
  2. src.utils.clip_weights, when the classes run overlaid on a reference checkout (Level 1), called exactly
     as the reference calls it;
  3. otherwise a ValueError naming text_features.
K must equal args.num_classes_test."""
import os

import numpy as np
import torch


def load_text_features(tf):
    """a tensor, or the (K, D) tensor of a .pt / .npy file"""
    if isinstance(tf, (str, os.PathLike)):
        path = os.fspath(tf)
        if path.endswith(".npy"):
            return torch.from_numpy(np.load(path))
        if path.endswith(".pt"):
            return torch.load(path, map_location="cpu")
        raise ValueError(f"text_features: {path} is neither a .pt nor a .npy file")
    return torch.as_tensor(tf)


def text_features(model, args, device):
    """(K, D) float32 text features on `device` (see the module docstring for where they come from)."""
    tf = getattr(args, "text_features", None)
    if tf is not None:
        text = load_text_features(tf)
    else:
        try:
            from src.utils import clip_weights
        except ImportError:
            clip_weights = None
        if clip_weights is None:
            raise ValueError("visual features (use_softmax_feature: False) need text features: set args.text_features to a "
                             "(K, D) tensor or a .pt / .npy file (main_features.py --text-features), or run the class "
                             "overlaid on a reference checkout whose src.utils.clip_weights can build them")
        text = clip_weights(model, args.classnames, args.template, device)
    text = text.float()
    K = int(args.num_classes_test)
    if text.dim() != 2 or text.shape[0] != K:
        raise ValueError(f"text_features must be ({K}, D) for num_classes_test = {K}, got {tuple(text.shape)}")
    return text.to(device).contiguous()
