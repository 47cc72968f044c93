"""Inductive zero-shot CLIP on probability features, drop-in for the reference's
src/methods/zero_shot/inductive_clip.py (the baseline every transductive method is compared with):
no adaptation, u = the query features, prediction = their arg-max, plain accuracy (no cluster
matching).  The arg-max runs in libtclip.so (tclip_argmax_rows).  On visual features (use_softmax_feature: False)
u = softmax_k(T * (x/||x||) . text_k) (reference :115-124; tclip_visual_init) with the text features of
src/methods/_visual.py."""
import numpy as np
import torch

from src.methods._em_dirichlet_base import MethodBase, ZeroShotMixin
from tclip_amd import engine


class BASE(ZeroShotMixin, MethodBase):
    LOGGER_NAME = __name__

    def compute_acc(self, y_q):
        self.preds = engine.argmax_rows(self.u)
        super().compute_acc(y_q)

    def get_logs(self):
        self.criterions = torch.stack(self.criterions, dim=0).cpu().numpy()
        self.test_acc = torch.cat(self.test_acc, dim=1).cpu().numpy()
        return {'timestamps': np.array(self.timestamps).mean(), 'criterions': self.criterions,
                'acc': self.test_acc}


class CLIP(BASE):
    def run_method(self, query, y_q, n_batches=1):
        dev = self._cuda_device()
        text = None if self.args.use_softmax_feature else self._text_features(dev)
        self.logger.info(" ==> Executing CLIP")
        self.u = query if text is None else engine.visual_init(query, text, self.args.T)
        self.record_convergence(new_time=0, criterions=torch.zeros(()))      # ||u - copy of u|| (:126-128)
        self.compute_acc(y_q)
