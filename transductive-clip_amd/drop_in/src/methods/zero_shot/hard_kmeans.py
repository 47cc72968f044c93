"""Zero-shot HARD_KMEANS on probability features, drop-in for the reference's
src/methods/zero_shot/hard_kmeans.py.  Same constructor / run_task / logs contract
as the EM-Dirichlet classes; the loop runs in libtclip.so (tclip_hard_kmeans_run).  On visual features
(use_softmax_feature: False) the initial assignment comes from the text features (reference :172-184;
src/methods/_visual.py) and the loop runs in the embedding space (tclip_kmeans_visual_run)."""
from src.methods._em_dirichlet_base import EMDirichletBase, ZeroShotMixin
from tclip_amd import engine


class BASE(ZeroShotMixin, EMDirichletBase):
    pass


class HARD_KMEANS(BASE):
    BANNER = "HARD_KMEANS"
    ARG_DEFAULTS = {"iter_mm": 0}          # hard_kmeans.yaml has no iter_mm

    def run_method(self, query, y_q, n_batches=1):
        (self.u, self.w, self.preds, crit), total, text = self._run_clustering(
            query, lambda: engine.run_hard_kmeans(query, iters=self.iter, n_batches=n_batches),
            lambda u0: engine.run_hard_kmeans_visual(query, u0, iters=self.iter, n_batches=n_batches))
        crit = crit.cpu()
        # the reference records every iteration twice (hard_kmeans.py:198-204)
        self.timestamps += self.spread_time("twice", total, self.iter, query.shape[0])
        self.criterions = [crit[0, i] for i in range(self.iter) for rep in range(2)]
        self.compute_acc_clustering(query, y_q, text)
