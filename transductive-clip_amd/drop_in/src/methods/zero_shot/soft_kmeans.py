"""Zero-shot SOFT_KMEANS on probability features, drop-in for the reference's
src/methods/zero_shot/soft_kmeans.py (BASELINE config 3's second method).
Same constructor / run_task / logs contract as the EM-Dirichlet classes; the loop runs in
libtclip.so (tclip_soft_kmeans_run).  On visual features (use_softmax_feature: False) the initial assignment comes from the
text features (reference :185-197; src/methods/_visual.py) and the loop runs in the embedding space
(tclip_kmeans_visual_run)."""
from src.methods._em_dirichlet_base import EMDirichletBase, ZeroShotMixin
from tclip_amd import engine


class BASE(ZeroShotMixin, EMDirichletBase):
    pass


class SOFT_KMEANS(BASE):
    BANNER = "SOFT K-MEANS"
    ARG_DEFAULTS = {"iter_mm": 0}          # soft_kmeans.yaml has no iter_mm

    def run_method(self, query, y_q, n_batches=1):
        (self.u, self.w, self.preds), total, text = self._run_clustering(
            query, lambda: engine.run_soft_kmeans(query, iters=self.iter, temperature=self.args.T),
            lambda u0: engine.run_soft_kmeans_visual(query, u0, iters=self.iter, temperature=self.args.T))
        # the reference restarts its clock every iteration (soft_kmeans.py:203-216)
        self.timestamps += self.spread_time("share", total, self.iter, query.shape[0])
        self.criterions = [0.0] * self.iter       # the reference compares u with a copy of itself
        self.compute_acc_clustering(query, y_q, text)
