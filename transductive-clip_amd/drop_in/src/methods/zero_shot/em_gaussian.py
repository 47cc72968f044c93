"""Zero-shot EM_GAUSSIAN on probability features, drop-in for the reference's
src/methods/zero_shot/em_gaussian.py: SOFT_KMEANS plus the class-proportion term of
EM-Dirichlet.  Same constructor / run_task / logs contract; the loop runs in libtclip.so
(tclip_em_gaussian_run).  On visual features (use_softmax_feature: False) the initial assignment comes from the text
features (reference :188-198; src/methods/_visual.py) and the loop runs in the embedding space (tclip_kmeans_visual_run)."""
from src.methods._em_dirichlet_base import EMDirichletBase, ZeroShotMixin
from tclip_amd import engine


class BASE(ZeroShotMixin, EMDirichletBase):
    pass


class EM_GAUSSIAN(BASE):
    BANNER = "EM_GAUSSIAN"
    ARG_DEFAULTS = {"iter_mm": 0}          # em_gaussian.yaml has no iter_mm; lambd = int(K/5) * n_query (:20)

    def run_method(self, query, y_q, n_batches=1):
        kw = dict(iters=self.iter, temperature=self.args.T, lambd=self.lambd)
        (self.u, self.v, self.w, self.preds), total, text = self._run_clustering(
            query, lambda: engine.run_em_gaussian(query, **kw), lambda u0: engine.run_em_gaussian_visual(query, u0, **kw))
        # the reference restarts its clock every iteration (em_gaussian.py:204-224)
        self.timestamps += self.spread_time("share", total, self.iter, query.shape[0])
        self.criterions = [0.0] * self.iter       # the reference compares u with a copy of itself
        self.compute_acc_clustering(query, y_q, text)
