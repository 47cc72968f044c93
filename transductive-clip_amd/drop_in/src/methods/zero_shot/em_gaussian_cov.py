"""Zero-shot EM_GAUSSIAN_COV on probability features, drop-in for the reference's
src/methods/zero_shot/em_gaussian_cov.py: EM_GAUSSIAN with a diagonal inverse
covariance per cluster and no temperature.  Same constructor / run_task / logs contract; the loop
runs in libtclip.so (tclip_em_gaussian_cov_run).  On visual features the engine has an entry of its own
(engine.run_em_gaussian_cov_visual, initial assignment from the text features as in reference :219-229); this class
does not call it yet and refuses them."""
from src.methods._em_dirichlet_base import EMDirichletBase, ZeroShotMixin
from tclip_amd import engine


class BASE(ZeroShotMixin, EMDirichletBase):
    pass


class EM_GAUSSIAN_COV(BASE):
    BANNER = "EM_GAUSSIAN_COV"
    ARG_DEFAULTS = {"iter_mm": 0}          # em_gaussian_cov.yaml has no iter_mm; lambd = int(K/5) * n_query (:20)

    def run_method(self, query, y_q, n_batches=1):
        if not self.args.use_softmax_feature:
            raise NotImplementedError("EM_GAUSSIAN_COV on visual features is not supported: use probability features (use_softmax_feature: True)")
        (self.u, self.v, self.w, self.s, self.preds), total = self._execute(
            " ==> Executing EM_GAUSSIAN_COV with T = {}".format(self.args.T),
            lambda: engine.run_em_gaussian_cov(query, iters=self.iter, lambd=self.lambd))
        # the reference restarts its clock every iteration (em_gaussian_cov.py:234-254)
        self.timestamps += self.spread_time("share", total, self.iter, query.shape[0])
        self.criterions = [0.0] * self.iter       # the reference compares u with a copy of itself
        self.compute_acc_clustering(query, y_q)
