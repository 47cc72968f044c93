"""Zero-shot KL_KMEANS on probability features, drop-in for the reference's
src/methods/zero_shot/kl_kmeans.py.  Same constructor / run_task / logs contract; the
loop runs in libtclip.so (tclip_kl_kmeans_run).  Visual features are refused for good: the KL divergence of
embeddings that are not on the simplex is undefined (the reference's own branch, :148-158, only changes the
initial assignment)."""
from src.methods._em_dirichlet_base import EMDirichletBase, ZeroShotMixin
from tclip_amd import engine


class BASE(ZeroShotMixin, EMDirichletBase):
    pass


class KL_KMEANS(BASE):
    BANNER = "KL KMEANS"
    ARG_DEFAULTS = {"iter_mm": 0}          # kl_kmeans.yaml has no iter_mm

    def run_method(self, query, y_q, n_batches=1):
        if not self.args.use_softmax_feature:
            raise NotImplementedError("KL_KMEANS needs probability features: the KL divergence of visual embeddings (not on the simplex) is undefined")
        (self.u, self.w, self.preds, crit), total = self._execute(
            " ==> Executing KL KMEANS with T = {}".format(self.args.T),
            lambda: engine.run_kl_kmeans(query, iters=self.iter, n_batches=n_batches))
        crit = crit.cpu()
        # the reference records every iteration twice (kl_kmeans.py:178-187)
        self.timestamps += self.spread_time("twice", total, self.iter, query.shape[0])
        self.criterions = [crit[0, i] for i in range(self.iter) for rep in range(2)]
        self.compute_acc_clustering(query, y_q)
