"""Few-shot PADDLE on probability features and on visual features, drop-in for the reference's
src/methods/few_shot/paddle.py.  Same constructor / run_task / logs contract; the
loop runs in libtclip.so (tclip_paddle_run; tclip_paddle_visual_run when args.use_softmax_feature
is False; run_tables, the task-batch loop's entry, reads the support rows from the feature table in
place through tclip_paddle_run_tasks / tclip_paddle_visual_run_tasks).  `args.lambd` is the method's own float (paddle.yaml), not the class-count formula of
EM-Dirichlet.  On visual features the rows are D-dim embeddings and the class count is
args.num_classes_test, as in the reference; the reference's text-prompt u (:186-196) is overwritten by
the first u_update before anything reads it, so no text features are asked for."""
from src.methods._em_dirichlet_base import EMDirichletBase, FewShotMixin
from tclip_amd import engine
from tclip_amd.reporting import VAL_PARAM


class BASE(FewShotMixin, EMDirichletBase):
    FEW_SHOT = True


class PADDLE(BASE):
    BANNER = "PADDLE"
    ARG_DEFAULTS = {"iter_mm": 0}          # paddle.yaml has no iter_mm
    IN_PLACE_FEATURES = ("softmax", "visual")
    SWEEP_ATTR = VAL_PARAM["PADDLE"]

    def __init__(self, model, device, log_file, args):
        super().__init__(model=model, device=device, log_file=log_file, args=args)
        self.lambd = args.lambd       # paddle.py:26

    def run_method(self, support, query, y_s, y_q, n_batches=1):
        if self.args.use_softmax_feature:
            call = lambda: engine.run_paddle(query, support, y_s, iters=self.iter, lambd=self.lambd)      # noqa: E731
        else:
            call = lambda: engine.run_paddle_visual(query, support, y_s, n_class=self.args.num_classes_test,      # noqa: E731
                                                    iters=self.iter, lambd=self.lambd)
        self._run(call, query.shape[0], y_q)

    def run_tables(self, table_s, s_idx, table_q, q_idx, cols, y_s, y_q, n_batches=1):
        """run_method for the task-batch loop (Evaluator_few_shot.evaluate_tasks) on either feature kind: the support / query
        rows of task t are table_s[s_idx[t]] / table_q[q_idx[t]], on softmax features with the columns permuted by cols[t]
        (cols is None on visual features, whose labels are not re-indexed either).  The (T,S,D) support tensor is never
        built.  Overrides FewShotMixin.run_tables, which drives the EM-Dirichlet engine."""
        if self.args.use_softmax_feature:
            call = lambda: engine.run_paddle_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=self.iter,      # noqa: E731
                                                   lambd=self.lambd)
        else:
            if cols is not None:
                raise ValueError("PADDLE on visual features permutes no columns: cols must be None")
            call = lambda: engine.run_paddle_visual_tasks(table_q, q_idx, table_s, s_idx, y_s,      # noqa: E731
                                                          n_class=self.args.num_classes_test, iters=self.iter, lambd=self.lambd)
        self._run(call, q_idx.shape[0], y_q)

    def _sweep(self, values, table_s, s_idx, table_q, q_idx, cols, y_s, n_batches):
        """run_tables' engine call for a list of lambd values (FewShotMixin.run_tables_sweep)"""
        if not self.args.use_softmax_feature and cols is not None:
            raise ValueError("PADDLE on visual features permutes no columns: cols must be None")
        return engine.sweep_paddle_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=self.iter, values=values,
                                         n_class=None if self.args.use_softmax_feature else self.args.num_classes_test)

    def _banner(self):
        return " ==> Executing PADDLE with LAMBDA = {} and T = {}".format(self.lambd, self.args.T)

    def _run(self, call, n_task, y_q):
        """the engine call, then the reference's bookkeeping"""
        self._finish(*self._execute(self._banner(), call), n_task, y_q)

    def _finish(self, result, total, n_task, y_q, n_batches=1):
        self.u, self.v, self.w, self.preds = result
        # cumulative wall time per iteration over n_task (paddle.py:214-216)
        self.timestamps += self.spread_time("cumulative", total, self.iter, n_task)
        self.criterions = [0.0] * self.iter       # the reference compares u with a copy of itself (:211-212)
        self.compute_acc(y_q=y_q)
