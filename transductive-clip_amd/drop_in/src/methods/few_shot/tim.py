"""Few-shot TIM_GD and ALPHA_TIM, drop-in for the reference's src/methods/few_shot/tim.py: BASE, TIM_GD
(tim.py:90-189) and ALPHA_TIM (tim.py:192-322).  Same constructor / run_task / logs contract; the `iter` Adam steps run in
libtclip.so (tclip_tim_gd_run, tclip_alpha_tim_run) with the gradient in closed form instead of autograd.  The reference's
MKL matmuls and autograd accumulation order leave no bit-level target, so both classes are pinned to the reference within a
float tolerance (tests/test_alpha_tim.py, tests/test_gpu_tim_gd.py).  TIM_GD never reads use_softmax_feature and normalises
nothing: it runs on probability features and on D-dim embeddings alike, the class count being args.num_classes_test.
ALPHA_TIM takes probability features only.  run_tables, which the task-batch loop takes with `in_place_loop: True`, reads both
row sets from the feature tables in place in every Adam step (tclip_tim_gd_run_tasks, tclip_alpha_tim_run_tasks): the same bits
without the (T,S,D) and (T,Q,D) tensors."""
from src.methods._em_dirichlet_base import EMDirichletBase, FewShotMixin
from tclip_amd import engine
from tclip_amd.reporting import VAL_PARAM


# tim.yaml and alpha_tim.yaml have no iter_mm; k_eff only feeds the unused EM-Dirichlet lambd of the shared base
_ARG_DEFAULTS = {"iter_mm": 0, "k_eff": 5}


class BASE(FewShotMixin, EMDirichletBase):
    FEW_SHOT = True


class TIM_GD(BASE):
    BANNER = "TIM"
    ARG_DEFAULTS = _ARG_DEFAULTS
    IN_PLACE_LOOP = ("softmax", "visual")

    def __init__(self, model, device, log_file, args):
        super().__init__(model=model, device=device, log_file=log_file, args=args)
        self.loss_weights = list(args.loss_weights)      # tim.py:29 (.copy())
        self.temp = args.temp
        self.lr = float(args.lr_tim)                     # tim.py:94

    def run_method(self, support, query, y_s, y_q, n_batches=1):
        # rows of D = query.shape[2] elements, D = n_class on probability features and the embedding length otherwise
        self._run(lambda: engine.run_tim_gd(query, support, y_s, n_class=self.args.num_classes_test, iters=self.iter,
                                            temp=self.temp, lr=self.lr, loss_weights=self.loss_weights, n_batches=n_batches),
                  query.shape[0], y_q)

    def run_tables(self, table_s, s_idx, table_q, q_idx, cols, y_s, y_q, n_batches=1):
        """run_method for the task-batch loop (Evaluator_few_shot.evaluate_tasks with in_place_loop): the support / query rows
        of task t are table_s[s_idx[t]] / table_q[q_idx[t]], on softmax features with the columns permuted by cols[t] (None on
        visual features, whose labels are not re-indexed either).  Neither (T,S,D) nor (T,Q,D) is built: the table rows are
        read in every Adam step.  Overrides FewShotMixin.run_tables, which drives the EM-Dirichlet engine."""
        self._run(lambda: engine.run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, n_class=self.args.num_classes_test,
                                                  iters=self.iter, temp=self.temp, lr=self.lr, loss_weights=self.loss_weights,
                                                  n_batches=n_batches),
                  q_idx.shape[0], y_q)

    def _run(self, call, n_task, y_q):
        """the engine call, then the reference's bookkeeping"""
        (self.weights, self.logits_q, self.preds, crit), total = self._execute(" ==> Executing TIM with T = {}".format(self.args.T), call)
        # cumulative wall time per iteration over n_task (tim.py:184-186)
        self.timestamps += self.spread_time("cumulative", total, self.iter, n_task)
        crit = crit.cpu().numpy()                        # (iter, n_task): mean_class ||w_old - w|| of every task (tim.py:181)
        self.criterions_per_task = crit
        self.criterions = list(crit)
        self.compute_acc(y_q=y_q)                        # argmax of the last iteration's query logits (tim.py:189)


class ALPHA_TIM(BASE):
    BANNER = "ALPHA_TIM"
    ARG_DEFAULTS = _ARG_DEFAULTS
    IN_PLACE_LOOP = ("softmax",)
    SWEEP_ATTR = VAL_PARAM["ALPHA_TIM"]
    _VISUAL = "ALPHA_TIM here takes probability features (use_softmax_feature: True, feature dimension = n_class)"

    def __init__(self, model, device, log_file, args):
        super().__init__(model=model, device=device, log_file=log_file, args=args)
        self.loss_weights = list(args.loss_weights)      # tim.py:29 (.copy())
        self.temp = args.temp
        self.lr = float(args.lr_alpha_tim)               # tim.py:196
        self.entropies = list(args.entropies)
        self.alpha_value = args.alpha_value

    def run_method(self, support, query, y_s, y_q, n_batches=1):
        if query.shape[2] != self.args.num_classes_test:
            raise NotImplementedError(self._VISUAL)
        self._run(lambda: engine.run_alpha_tim(query, support, y_s, iters=self.iter, temp=self.temp, lr=self.lr,
                                               alpha_value=self.alpha_value, loss_weights=self.loss_weights,
                                               entropies=self.entropies, n_batches=n_batches),
                  query.shape[0], y_q, n_batches)

    def run_tables(self, table_s, s_idx, table_q, q_idx, cols, y_s, y_q, n_batches=1):
        """run_method for the task-batch loop (Evaluator_few_shot.evaluate_tasks with in_place_loop), as TIM_GD.run_tables;
        visual features are refused as run_method refuses them."""
        if table_q.shape[1] != self.args.num_classes_test:
            raise NotImplementedError(self._VISUAL)
        self._run(lambda: engine.run_alpha_tim_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=self.iter, temp=self.temp,
                                                     lr=self.lr, alpha_value=self.alpha_value, loss_weights=self.loss_weights,
                                                     entropies=self.entropies, n_batches=n_batches),
                  q_idx.shape[0], y_q, n_batches)

    def _sweep(self, values, table_s, s_idx, table_q, q_idx, cols, y_s, n_batches):
        """run_tables' engine call for a list of alpha values (FewShotMixin.run_tables_sweep); visual features are refused as
        run_tables refuses them"""
        if table_q.shape[1] != self.args.num_classes_test:
            raise NotImplementedError(self._VISUAL)
        return engine.sweep_alpha_tim_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=self.iter, temp=self.temp, lr=self.lr,
                                            values=values, loss_weights=self.loss_weights, entropies=self.entropies,
                                            n_batches=n_batches)

    def _banner(self):
        return " ==> Executing ALPHA_TIM with ALPHA = {} and T = {}".format(self.alpha_value, self.args.T)

    def _run(self, call, n_task, y_q, n_batches):
        """the engine call, then the reference's bookkeeping"""
        self._finish(*self._execute(self._banner(), call), n_task, y_q, n_batches)

    def _finish(self, result, total, n_task, y_q, n_batches=1):
        self.weights, self.logits_q, self.preds, crit = result
        # cumulative wall time per iteration over n_task (tim.py:317-319)
        self.timestamps += self.spread_time("cumulative", total, self.iter, n_task)
        crit = crit.cpu().numpy()                        # (n_batches, iter): mean_{task,class} ||w_old - w||
        self.criterions_per_batch = crit
        self.criterions = list(crit.mean(0)) if n_batches > 1 else list(crit[0])
        self.compute_acc(y_q=y_q)                        # argmax of the last iteration's query logits (tim.py:321)
