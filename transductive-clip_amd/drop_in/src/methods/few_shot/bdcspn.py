"""Few-shot BD-CSPN (prototype rectification) on probability features and on visual features, drop-in for the reference's
src/methods/few_shot/bdcspn.py.  Same constructor / run_task / logs contract
(args.norm_type, args.temp, args.n_class; one timestamp, one zero criterion, plain accuracy); the
whole pass runs in libtclip.so, all tasks of the batch at once instead of the reference's per-task
Python loop (:124-141): tclip_bdcspn_run when the feature width equals args.n_class, tclip_bdcspn_visual_run
for D-dim embeddings otherwise (the reference never looks at use_softmax_feature here).  run_tables, which the task-batch
loop takes with `in_place_support: True`, reads both row sets from the feature tables in place (tclip_bdcspn_run_tasks /
tclip_bdcspn_visual_run_tasks): the same bits without the (T,S,D) and (T,Q,D) tensors."""
import numpy as np
import torch

from src.methods._em_dirichlet_base import FewShotMixin, MethodBase
from tclip_amd import engine
from tclip_amd.reporting import VAL_PARAM


class BDCSPN(FewShotMixin, MethodBase):
    LOGGER_NAME = __name__
    IN_PLACE_SUPPORT = ("softmax", "visual")
    SWEEP_ATTR = VAL_PARAM["BDCSPN"]

    def __init__(self, model, device, log_file, args):
        super().__init__(model=model, device=device, log_file=log_file, args=args)
        self.norm_type = args.norm_type
        self.temp = args.temp
        self.n_class = args.n_class

    def get_logs(self):
        self.criterions = torch.stack(self.criterions, dim=0).cpu().numpy()
        self.test_acc = torch.cat(self.test_acc, dim=1).cpu().numpy()
        return {'timestamps': np.array(self.timestamps).mean(), 'criterions': self.criterions,
                'acc': self.test_acc}

    def run_task(self, task_dic, shot=None):
        # the reference normalises here (:165-166) and hands the result to run_method; the engine does both in run_batch
        return super().run_task(task_dic, shot)

    def run_method(self, support, query, y_s, y_q, shot=None, n_batches=1):
        """Reference semantics (:172-200): `support` and `query` are already normalised."""
        self.run_batch(support, query, y_s, y_q, norm_type="UN")

    def run_batch(self, support, query, y_s, y_q, n_batches=1, norm_type=None):
        """Normalisation + BD-CSPN for all tasks at once (what run_task does for one batch)."""
        norm_type = self.norm_type if norm_type is None else norm_type
        if query.shape[2] == self.n_class:
            call = lambda: engine.run_bdcspn(query, support, y_s, temp=self.temp, norm_type=norm_type)      # noqa: E731
        else:
            call = lambda: engine.run_bdcspn_visual(query, support, y_s, n_class=self.n_class, temp=self.temp,      # noqa: E731
                                                    norm_type=norm_type)
        self._run(call, y_q)

    def run_tables(self, table_s, s_idx, table_q, q_idx, cols, y_s, y_q, n_batches=1):
        """run_batch for the task-batch loop (Evaluator_few_shot.evaluate_tasks with in_place_support): the support / query
        rows of task t are table_s[s_idx[t]] / table_q[q_idx[t]], on softmax features with the columns permuted by cols[t]
        (None on visual features, whose labels are not re-indexed either).  Neither (T,S,D) nor (T,Q,D) is built.  Overrides
        FewShotMixin.run_tables, which drives the EM-Dirichlet engine."""
        if table_q.shape[1] == self.n_class:
            call = lambda: engine.run_bdcspn_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, temp=self.temp,      # noqa: E731
                                                   norm_type=self.norm_type)
        else:
            if cols is not None:
                raise ValueError("BDCSPN on visual features permutes no columns: cols must be None")
            call = lambda: engine.run_bdcspn_visual_tasks(table_q, q_idx, table_s, s_idx, y_s, n_class=self.n_class,      # noqa: E731
                                                          temp=self.temp, norm_type=self.norm_type)
        self._run(call, y_q)

    def _sweep(self, values, table_s, s_idx, table_q, q_idx, cols, y_s, n_batches):
        """run_tables' engine call for a list of temp values (FewShotMixin.run_tables_sweep)"""
        visual = table_q.shape[1] != self.n_class
        if visual and cols is not None:
            raise ValueError("BDCSPN on visual features permutes no columns: cols must be None")
        return engine.sweep_bdcspn_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, values=values, norm_type=self.norm_type,
                                         n_class=self.n_class if visual else None)

    def _banner(self):
        return " ==> Executing BD-CSPN"

    def _run(self, call, y_q):
        """the engine call, then the reference's bookkeeping"""
        self._finish(*self._execute(self._banner(), call), None, y_q)

    def _finish(self, result, total, n_task, y_q, n_batches=1):
        self.prototypes, self.u, self.preds = result
        self.record_convergence(new_time=total, criterions=torch.zeros(1))
        self.compute_acc(y_q)
