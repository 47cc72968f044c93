"""Few-shot LAPLACIAN_SHOT on probability features, drop-in for the reference's src/methods/few_shot/laplacian_shot.py
(SURVEY.md F4).  Same constructor / run_task / logs contract (`acc` is (n_task, iter): the accuracy after every bound
update, the evaluator reads the last column; `ent_energy` (n_task, iter); `criterions` one [0] per task); normalisation,
prototypes, unary term, kNN graph and the bound updates run in libtclip.so (tclip_laplacian_shot_run), one workgroup per
task instead of the reference's numpy / scipy.sparse / sklearn host loop.  Pinned to reference-made fixtures within a
tolerance (tests/test_laplacian_shot.py).  The reference class itself does not run on numpy >= 1.24
(`dtype=np.float`, laplacian_shot.py:100).  run_tables, which the task-batch loop takes with `in_place_support: True`, reads
the task rows from the feature tables in place (tclip_laplacian_shot_run_tasks): the same bits without the (T,S,K) and
(T,Q,K) tensors."""
import numpy as np

from src.methods._em_dirichlet_base import FewShotMixin, MethodBase
from tclip_amd import engine
from tclip_amd.reporting import VAL_PARAM


class LAPLACIAN_SHOT(FewShotMixin, MethodBase):
    LOGGER_NAME = __name__
    IN_PLACE_SUPPORT = ("softmax",)          # run_method refuses visual features, and so does run_tables
    SWEEP_ATTR = VAL_PARAM["LAPLACIAN_SHOT"]

    def __init__(self, model, device, log_file, args):
        super().__init__(model=model, device=device, log_file=log_file, args=args)
        self.knn = args.knn
        self.norm_type = args.norm_type
        self.iter = args.iter
        self.number_tasks = args.batch_size
        self.shots = args.shots
        self.lmd = args.lmd
        self.temp = args.temp
        self.ent_energy = []

    def get_logs(self):
        self.test_acc = np.asarray(self.test_acc, dtype=np.float32)
        self.ent_energy = np.asarray(self.ent_energy)
        self.timestamps = np.array(self.timestamps).mean()
        return {'timestamps': np.array(self.timestamps).mean(), 'acc': self.test_acc, 'ent_energy': self.ent_energy,
                'criterions': self.criterions}

    def run_task(self, task_dic, shot):
        return super().run_task(task_dic, shot)

    def run_method(self, support, query, y_s, y_q, n_batches=1):
        if query.shape[2] != self.args.num_classes_test:
            raise NotImplementedError("LAPLACIAN_SHOT here takes probability features (use_softmax_feature: True, feature dimension = n_class)")
        self._run(lambda: engine.run_laplacian_shot(query, support, y_s, iters=self.iter, knn=self.knn, lmd=self.lmd,
                                                    norm_type=self.norm_type), query.shape[0], y_q)

    def run_tables(self, table_s, s_idx, table_q, q_idx, cols, y_s, y_q, n_batches=1):
        """run_method for the task-batch loop (Evaluator_few_shot.evaluate_tasks with in_place_support): the support / query
        rows of task t are table_s[s_idx[t]] / table_q[q_idx[t]] with the columns permuted by cols[t]; neither (T,S,K) nor
        (T,Q,K) is built.  Overrides FewShotMixin.run_tables, which drives the EM-Dirichlet engine."""
        if table_q.shape[1] != self.args.num_classes_test:
            raise NotImplementedError("LAPLACIAN_SHOT here takes probability features (use_softmax_feature: True, feature dimension = n_class)")
        self._run(lambda: engine.run_laplacian_shot_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=self.iter, knn=self.knn,
                                                          lmd=self.lmd, norm_type=self.norm_type), q_idx.shape[0], y_q)

    def _sweep(self, values, table_s, s_idx, table_q, q_idx, cols, y_s, n_batches):
        """run_tables' engine call for a list of lmd values (FewShotMixin.run_tables_sweep); visual features are refused as
        run_tables refuses them"""
        if table_q.shape[1] != self.args.num_classes_test:
            raise NotImplementedError("LAPLACIAN_SHOT here takes probability features (use_softmax_feature: True, feature dimension = n_class)")
        return engine.sweep_laplacian_shot_tasks(table_q, q_idx, table_s, s_idx, y_s, cols, iters=self.iter, knn=self.knn,
                                                 values=values, norm_type=self.norm_type)

    @staticmethod
    def _sweep_slice(outs, i):
        # the unary term and the neighbour lists do not depend on lmd: one copy serves every value
        return outs[0], outs[1], outs[2][i], outs[3][i]

    def _banner(self):
        return " ==> Executing LAPLACIAN SHOT with lmd = {}".format(self.lmd)

    def _run(self, call, n_task, y_q):
        """the engine call, then the reference's bookkeeping"""
        self._finish(*self._execute(self._banner(), call), n_task, y_q)

    def _finish(self, result, total, n_task, y_q, n_batches=1):
        self.unary, self.neighbours, self.preds_iter, energies = result
        self.preds = self.preds_iter[:, -1, :]
        # accuracy after every update, on the host: means of 75 zeros and ones rounded as the reference's CPU op rounds them
        hit = (self.preds_iter.long().cpu() == y_q.cpu().unsqueeze(1)).float()          # (n_task, iter, Q)
        self.test_acc = list(hit.mean(2).numpy())
        self.ent_energy = list(energies.cpu().numpy())
        # the reference appends the cumulative wall time after every task (laplacian_shot.py:243-245)
        self.timestamps += self.spread_time("per_task", total, self.iter, n_task)
        self.criterions += [[0] for _ in range(n_task)]
