"""Shared host logic of the reference-named method classes.

MethodBase holds what every class repeats around its engine call: constructor state and logger, the device check, the timed
call, the rules that spread one wall time over the reference's per-iteration records, the accuracy helpers and get_logs.
EMDirichletBase adds the EM-Dirichlet loop; ZeroShotMixin / FewShotMixin add run_task.  Together they mirror the
reference's BASE/EM_DIRICHLET interface (constructor keywords, run_task, the logs dict, the post-call attributes
u / v / alpha) while the loop itself runs in libtclip.so on the GPU (tclip_amd.engine).  Reference:
src/methods/zero_shot/em_dirichlet.py:9-246, src/methods/few_shot/em_dirichlet.py:9-220 and their hard_ twins."""
import time

import numpy as np
import torch

from src.utils import Logger
from tclip_amd import engine

_SIMPLEX_ERROR = "The selected method is unable to handle query features that are not in the unit simplex"


class MethodBase(object):
    LOGGER_NAME = __name__      # a class outside the EM-Dirichlet family logs under its own module's name, as the reference's does
    ARG_DEFAULTS = {}           # written into args where the method's YAML has no such key

    def __init__(self, model, device, log_file, args):
        for key, value in self.ARG_DEFAULTS.items():
            if not hasattr(args, key):
                setattr(args, key, value)
        self.device = device
        self.model = model
        self.log_file = log_file
        self.logger = Logger(self.LOGGER_NAME, self.log_file)
        self.init_info_lists()
        self.args = args

    def __del__(self):
        try:
            self.logger.del_logger()
        except Exception:
            pass

    def init_info_lists(self):
        self.timestamps = []
        self.criterions = []
        self.test_acc = []

    def record_convergence(self, new_time, criterions):
        self.criterions.append(criterions)
        self.timestamps.append(new_time)

    def get_logs(self):
        self.criterions = np.asarray(self.criterions, dtype=np.float32)
        on_device = any(a.is_cuda for a in self.test_acc)
        self.test_acc = torch.cat(self.test_acc, dim=1).cpu()
        if on_device:            # args.device_matching: a task the host matching raises for has a NaN accuracy there
            engine.match_status_ok(self.test_acc)
        self.test_acc = self.test_acc.numpy()
        return {'timestamps': np.array(self.timestamps).mean(), 'criterions': self.criterions,
                'acc': self.test_acc}

    # -- the engine call --------------------------------------------------------------------
    def _cuda_device(self, name=None):
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("{} on MI355X needs device='cuda': there is no CPU fallback in this package".format(
                name or type(self).__name__))
        return dev

    def _timed(self, call):
        """call() between two device synchronisations: its result and the wall time of the interval"""
        dev = torch.device(self.device)
        torch.cuda.synchronize(dev)
        t0 = time.time()
        out = call()
        torch.cuda.synchronize(dev)
        return out, time.time() - t0

    def _execute(self, banner, call, name=None):
        """device check, banner log line, timed engine call"""
        self._cuda_device(name)
        self.logger.info(banner)
        return self._timed(call)

    @staticmethod
    def spread_time(rule, total, iters, n_task):
        """The reference appends one host-clock reading per outer iteration (or task); the fused loops have no such clock,
        so the total of one call is spread by the rule of the reference file the class mirrors:
          cumulative  the clock keeps running, every reading divided by n_task (em_dirichlet.py:242-244, paddle.py:214-216,
                      tim.py:184-186 and :317-319); reproduces the reference's "mean of cumulative times" statistic
          share       the clock restarts every iteration (soft_kmeans.py:203-216, em_gaussian.py:204-224)
          twice       every iteration is recorded twice, once undivided (hard_kmeans.py:198-204, kl_kmeans.py:178-187)
          per_task    one cumulative reading after every task (laplacian_shot.py:243-245)"""
        per_iter = total / max(iters, 1)
        if rule == "cumulative":
            return [total * (i + 1) / max(iters, 1) / n_task for i in range(iters)]
        if rule == "share":
            return [per_iter / n_task] * iters
        if rule == "twice":
            return [per_iter, per_iter / n_task] * iters
        if rule == "per_task":
            return [total * (t + 1) / n_task for t in range(n_task)]
        raise ValueError(f"unknown timestamp rule {rule!r}")

    def _text_features(self, dev):
        # imported here: a Level-1 overlay that copies only the modules of the probability-feature path keeps working
        from src.methods._visual import text_features
        return text_features(self.model, self.args, dev)

    # -- accuracy ---------------------------------------------------------------------------
    def compute_acc(self, y_q, preds_q=None):
        # on the host: the mean of 75 zeros and ones is rounded as the reference's CPU op rounds it
        preds_q = (self.preds if preds_q is None else preds_q).long().cpu()
        accuracy = (preds_q == y_q.cpu()).float().mean(1, keepdim=True)
        self.test_acc.append(accuracy)

    def _matching(self):
        """args.device_matching (main_features.py --opts device_matching True): the cluster-to-class matching runs on the
        device too; accuracies and matched predictions stay there until get_logs.  The option is optional, and args may be
        a namespace (a missing attribute is an AttributeError) or a dict with attribute access (a KeyError)."""
        try:
            on = getattr(self.args, "device_matching", False)
        except KeyError:
            on = False
        return "device" if on else "host"

    def compute_acc_clustering(self, query, y_q, text=None):
        """`text` given: the accuracy tail on visual features (soft_kmeans.py:36-66): D-dim prototypes, scored against the
        text features"""
        kw = dict(graph_matching=bool(self.args.graph_matching), matching=self._matching())
        if text is None:
            acc, new_preds = engine.clustering_accuracy(query, self.preds, y_q, **kw)
        else:
            acc, new_preds = engine.clustering_accuracy_visual(query, self.preds, y_q, text, self.args.T, **kw)
        self.matched_preds = new_preds
        self.test_acc.append(acc.view(-1, 1))


class EMDirichletBase(MethodBase):
    HARD = False
    FEW_SHOT = False
    BANNER = "EM-DIRICHLET"

    def __init__(self, model, device, log_file, args):
        super().__init__(model=model, device=device, log_file=log_file, args=args)
        self.iter = args.iter
        # `lambd` from the YAML is ignored by the reference too (em_dirichlet.py:14)
        if self.FEW_SHOT:
            self.lambd = int(args.num_classes_test / args.k_eff) * args.n_query
        else:
            self.lambd = int(args.num_classes_test / 5) * args.n_query
        self.eps = 1e-15
        self.iter_mm = args.iter_mm
        self.mm_iters = None

    def _stop_patience(self):
        """args.stop_patience (main_features.py --opts stop_patience 2): a batch stops once its predictions have stood still
        for that many outer iterations in a row (tclip_amd.until_stable).  Optional like device_matching: None when absent."""
        try:
            return getattr(self.args, "stop_patience", None)
        except KeyError:
            return None

    def _record_objective(self):
        """args.record_objective (main_features.py --opts record_objective True): the penalised objective of every task after
        every outer iteration (tclip_amd.objective).  Optional like stop_patience: off when absent."""
        try:
            return bool(getattr(self.args, "record_objective", None))
        except KeyError:
            return False

    def get_logs(self):
        logs = super().get_logs()
        if self._record_objective():
            logs['objectives'] = self.objectives
        return logs

    # -- the loop ---------------------------------------------------------------------------
    def _run_engine(self, query, support=None, y_s=None, n_batches=1, tables=None):
        """`tables` = dict(table_q, q_idx[, table_s, s_idx, cols]): the task rows are read from the feature tables through the
        task-batch loop's index tensors (engine.run_em_dirichlet_tasks) and `query` / `support` are not used"""
        if not self.args.use_softmax_feature:
            raise ValueError(_SIMPLEX_ERROR)
        n_task = tables["q_idx"].shape[0] if tables is not None else query.shape[0]
        kw = dict(n_batches=n_batches, iters=self.iter, iter_mm=self.iter_mm, lambd=self.lambd, hard=self.HARD)
        runner = engine
        patience = self._stop_patience()
        record = self._record_objective()
        if patience is not None:
            from tclip_amd import until_stable as runner
            kw["patience"] = runner.check_patience(patience)
        if record:                     # the same run, observed: with the patience when there is one
            from tclip_amd import objective as runner
        if tables is not None:
            call = lambda: runner.run_em_dirichlet_tasks(tables["table_q"], tables["q_idx"], tables.get("table_s"),      # noqa: E731
                                                         tables.get("s_idx"), y_s, tables.get("cols"), **kw)
        else:
            call = lambda: runner.run_em_dirichlet(query, support, y_s, **kw)      # noqa: E731
        res, total = self._execute(" ==> Executing {} with LAMBDA = {} and T = {}".format(self.BANNER, self.lambd, self.args.T),
                                   call, name="EM-Dirichlet")
        self.u, self.v, self.alpha, self.preds = res.u, res.v, res.alpha, res.preds
        self.mm_iters = res.mm_iters.cpu().numpy()
        crit = res.criterions.cpu().numpy()            # (n_batches, iters)
        self.timestamps += self.spread_time("cumulative", total, self.iter, n_task)
        self.criterions = list(crit.mean(0)) if n_batches > 1 else list(crit[0])
        self.criterions_per_batch = crit
        if patience is not None:       # the logs keep their shapes: a stopped batch's records are 0 from its outer_iters on
            self.outer_iters = res.outer_iters.cpu().numpy()                    # (n_batches,)
            self.assignment_changes = res.changes.cpu().numpy()                 # (n_batches, iter)
        if record:                     # float64; with a patience a stopped batch's rows are 0 from its outer_iters on
            self.objective_terms = res.objective_terms.cpu().numpy()            # (n_task, iter, 4)
            self.objectives = runner.objective(self.objective_terms, self.lambd)        # (n_task, iter)
        return res

    # -- scoring with the fitted model ------------------------------------------------------
    def _score_kw(self, hard):
        """what the scoring calls take from the last run: its alpha and v, the class's lambd, args.n_query, HARD"""
        if not self.args.use_softmax_feature:
            raise ValueError(_SIMPLEX_ERROR)
        if getattr(self, "alpha", None) is None or getattr(self, "v", None) is None:
            raise RuntimeError("{} has no fitted model to score with: run_task (or run_method) goes first".format(type(self).__name__))
        self._cuda_device("EM-Dirichlet")
        return dict(lambd=self.lambd, n_query=self.args.n_query, hard=self.HARD if hard is None else bool(hard))

    def score_rows(self, x, hard=None):
        """One E-step of the model the last run left (self.alpha, self.v) on rows that need not have been its queries:
        x (T,R,K) probability features, T the tasks of that run, any R -> tclip_amd.score.ScoreResult(u (T,R,K), preds (T,R)
        i32, logits None), cuda.  hard=None takes the class's HARD.  score_rows(x_q) of the run's own queries returns its
        self.u and self.preds bit for bit.  In zero-shot the result indexes CLUSTERS: mapping clusters to classes stays with
        the accuracy tail (compute_acc_clustering) and is not applied here.  Keeps nothing and logs nothing."""
        kw = self._score_kw(hard)
        from tclip_amd import score
        return score.score_em_dirichlet(x.to(self.device), self.alpha, self.v, **kw)

    def score_table_rows(self, table, idx, cols=None, hard=None):
        """score_rows with the rows read in place from a feature table: table (rows,K), idx (T,R) rows of it, cols (T,K) the
        per-task column permutation or None (tclip_amd.score.score_em_dirichlet_tasks); the bits of score_rows on the
        gathered rows.  Clusters, not classes, in zero-shot - as score_rows."""
        kw = self._score_kw(hard)
        from tclip_amd import score
        return score.score_em_dirichlet_tasks(table.to(self.device), idx, self.alpha, self.v, cols, **kw)


class ZeroShotMixin:
    def run_task(self, task_dic):
        y_q = task_dic['y_q']
        query = task_dic['x_q']
        query = query.to(self.device).float()
        y_q = y_q.long().squeeze(2).to(self.device)
        del task_dic
        self.run_method(query=query, y_q=y_q)
        return self.get_logs()

    def run_method(self, query, y_q, n_batches=1):
        self._run_engine(query, n_batches=n_batches)
        self.compute_acc_clustering(query, y_q)

    def _run_clustering(self, query, run, run_visual):
        """The head SOFT_KMEANS, HARD_KMEANS and EM_GAUSSIAN share: run() on probability features; on visual features
        (use_softmax_feature: False) run_visual(u0) with the initial assignment u0 from the text features.  Returns the
        engine's result, the wall time and the text features (None on probability features) for compute_acc_clustering."""
        dev = self._cuda_device()
        text = None if self.args.use_softmax_feature else self._text_features(dev)
        self.logger.info(" ==> Executing {} with T = {}".format(self.BANNER, self.args.T))
        if text is None:
            out, total = self._timed(run)
        else:
            out, total = self._timed(lambda: run_visual(engine.visual_init(query, text, self.args.T)))
        return out, total, text


class FewShotMixin:
    IN_PLACE_FEATURES = ()      # of "softmax" / "visual": the feature kinds on which run_tables reads the task rows in place

    @classmethod
    def reads_rows_in_place(cls, use_softmax_feature):
        return ("softmax" if use_softmax_feature else "visual") in cls.IN_PLACE_FEATURES

    # the feature kinds on which run_tables reads the task rows in place only when the evaluator is asked to
    # (args.in_place_support): these classes keep the builder route by default
    IN_PLACE_SUPPORT = ()

    @classmethod
    def can_read_rows_in_place(cls, use_softmax_feature):
        return ("softmax" if use_softmax_feature else "visual") in cls.IN_PLACE_SUPPORT

    # the feature kinds on which run_tables reads the task rows in place in EVERY step of the method's loop (TIM-GD, ALPHA_TIM:
    # both GEMMs of an Adam step), taken only when the evaluator is asked to (args.in_place_loop): a switch of its own,
    # because these classes pay the indirection per step, not once
    IN_PLACE_LOOP = ()

    @classmethod
    def can_read_rows_in_place_per_step(cls, use_softmax_feature):
        return ("softmax" if use_softmax_feature else "visual") in cls.IN_PLACE_LOOP

    @classmethod
    def rows_in_place(cls, args):
        """Whether the task-batch loop (Evaluator_few_shot.evaluate_tasks) hands this class the feature tables and the index
        tensors (run_tables) instead of task tensors (run_batch).  The whole route of a group of batches:

          materialise_tasks                              gather_rows + relabel_batch -> run_batch    (the reference's route)
          softmax features, a support set misses a class gather_rows + relabel_batch -> run_batch    (relabel_indices: None)
          otherwise, rows_in_place(args)                 run_tables                                  (no task tensor is built)
          otherwise                                      gather_task_rows, the fused builder -> run_batch

        and rows_in_place, by class and feature kind (visual: use_softmax_feature False):

          EM_DIRICHLET, HARD_EM_DIRICHLET   softmax            always    (IN_PLACE_FEATURES; visual features are refused)
          PADDLE                            softmax, visual    always    (IN_PLACE_FEATURES)
          BDCSPN                            softmax, visual    with in_place_support    (IN_PLACE_SUPPORT)
          LAPLACIAN_SHOT                    softmax            with in_place_support    (IN_PLACE_SUPPORT; visual: refused)
          TIM_GD                            softmax, visual    with in_place_loop       (IN_PLACE_LOOP: the rows are read per step)
          ALPHA_TIM                         softmax            with in_place_loop       (IN_PLACE_LOOP; visual: refused)

        A switch that does not belong to the class changes nothing.  evaluate_sweep always reads the rows in place."""
        soft = args.use_softmax_feature
        return (cls.reads_rows_in_place(soft)
                or bool(getattr(args, "in_place_support", False)) and cls.can_read_rows_in_place(soft)
                or bool(getattr(args, "in_place_loop", False)) and cls.can_read_rows_in_place_per_step(soft))

    # ---- a sweep of the class's validation-tuned parameter over the same tasks (Evaluator_few_shot.evaluate_sweep) ----------
    # The four tunable classes take the attribute's name from reporting.VAL_PARAM (SWEEP_ATTR) and split their `_run` into
    # `_banner` and `_finish`, so that
    # the reference's bookkeeping of one run can follow an engine call that served several objects.
    SWEEP_ATTR = None

    @classmethod
    def run_tables_sweep(cls, methods, table_s, s_idx, table_q, q_idx, cols, y_s, y_q, n_batches=1):
        """run_tables for a list of objects of this class that differ in SWEEP_ATTR only (one per value, built from args as a
        run with that value builds it): ONE engine call (engine.sweep_*_tasks) solves the tasks for every object's value, then
        each object keeps its slice and does the bookkeeping of a run of its own - test_acc, criterions, and timestamps from an
        equal share of the call's wall time.  The task rows are always read from the tables in place."""
        if cls.SWEEP_ATTR is None:
            raise NotImplementedError("{} has no validation-tuned parameter to sweep".format(cls.__name__))
        first = methods[0]
        first._cuda_device()
        values = [getattr(m, cls.SWEEP_ATTR) for m in methods]
        for m in methods:
            m.logger.info(m._banner())
        outs, total = first._timed(lambda: first._sweep(values, table_s, s_idx, table_q, q_idx, cols, y_s, n_batches))
        for i, m in enumerate(methods):
            m._finish(first._sweep_slice(outs, i), total / len(methods), q_idx.shape[0], y_q, n_batches)

    @staticmethod
    def _sweep_slice(outs, i):
        """what the single-value engine call returns for value i, out of the sweep's value-major outputs"""
        return tuple(o[i] for o in outs)

    def run_task(self, task_dic, shot=10):
        y_s, y_q = task_dic['y_s'], task_dic['y_q']
        support, query = task_dic['x_s'], task_dic['x_q']
        support = support.to(self.device).float()
        query = query.to(self.device).float()
        y_s = y_s.long().squeeze(2).to(self.device)
        y_q = y_q.long().squeeze(2).to(self.device)
        del task_dic
        self.run_batch(support=support, query=query, y_s=y_s, y_q=y_q)
        return self.get_logs()

    def run_batch(self, support, query, y_s, y_q, n_batches=1):
        """what run_task runs on the tensors of its tasks: run_method, unless a class prepares its inputs first (BDCSPN)"""
        self.run_method(support=support, query=query, y_s=y_s, y_q=y_q, n_batches=n_batches)

    def run_method(self, support, query, y_s, y_q, n_batches=1):
        # unlike the reference (few_shot/em_dirichlet.py:186-190) the inputs are left untouched:
        # the engine keeps its own log-features
        self._run_engine(query, support, y_s, n_batches=n_batches)
        self.compute_acc(y_q=y_q)

    def run_tables(self, table_s, s_idx, table_q, q_idx, cols, y_s, y_q, n_batches=1):
        """run_method for the task-batch loop (Evaluator_few_shot.evaluate_tasks): the support / query rows of task t are
        table_s[s_idx[t]] / table_q[q_idx[t]] with the columns permuted by cols[t] (Tasks_Generator_few_shot.get_task's
        `data[:, unique_labels]`), y_s / y_q the re-indexed labels.  The (T,S,K) support tensor - 16 MB per task at
        K = 1000 with 4 shots - is never built."""
        self._run_engine(None, None, y_s, n_batches=n_batches,
                         tables=dict(table_q=table_q, q_idx=q_idx, table_s=table_s, s_idx=s_idx, cols=cols))
        self.compute_acc(y_q=y_q)
