"""Task-batch loop of the few-shot evaluation (reference: src/eval_few_shot.py:213-270) on the
batched engine; see src/eval_zero_shot.py for the structure.  Per batch the reference draws all
query index sets first, then all support index sets (eval_few_shot.py:233-241); the same order is
kept so that a seeded run sees the reference's tasks."""
import types

import numpy as np
import torch

from src._evaluator import EvaluatorBase, _as_tensor, arg_hidden, arg_set_to, check_record_objective, check_stop_patience
from src.methods.few_shot.em_dirichlet import EM_DIRICHLET
from src.methods.few_shot.hard_em_dirichlet import HARD_EM_DIRICHLET
from src.methods.few_shot.paddle import PADDLE
from src.methods.few_shot.bdcspn import BDCSPN
from src.methods.few_shot.tim import ALPHA_TIM, TIM_GD
from src.methods.few_shot.laplacian_shot import LAPLACIAN_SHOT
from src.sampler_few_shot import CategoriesSampler_few_shot, SamplerQuery_few_shot, SamplerSupport_few_shot
from src.task_generator_few_shot import label_permutation, relabel
from src.utils import compute_confidence_interval
from tclip_amd import engine, reporting, sharding


def relabel_batch(x_s, x_q, y_s, y_q, use_softmax_feature):
    xs2, xq2, ys2, yq2 = [], [], [], []
    for t in range(x_s.shape[0]):
        a_, b_, c_, d_ = relabel(x_s[t], x_q[t], y_s[t], y_q[t], use_softmax_feature)
        xs2.append(a_)
        xq2.append(b_)
        ys2.append(c_)
        yq2.append(d_)
    return torch.stack(xs2, 0), torch.stack(xq2, 0), torch.stack(ys2, 0), torch.stack(yq2, 0)


def relabel_indices(y_s, y_q, n_class):
    """Tasks_Generator_few_shot.get_task (task_generator_few_shot.py:41-52) for a whole set of tasks WITHOUT touching the
    features: per task the column permutation `unique_labels` as an int32 row and the re-indexed support / query labels.
    None when some task's support set misses a class (the permuted task would have fewer than n_class columns; the caller
    materialises the tensors then, as the reference does)."""
    y_s, y_q = y_s.long(), y_q.long()
    if y_s.numel() and int(y_s.min()) >= 0 and int(y_s.max()) < n_class:
        present = torch.zeros(y_s.shape[0], n_class, dtype=torch.bool).scatter_(1, y_s, True)
        if bool(present.all()):
            # every class in every support set (what the reference's sampler draws): unique_labels = flip(arange(K)) for
            # every task, i.e. column d <- table column K-1-d and label y <- K-1-y, without a torch.unique per task
            cols = torch.arange(n_class - 1, -1, -1, dtype=torch.int32).repeat(y_s.shape[0], 1)
            return cols, n_class - 1 - y_s, n_class - 1 - y_q
    cols, ys2, yq2 = [], [], []
    for t in range(y_s.shape[0]):
        uniq, lut = label_permutation(y_s[t])
        if len(uniq) != n_class:
            return None
        cols.append(uniq.to(torch.int32))
        ys2.append(lut[y_s[t].long()])
        yq2.append(lut[y_q[t].long()])
    return torch.stack(cols, 0), torch.stack(ys2, 0), torch.stack(yq2, 0)


def checked_sweep_values(args, values, distributed=None):
    """What a parameter sweep (Evaluator_few_shot.evaluate_sweep, main_features.py `--opts sweep_values "[...]"`) refuses, checked
    before any device work: a split other than `val` (the sweep file is the validation file), a method without a
    validation-tuned parameter, an empty list or an element that is not a finite number, and a job under torch.distributed
    (`distributed`: None asks torch).  Returns the values as a list, every element with the type it was written with."""
    if getattr(args, 'used_test_set', 'test') != 'val':
        raise ValueError("sweep_values tunes a parameter on the validation split: used_test_set must be 'val', not {!r}".format(
            getattr(args, 'used_test_set', 'test')))
    if getattr(args, 'name_method', None) not in reporting.VAL_PARAM:
        raise ValueError("method {} has no validation-tuned parameter to sweep (the tunable methods: {})".format(
            getattr(args, 'name_method', None), ', '.join(sorted(reporting.VAL_PARAM))))
    if not isinstance(values, (list, tuple)) or len(values) == 0:
        raise ValueError("sweep_values must be a non-empty list of numbers, e.g. \"[1.0, 2.0, 5.0]\"")
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float('inf'), float('-inf')):
            raise ValueError("sweep_values must be a list of finite numbers: {!r} is not one".format(v))
    if distributed is None:
        distributed = torch.distributed.is_available() and torch.distributed.is_initialized()
    if distributed:
        raise RuntimeError("parameter sweeps are single-process: run sweep_values without torch.distributed "
                           "(one process already solves every value on the same tasks)")
    return list(values)


_METHODS = {'EM_DIRICHLET': EM_DIRICHLET, 'HARD_EM_DIRICHLET': HARD_EM_DIRICHLET, 'PADDLE': PADDLE, 'BDCSPN': BDCSPN,
            'ALPHA_TIM': ALPHA_TIM, 'LAPLACIAN_SHOT': LAPLACIAN_SHOT,
            'TIM-GD': TIM_GD, 'TIM_GD': TIM_GD}      # tim.yaml's name_method is 'TIM-GD'


class Evaluator_few_shot(EvaluatorBase):
    _METHODS = _METHODS
    # the validation-tuned parameter of a method (reference: eval_few_shot.py:130-187).  TIM-GD has no branch in the reference's
    # set_value_opt_param: nothing of it is tuned
    _TUNED = reporting.VAL_PARAM

    def run_full_evaluation(self, model, preprocess):
        """eval_few_shot.py:42-74 from saved feature files (see Evaluator_zero_shot.run_full_evaluation): the
        support table is the train split, the query table the `used_test_set` split."""
        if getattr(self.args, 'sweep_values', None) is not None:
            return self.run_full_sweep(model)
        mean_accuracies, mean_times = self.evaluate_tasks(model, *self._saved_tables(model))
        if mean_accuracies is not None:
            self.report_results(mean_accuracies, mean_times)
        return mean_accuracies, mean_times

    def run_full_sweep(self, model, tables=None):
        """run_full_evaluation with `sweep_values`: what the reference's scripts/opt_parameters.sh does with one process per
        value.  One evaluate_sweep, then one `val_param<TAB>acc` row per value through report_results, in the order given -
        the file separate runs with the same seed write, byte for byte.  `tables`: (features_s, labels_s, features_q, labels_q)
        already loaded (main_features.py), None loads them from the reference's layout."""
        a = self.args
        values = checked_sweep_values(a, a.sweep_values)
        if tables is None:
            tables = self._saved_tables(model)
        accs, mean_time = self.evaluate_sweep(model, *tables, values=values)
        for v, acc in zip(values, accs):
            with arg_set_to(a, self._TUNED[a.name_method], v):
                self.report_results(acc, mean_time)
        return accs, mean_time

    def extract_and_load_features(self, model, dataset, data_loaders):
        """eval_few_shot.py:91-128, loading only: the train split, then the `used_test_set` split (EvaluatorBase.load_split)."""
        return self.load_split('train'), self.load_split(self.args.used_test_set)

    def _saved_tables(self, model):
        dic_s, dic_q = self.extract_and_load_features(model, None, None)
        return (dic_s['concat_features'].to('cpu'), dic_s['concat_labels'].long().to('cpu'),
                dic_q['concat_features'].to('cpu'), dic_q['concat_labels'].long().to('cpu'))

    def set_value_opt_param(self, opt_param):
        if self.args.name_method in self._TUNED:
            self.args[self._TUNED[self.args.name_method]] = opt_param

    def set_method_opt_param(self):
        """Test runs of a tunable method use the parameter that did best on the validation split: the
        sweep file results_few_shot/val/<dataset>/<METHOD>_<softmax|visual>_s<shots>.txt (imagenet borrows
        caltech101's, eval_few_shot.py:161-166), rows `param<TAB>acc`, the LAST best row wins.  A missing or
        unreadable file is an error, as in the reference."""
        a = self.args
        name_file = reporting.validation_file(a, getattr(a, 'results_root', '.'), 'caltech101' if a.dataset == 'imagenet' else None)
        try:
            params, accs = [], []
            with open(name_file, 'r') as f:
                for i, line in enumerate(f):
                    if i < 2:
                        continue
                    cells = line.split('\t')
                    params.append(float(cells[0]))
                    accs.append(float(cells[1]))
            accs = np.array(accs)
            opt_param = params[int(np.argwhere(accs == np.amax(accs))[-1][0])]
        except Exception:
            raise ValueError("The optimal parameter was not found. Please make sure you have performed the "
                             "tuning of the parameter on the validation set.")
        self.logger.info('opt param {}'.format(opt_param))
        self.set_value_opt_param(opt_param)
        return opt_param

    def sample_indices(self, all_labels_support, all_labels_query):
        """(support, query) index tensors (n_batches, batch_size, n); per batch the reference draws all query index sets first,
        then all support index sets"""
        a = self.args
        q_idx, s_idx = self._draw_batches(lambda: CategoriesSampler_few_shot(a.batch_size, a.k_eff, a.n_class, a.shots, a.n_query,
                                                                             force_query_size=True),
                                          (all_labels_support, all_labels_query), (SamplerQuery_few_shot, SamplerSupport_few_shot))
        return s_idx, q_idx

    def _tasks(self, all_features_support, all_labels_support, all_features_query, all_labels_query, indices):
        """What evaluate_tasks and evaluate_sweep prepare alike: the labels on the host, the (support, query) index tensors -
        `indices`, or drawn here - and their shape, the feature width W and the class count K: one number on softmax features,
        the embedding length D and args.n_class on visual features (use_softmax_feature: False; the labels are not re-indexed
        there).  tables() puts the (support, query) feature tables on the device: called by whoever runs a method on them, so
        that a sweep which falls back to ordinary runs holds no copy of its own."""
        a, dev = self.args, torch.device(self.device)
        feats_s, feats_q = _as_tensor(all_features_support), _as_tensor(all_features_query)
        t = types.SimpleNamespace(tables=lambda: (feats_s.float().to(dev), feats_q.float().to(dev)),
                                  lab_s=_as_tensor(all_labels_support).long().cpu(), lab_q=_as_tensor(all_labels_query).long().cpu())
        t.s_idx, t.q_idx = self.sample_indices(t.lab_s.numpy(), t.lab_q.numpy()) if indices is None else indices
        t.n_batches, t.N, t.S = t.s_idx.shape
        t.Q = t.q_idx.shape[2]
        t.W = feats_q.shape[1]
        t.K = t.W if a.use_softmax_feature else int(a.n_class)
        return t

    def _block(self, t, ids=slice(None), relabelled=True):
        """The tasks of the batches `ids` of `t`: (si (T,S), qi (T,Q), y_s, y_q, rel).  rel = (cols, y_s, y_q): the label
        re-indexing / column permutation of Tasks_Generator_few_shot.get_task WITHOUT touching the features - softmax features
        only (visual features keep labels and columns: cols None); rel is None when a support set misses a class, or when not
        `relabelled`: the tensors are then materialised and relabelled as the reference does."""
        si, qi = t.s_idx[ids].reshape(-1, t.S), t.q_idx[ids].reshape(-1, t.Q)
        y_s, y_q = t.lab_s[si.reshape(-1)].view(-1, t.S), t.lab_q[qi.reshape(-1)].view(-1, t.Q)
        rel = None
        if relabelled:
            rel = relabel_indices(y_s, y_q, t.K) if self.args.use_softmax_feature else (None, y_s, y_q)
        return si, qi, y_s, y_q, rel

    def evaluate_sweep(self, model, all_features_support, all_labels_support, all_features_query, all_labels_query, values,
                       indices=None):
        """evaluate_tasks for every value of the method's validation-tuned parameter (`_TUNED`) on the SAME tasks, in one
        engine call per method (engine.sweep_*_tasks through the class's run_tables_sweep): the indices are drawn once, with
        the stream evaluate_tasks draws them with, and relabelled once.  Returns (mean accuracies [len(values)], mean time);
        entry p is what evaluate_tasks returns with the parameter set to values[p].  The task rows are always read from the
        tables in place (in_place_support, in_place_loop, materialise_tasks and batches_per_call do not apply; the results
        are the same bits either way).  When a support set misses a class the tasks cannot be addressed in place
        (relabel_indices) and the values run one after the other as ordinary evaluate_tasks calls on the same indices."""
        a = self.args
        values = checked_sweep_values(a, values)
        attr = self._TUNED[a.name_method]
        self.logger.info("=> Runnning a sweep of {} over {} with method {} on {} dataset".format(
            attr, values, a.name_method, a.used_test_set))
        t = self._tasks(all_features_support, all_labels_support, all_features_query, all_labels_query, indices)
        si, qi, _, _, rel = self._block(t)
        accs, times, methods = [], [], []
        for v in values:
            # a sweep ignores the stop and the objective record: no swept method has either
            with arg_set_to(a, attr, v), arg_hidden(a, 'stop_patience'), arg_hidden(a, 'record_objective'):
                if rel is None:
                    acc, time = self.evaluate_tasks(model, all_features_support, all_labels_support, all_features_query,
                                                    all_labels_query, indices=(t.s_idx, t.q_idx))
                    accs.append(acc)
                    times.append(time)
                else:                              # one object per value, built as a run with that value builds it
                    methods.append(self.get_method_builder(model=model, device=self.device, args=a, log_file=self.log_file))
        if rel is not None:
            cols, y_s, y_q = rel
            dev = torch.device(self.device)
            tab_s, tab_q = t.tables()
            type(methods[0]).run_tables_sweep(methods, table_s=tab_s, s_idx=si, table_q=tab_q, q_idx=qi, cols=cols,
                                              y_s=y_s.to(dev), y_q=y_q.to(dev), n_batches=t.n_batches)
            for m in methods:
                logs = m.get_logs()
                acc = sharding.task_accuracies(logs, t.n_batches, t.N).numpy()
                accs.append(np.asarray([compute_confidence_interval(acc[b])[0] for b in range(t.n_batches)]).mean())
                times.append(float(logs['timestamps']))
            self.last_methods = methods
        return np.asarray(accs), float(np.mean(times))

    def evaluate_tasks(self, model, all_features_support, all_labels_support, all_features_query, all_labels_query,
                       indices=None):
        """`indices`: a (support, query) index pair drawn earlier with sample_indices(); None draws it here."""
        a = self.args
        check_stop_patience(a)
        check_record_objective(a)
        self.logger.info("=> Runnning evaluation with method {} on {} dataset".format(
            a.name_method, getattr(a, 'used_test_set', 'test')))
        t = self._tasks(all_features_support, all_labels_support, all_features_query, all_labels_query, indices)
        tab_s, tab_q = t.tables()
        dev = torch.device(self.device)
        mine = sharding.my_batches(t.n_batches)
        # The parameter tuned on the validation split, when the test split is evaluated.  The reference builds the
        # method of a batch FIRST and reads the sweep file afterwards (eval_few_shot.py:250-254), and every method
        # copies its parameter in __init__ (paddle.py:26, bdcspn.py:18, tim.py:198, laplacian_shot.py:32): its batch 0
        # therefore runs with the YAML default and only batches 1.. with the tuned value.  That is reproduced here, so
        # that result files agree with the reference's; `tuned_param_for_every_batch: True` applies it to batch 0 too.
        tuned = getattr(a, 'used_test_set', 'test') == 'test' and getattr(a, 'tunable', False) \
            and not getattr(a, 'skip_tuned_param', False)
        first_method = None
        if tuned:
            if 0 in mine and not getattr(a, 'tuned_param_for_every_batch', False):
                first_method = self.get_method_builder(model=model, device=self.device, args=a, log_file=self.log_file)
            self.set_method_opt_param()
        method = self.get_method_builder(model=model, device=self.device, args=a, log_file=self.log_file)
        runs = [(first_method, mine[:1]), (method, mine[1:])] if first_method is not None else [(method, mine)]
        # batches_per_call (absent or 0: all batches of a run in one engine call): consecutive groups of at most that many
        # batches, each with a method object of its own, as the reference builds one per batch - what bounds the (T,S,W)
        # tensors of the methods that cannot read their rows in place.  The first group keeps the run's object (batch 0 of a
        # tuned run was built before the sweep file was read); the others are built from args as they now stand.
        per_call = int(getattr(a, 'batches_per_call', 0) or 0)
        if per_call < 0:
            raise ValueError("batches_per_call must be a non-negative number of batches")
        groups = []
        for m, ids in runs:
            step = per_call if per_call > 0 else max(len(ids), 1)
            for g0 in range(0, len(ids), step):
                groups.append((m if g0 == 0 else None, ids[g0:g0 + step]))
        timestamps, parts = [], None
        ran = None                        # the last method object that actually executed on this rank
        for m, ids in groups:
            if m is None:
                m = self.get_method_builder(model=model, device=self.device, args=a, log_file=self.log_file)
            ran = m
            # the route (FewShotMixin.rows_in_place has the table).  materialise_tasks: no rel, the reference's route
            si, qi, y_s, y_q, rel = self._block(t, ids, relabelled=not getattr(a, 'materialise_tasks', False))
            in_place = rel is not None and m.rows_in_place(a)
            if rel is None:
                x_s = engine.gather_rows(tab_s, si.reshape(-1)).view(len(ids) * t.N, t.S, t.W)
                x_q = engine.gather_rows(tab_q, qi.reshape(-1)).view(len(ids) * t.N, t.Q, t.W)
                x_s, x_q, y_s, y_q = relabel_batch(x_s, x_q, y_s, y_q, a.use_softmax_feature)
            else:
                cols, y_s, y_q = rel
                if not in_place:      # the fused task builder: `table[idx][..., cols]` in one device pass
                    x_s, x_q = engine.gather_task_rows(tab_s, si, cols), engine.gather_task_rows(tab_q, qi, cols)
            labels = dict(y_s=y_s.to(dev), y_q=y_q.to(dev), n_batches=len(ids))
            if in_place:
                # the class reads the task rows from the tables through the index tensors (label flip and column permutation
                # inside the kernels): x_s (T,S,K) - 1.6 GB per 100 tasks at K = 1000, 4 shots - is never built
                m.run_tables(table_s=tab_s, s_idx=si, table_q=tab_q, q_idx=qi, cols=cols, **labels)
            else:
                # BDCSPN normalises the features in run_task, before run_method (few_shot/bdcspn.py:165-166): run_batch does both
                m.run_batch(support=x_s, query=x_q, **labels)
            logs = m.get_logs()
            parts = sharding.concat_parts(parts, sharding.method_parts(a, m, logs, len(ids), t.N, t.Q, dev))
            timestamps += [float(logs['timestamps'])] * len(ids)
        # a rank whose only batch is batch 0 of a tuned run executes `first_method` alone: `method` never ran there and
        # carries no records (mm_iters None); a rank without a batch keeps the freshly built object
        return self._gathered(parts, t.n_batches, t.N, t.Q, ran if ran is not None else method, timestamps)
