"""Task-batch loop of the few-shot evaluation (reference: src/eval_few_shot.py:213-270) on the
batched engine; see src/eval_zero_shot.py for the structure.  Per batch the reference draws all
query index sets first, then all support index sets (eval_few_shot.py:233-241); the same order is
kept so that a seeded run sees the reference's tasks."""
import os

import numpy as np
import torch

from src.methods.few_shot.em_dirichlet import EM_DIRICHLET
from src.methods.few_shot.hard_em_dirichlet import HARD_EM_DIRICHLET
from src.methods.few_shot.paddle import PADDLE
from src.methods.few_shot.bdcspn import BDCSPN
from src.methods.few_shot.tim import ALPHA_TIM, TIM_GD
from src.methods.few_shot.laplacian_shot import LAPLACIAN_SHOT
from src.sampler_few_shot import CategoriesSampler_few_shot, SamplerQuery_few_shot, SamplerSupport_few_shot
from src.task_generator_few_shot import label_permutation, relabel
from src.utils import Logger, compute_confidence_interval
from tclip_amd import engine, features, reporting, sharding

def _as_tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


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


class Evaluator_few_shot:
    def __init__(self, device, args, log_file):
        self.device = device
        self.args = args
        self.log_file = log_file
        self.logger = Logger(__name__, self.log_file)

    def run_full_evaluation(self, model, preprocess):
        """eval_few_shot.py:42-74 from saved feature files (see Evaluator_zero_shot.run_full_evaluation): the
        support table is the train split, the query table the `used_test_set` split."""
        if getattr(self.args, 'sweep_values', None) is not None:
            return self.run_full_sweep(model)
        dic_s, dic_q = self.extract_and_load_features(model, None, None)
        mean_accuracies, mean_times = self.evaluate_tasks(
            model, dic_s['concat_features'].to('cpu'), dic_s['concat_labels'].long().to('cpu'),
            dic_q['concat_features'].to('cpu'), dic_q['concat_labels'].long().to('cpu'))
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
            dic_s, dic_q = self.extract_and_load_features(model, None, None)
            tables = (dic_s['concat_features'].to('cpu'), dic_s['concat_labels'].long().to('cpu'),
                      dic_q['concat_features'].to('cpu'), dic_q['concat_labels'].long().to('cpu'))
        accs, mean_time = self.evaluate_sweep(model, *tables, values=values)
        attr = self._TUNED[a.name_method]
        saved = a[attr]
        try:
            for v, acc in zip(values, accs):
                a[attr] = v
                self.report_results(acc, mean_time)
        finally:
            a[attr] = saved
        return accs, mean_time

    def extract_and_load_features(self, model, dataset, data_loaders):
        """eval_few_shot.py:91-128, loading only."""
        root = getattr(self.args, 'results_root', '.')
        out = []
        for split in ('train', self.args.used_test_set):
            path = reporting.saved_feature_path(self.args, split, root)
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path} not found: this package runs the reference's evaluation from saved "
                                        "feature files; extract them with the reference (CLIP is out of scope here)")
            feats, labels = features.load_features(path)
            out.append({'concat_features': feats, 'concat_labels': labels})
        return out[0], out[1]

    def report_results(self, mean_accuracies, mean_times):
        """eval_few_shot.py:272-338 (validation sweep row, or the test-mode row)."""
        return reporting.report_results(self.args, mean_accuracies, mean_times, self.logger,
                                        root=getattr(self.args, 'results_root', '.'))

    def get_method_builder(self, model, device, args, log_file):
        try:
            cls = _METHODS[args.name_method]
        except KeyError:
            raise ValueError(f"method {args.name_method!r} is not part of the EM-Dirichlet engine")
        return cls(model=model, device=device, log_file=log_file, args=args)

    # ---- validation-tuned parameter (reference: eval_few_shot.py:130-187)
    # TIM-GD has no branch in the reference's set_value_opt_param: nothing of it is tuned
    _TUNED = {'LAPLACIAN_SHOT': 'lmd', 'ALPHA_TIM': 'alpha_value', 'PADDLE': 'lambd', 'BDCSPN': 'temp'}

    def set_value_opt_param(self, opt_param):
        if self.args.name_method in self._TUNED:
            self.args[self._TUNED[self.args.name_method]] = opt_param

    def set_method_opt_param(self):
        """Test runs of a tunable method use the parameter that did best on the validation split: the
        sweep file results_few_shot/val/<dataset>/<METHOD>_<softmax|visual>_s<shots>.txt (imagenet borrows
        caltech101's, eval_few_shot.py:161-166), rows `param<TAB>acc`, the LAST best row wins.  A missing or
        unreadable file is an error, as in the reference."""
        a = self.args
        word = '_softmax' if a.use_softmax_feature else '_visual'
        dataset = 'caltech101' if a.dataset == 'imagenet' else a.dataset
        name_file = os.path.join(getattr(a, 'results_root', '.'), 'results_few_shot', 'val', str(dataset),
                                 '{}_s{}.txt'.format(a.name_method + word, a.shots))
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
        a = self.args
        q_all, s_all, lists = [], [], None
        for _ in range(int(a.number_tasks / a.batch_size)):
            sampler = CategoriesSampler_few_shot(a.batch_size, a.k_eff, a.n_class, a.shots, a.n_query,
                                                 force_query_size=True)
            if lists is None:             # label -> index lists: no random numbers involved, built once (see eval_zero_shot.py)
                sampler.create_list_classes(all_labels_support, all_labels_query)
                lists = (sampler.m_ind_support, sampler.m_ind_query)
            else:
                sampler.m_ind_support, sampler.m_ind_query = lists
            q_all.append(torch.stack(list(SamplerQuery_few_shot(sampler)), 0))
            s_all.append(torch.stack(list(SamplerSupport_few_shot(sampler)), 0))
        return torch.stack(s_all, 0), torch.stack(q_all, 0)

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
        lab_s = _as_tensor(all_labels_support).long().cpu()
        lab_q = _as_tensor(all_labels_query).long().cpu()
        s_idx, q_idx = self.sample_indices(lab_s.numpy(), lab_q.numpy()) if indices is None else indices
        n_batches, N, S = s_idx.shape
        Q = q_idx.shape[2]
        si, qi = s_idx.reshape(-1, S), q_idx.reshape(-1, Q)
        y_s, y_q = lab_s[si.reshape(-1)].view(-1, S), lab_q[qi.reshape(-1)].view(-1, Q)
        W = _as_tensor(all_features_query).shape[1]
        K = W if a.use_softmax_feature else int(a.n_class)
        rel = relabel_indices(y_s, y_q, K) if a.use_softmax_feature else (None, y_s, y_q)
        saved = a[attr]
        try:
            if rel is None:
                accs, times = [], []
                for v in values:
                    a[attr] = v
                    acc, t = self.evaluate_tasks(model, all_features_support, all_labels_support, all_features_query,
                                                 all_labels_query, indices=(s_idx, q_idx))
                    accs.append(acc)
                    times.append(t)
                return np.asarray(accs), float(np.mean(times))
            methods = []
            for v in values:                       # one object per value, built as a run with that value builds it
                a[attr] = v
                methods.append(self.get_method_builder(model=model, device=self.device, args=a, log_file=self.log_file))
        finally:
            a[attr] = saved
        dev = torch.device(self.device)
        tab_s = _as_tensor(all_features_support).float().to(dev)
        tab_q = _as_tensor(all_features_query).float().to(dev)
        cols, y_s, y_q = rel
        type(methods[0]).run_tables_sweep(methods, table_s=tab_s, s_idx=si, table_q=tab_q, q_idx=qi, cols=cols, y_s=y_s.to(dev),
                                          y_q=y_q.to(dev), n_batches=n_batches)
        accs, times = [], []
        for m in methods:
            logs = m.get_logs()
            acc = torch.from_numpy(logs['acc'][:, -1].copy()).view(n_batches, N).float().numpy()      # as sharding.method_parts
            accs.append(np.asarray([compute_confidence_interval(acc[b])[0] for b in range(n_batches)]).mean())
            times.append(float(logs['timestamps']))
        self.last_methods = methods
        return np.asarray(accs), float(np.mean(times))

    def evaluate_tasks(self, model, all_features_support, all_labels_support, all_features_query, all_labels_query,
                       indices=None):
        """`indices`: a (support, query) index pair drawn earlier with sample_indices(); None draws it here."""
        a = self.args
        self.logger.info("=> Runnning evaluation with method {} on {} dataset".format(
            a.name_method, getattr(a, 'used_test_set', 'test')))
        dev = torch.device(self.device)
        tab_s = _as_tensor(all_features_support).float().to(dev)
        tab_q = _as_tensor(all_features_query).float().to(dev)
        lab_s = _as_tensor(all_labels_support).long().cpu()
        lab_q = _as_tensor(all_labels_query).long().cpu()
        s_idx, q_idx = self.sample_indices(lab_s.numpy(), lab_q.numpy()) if indices is None else indices
        n_batches, N, S = s_idx.shape
        Q = q_idx.shape[2]
        mine = sharding.my_batches(n_batches)
        # the feature width and the class count: one number on softmax features, the embedding length D and args.n_class on
        # visual features (use_softmax_feature: False; PADDLE, BDCSPN and TIM-GD run there, the labels are not re-indexed)
        W = tab_q.shape[1]
        K = W if a.use_softmax_feature else int(a.n_class)
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
        timestamps, parts = [], None
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
        materialise = bool(getattr(a, 'materialise_tasks', False))
        ran = None                        # the last method object that actually executed on this rank
        for m, ids in groups:
            if m is None:
                m = self.get_method_builder(model=model, device=self.device, args=a, log_file=self.log_file)
            ran = m
            si, qi = s_idx[ids].reshape(-1, S), q_idx[ids].reshape(-1, Q)
            y_s, y_q = lab_s[si.reshape(-1)].view(-1, S), lab_q[qi.reshape(-1)].view(-1, Q)
            # label re-indexing / column permutation of Tasks_Generator_few_shot.get_task WITHOUT touching the features: softmax
            # features only (visual features keep labels and columns); None when a support set misses a class, and the tensors
            # are then materialised as the reference does
            cols, rel = None, None
            if not materialise:
                rel = relabel_indices(y_s, y_q, K) if a.use_softmax_feature else (None, y_s, y_q)
            # The EM-Dirichlet classes and PADDLE read the task rows from the tables through the index tensors (label flip and
            # column permutation inside the kernels): x_s (T,S,K) - 1.6 GB per 100 tasks at K = 1000, 4 shots - is never built
            # in_place_support (absent or False: the route above and below as it always was): BDCSPN and LAPLACIAN_SHOT, whose
            # first kernels normalise the task rows into their workspace, read them from the tables too
            in_place = m.reads_rows_in_place(a.use_softmax_feature)
            if not in_place and getattr(a, 'in_place_support', False) and hasattr(m, 'can_read_rows_in_place'):
                in_place = m.can_read_rows_in_place(a.use_softmax_feature)
            # in_place_loop (absent or False: as above): TIM-GD and ALPHA_TIM, which read their task rows in both GEMMs of EVERY
            # Adam step, read them from the tables too - a switch of its own, since they pay the indirection per step
            if not in_place and getattr(a, 'in_place_loop', False) and hasattr(m, 'can_read_rows_in_place_per_step'):
                in_place = m.can_read_rows_in_place_per_step(a.use_softmax_feature)
            if rel is not None:
                cols, y_s, y_q = rel
            if rel is not None and in_place:
                m.run_tables(table_s=tab_s, s_idx=si, table_q=tab_q, q_idx=qi, cols=cols, y_s=y_s.to(dev), y_q=y_q.to(dev),
                             n_batches=len(ids))
            else:
                if rel is not None:
                    # the fused task builder: `table[idx][..., cols]` in one device pass, the re-indexed labels from the same call
                    x_s = engine.gather_task_rows(tab_s, si, cols)
                    x_q = engine.gather_task_rows(tab_q, qi, cols)
                else:
                    x_s = engine.gather_rows(tab_s, si.reshape(-1)).view(len(ids) * N, S, W)
                    x_q = engine.gather_rows(tab_q, qi.reshape(-1)).view(len(ids) * N, Q, W)
                    x_s, x_q, y_s, y_q = relabel_batch(x_s, x_q, y_s, y_q, a.use_softmax_feature)
                # BDCSPN normalises the features in run_task, before run_method (few_shot/bdcspn.py:165-166): run_batch does both
                m.run_batch(support=x_s, query=x_q, y_s=y_s.to(dev), y_q=y_q.to(dev), n_batches=len(ids))
            logs = m.get_logs()
            parts = sharding.concat_parts(parts, sharding.method_parts(a, m, logs, len(ids), N, Q, dev))
            timestamps += [float(logs['timestamps'])] * len(ids)
        if parts is None:      # more ranks than batches: this rank only takes part in the gather
            parts = sharding.method_parts(a, None, None, 0, N, Q, dev)
        got = sharding.gather_packed(parts, n_batches)
        # a rank whose only batch is batch 0 of a tuned run executes `first_method` alone: `method` never ran there and
        # carries no records (mm_iters None); a rank without a batch keeps the freshly built object
        self.last_method = ran if ran is not None else method
        if got is None:
            return None, None
        acc = got['acc'].numpy()
        results_task = [compute_confidence_interval(acc[b])[0] for b in range(n_batches)]
        self.last_task_accuracies = acc
        self.last_task_predictions = got['preds'].view(n_batches, N, Q).numpy()
        self.last_batch_criterions = got['criterions'].numpy() if 'criterions' in got else None
        self.last_batch_mm_iters = got['mm_iters'].numpy() if 'mm_iters' in got else None
        return np.asarray(results_task).mean(), (float(np.mean(timestamps)) if timestamps else 0.0)
