"""What the two task-batch loops (src/eval_zero_shot.py, src/eval_few_shot.py) share: the constructor, the method table
look-up, the saved-feature files, the result rows, the per-batch samplers and the tail that gathers a run's results onto
rank 0."""
import contextlib
import os

import numpy as np
import torch

from src.utils import Logger, compute_confidence_interval
from tclip_amd import features, reporting, sharding


def _as_tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


@contextlib.contextmanager
def arg_set_to(args, attr, value):
    """args[attr] is `value` inside the block and what it was before afterwards, whatever the block raises"""
    saved = args[attr]
    args[attr] = value
    try:
        yield
    finally:
        args[attr] = saved


@contextlib.contextmanager
def arg_hidden(args, attr):
    """args has no `attr` inside the block and what it had before afterwards, whatever the block raises"""
    missing = object()
    saved = args.pop(attr, missing) if isinstance(args, dict) else missing
    try:
        yield
    finally:
        if saved is not missing:
            args[attr] = saved


_STOP_PATIENCE_METHODS = ('EM_DIRICHLET', 'HARD_EM_DIRICHLET')


def check_stop_patience(args):
    """args.stop_patience (not a default: absent unless given) belongs to the EM-Dirichlet classes: ValueError for any other
    method, before anything touches the device.  Returns the option's value or None."""
    try:
        patience = getattr(args, 'stop_patience', None)
    except KeyError:
        patience = None
    if patience is not None and getattr(args, 'name_method', None) not in _STOP_PATIENCE_METHODS:
        raise ValueError("stop_patience stops a batch of EM_DIRICHLET / HARD_EM_DIRICHLET once its assignments are stable: "
                         f"method {getattr(args, 'name_method', None)!r} has no such stop")
    return patience


def check_record_objective(args):
    """args.record_objective (not a default: absent unless given) belongs to the EM-Dirichlet classes too: ValueError for any
    other method, before anything touches the device.  Returns whether the objective is to be recorded."""
    try:
        on = bool(getattr(args, 'record_objective', None))
    except KeyError:
        on = False
    if on and getattr(args, 'name_method', None) not in _STOP_PATIENCE_METHODS:
        raise ValueError("record_objective records the penalised objective EM_DIRICHLET / HARD_EM_DIRICHLET descend: "
                         f"method {getattr(args, 'name_method', None)!r} has no such record")
    return on


class EvaluatorBase:
    _METHODS = {}       # name_method -> class: the subclass's table

    def __init__(self, device, args, log_file):
        self.device = device
        self.args = args
        self.log_file = log_file
        self.logger = Logger(type(self).__module__, self.log_file)

    def get_method_builder(self, model, device, args, log_file):
        try:
            cls = self._METHODS[args.name_method]
        except KeyError:
            raise ValueError(f"method {args.name_method!r} is not part of the EM-Dirichlet engine")
        return cls(model=model, device=device, log_file=log_file, args=args)

    def report_results(self, mean_accuracies, mean_times):
        """eval_zero_shot.py:189-232, eval_few_shot.py:272-338 (validation sweep row, or the test-mode row)."""
        return reporting.report_results(self.args, mean_accuracies, mean_times, self.logger,
                                        root=getattr(self.args, 'results_root', '.'))

    def load_split(self, split):
        """data/<dataset>/saved_features/<split>_{softmax_<backbone>_T<T>,visual_<backbone>}.plk under args.results_root
        (default: the working directory, as in the reference), as the reference's dictionary"""
        path = reporting.saved_feature_path(self.args, split, getattr(self.args, 'results_root', '.'))
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: this package runs the reference's evaluation from saved "
                                    "feature files; extract them with the reference (CLIP is out of scope here)")
        feats, labels = features.load_features(path)
        return {'concat_features': feats, 'concat_labels': labels}

    def _draw_batches(self, make_sampler, labels, draws):
        """One (n_batches, batch_size, n) index tensor per class of `draws`, drawn batch by batch exactly as the reference
        does: a fresh sampler per batch, the classes of `draws` iterated in their order.  The label -> index lists
        (`m_ind_*`) are a function of the labels alone and consume no random numbers: built for the first batch from `labels`,
        shared by the others (the reference rebuilds them per batch, sampler_zero_shot.py:31-36)."""
        a = self.args
        out, lists = [[] for _ in draws], None
        for _ in range(int(a.number_tasks / a.batch_size)):
            sampler = make_sampler()
            if lists is None:
                sampler.create_list_classes(*labels)
                lists = {k: v for k, v in vars(sampler).items() if k.startswith('m_ind_')}
            else:
                vars(sampler).update(lists)
            for drawn, draw in zip(out, draws):
                drawn.append(torch.stack(list(draw(sampler)), 0))
        return [torch.stack(drawn, 0) for drawn in out]

    def _gathered(self, parts, n_batches, N, Q, method, timestamps):
        """The one collective of a run and what it leaves behind: the per-task predictions, accuracies and per-batch records
        of every rank onto rank 0 (`parts`: this rank's, None when it had no batch; `timestamps`: one time per batch it ran).
        Sets last_method (`method`: the object that actually ran on this rank) and, on rank 0, last_task_accuracies,
        last_task_predictions, last_batch_criterions and last_batch_mm_iters (with args.stop_patience also
        last_batch_outer_iters, with args.record_objective also last_task_objectives).  Returns (mean over the batches of their mean
        accuracies, mean time), or (None, None) off rank 0."""
        if parts is None:      # more ranks than batches: this rank only takes part in the gather
            parts = sharding.method_parts(self.args, None, None, 0, N, Q, torch.device(self.device))
        got = sharding.gather_packed(parts, n_batches)
        self.last_method = method
        if got is None:
            return None, None
        acc = got['acc'].numpy()
        results_task = [compute_confidence_interval(acc[b])[0] for b in range(n_batches)]
        self.last_task_accuracies = acc
        self.last_task_predictions = got['preds'].view(n_batches, N, Q).numpy()      # class per query, every batch of the run
        self.last_batch_criterions = got['criterions'].numpy() if 'criterions' in got else None     # (n_batches, iter)
        self.last_batch_mm_iters = got['mm_iters'].numpy() if 'mm_iters' in got else None
        if 'outer_iters' in got:       # args.stop_patience: the outer iterations every batch ran, (n_batches,)
            self.last_batch_outer_iters = got['outer_iters'].numpy().reshape(n_batches)
        if 'objectives' in got:        # args.record_objective: the objective of every task after every outer iteration, float64
            self.last_task_objectives = sharding.objectives_of(got['objectives']).numpy()      # (n_batches, N, iter)
        return np.asarray(results_task).mean(), (float(np.mean(timestamps)) if timestamps else 0.0)
