"""Task-batch loop of the zero-shot evaluation (reference: src/eval_zero_shot.py:140-187),
rebuilt around the batched engine: the index tensors of ALL batches are drawn first (the method
itself consumes no random numbers, so the reference's RNG stream is reproduced), the feature
table lives on the GPU, rows are gathered there, and every batch of this rank runs in one engine
call with n_batches > 1 (each batch keeps its own MM stop test).  With torch.distributed
initialised, batches are dealt round-robin to the ranks and gathered once onto rank 0.

Feature extraction and dataset handling of the reference's Evaluator are out of scope (they need CLIP
weights and images): run_full_evaluation starts from the saved feature files the reference writes."""
import torch

from src._evaluator import EvaluatorBase, _as_tensor, check_record_objective, check_stop_patience
from src.methods.zero_shot.em_dirichlet import EM_DIRICHLET
from src.methods.zero_shot.hard_em_dirichlet import HARD_EM_DIRICHLET
from src.methods.zero_shot.em_gaussian import EM_GAUSSIAN
from src.methods.zero_shot.inductive_clip import CLIP
from src.methods.zero_shot.em_gaussian_cov import EM_GAUSSIAN_COV
from src.methods.zero_shot.hard_kmeans import HARD_KMEANS
from src.methods.zero_shot.kl_kmeans import KL_KMEANS
from src.methods.zero_shot.soft_kmeans import SOFT_KMEANS
from src.sampler_zero_shot import CategoriesSampler_zero_shot, SamplerQuery_zero_shot
from tclip_amd import engine, sharding

_METHODS = {'EM_DIRICHLET': EM_DIRICHLET, 'HARD_EM_DIRICHLET': HARD_EM_DIRICHLET, 'SOFT_KMEANS': SOFT_KMEANS,
            'HARD_KMEANS': HARD_KMEANS, 'EM_GAUSSIAN': EM_GAUSSIAN, 'EM_GAUSSIAN_COV': EM_GAUSSIAN_COV,
            'KL_KMEANS': KL_KMEANS, 'CLIP': CLIP}


class Evaluator_zero_shot(EvaluatorBase):
    _METHODS = _METHODS

    def run_full_evaluation(self, model, preprocess):
        """eval_zero_shot.py:44-72 for the case the reference itself short-cuts: when the feature file of the
        split is already saved the reference skips CLIP (utils.py:266-271 "Features already saved ... skipping")
        and goes from the pickle to evaluate_tasks and report_results; `model`/`preprocess` are then unused and
        may be None.  Extracting features needs CLIP and the image datasets and is not part of this package."""
        dic = self.extract_and_load_features(model, None, None)
        all_features_query = dic['concat_features'].to('cpu')
        all_labels_query = dic['concat_labels'].long().to('cpu')
        mean_accuracies, mean_times = self.evaluate_tasks(model, all_features_query, all_labels_query)
        if mean_accuracies is not None:            # rank 0 (every rank without torch.distributed)
            self.report_results(mean_accuracies, mean_times)
        return mean_accuracies, mean_times

    def extract_and_load_features(self, model, dataset, data_loaders):
        """eval_zero_shot.py:89-111, loading only: the `used_test_set` split (EvaluatorBase.load_split)."""
        return self.load_split(self.args.used_test_set)

    def sample_indices(self, all_labels_query):
        """(n_batches, batch_size, n_query) int64 index tensor, drawn batch by batch exactly as
        the reference does (a fresh sampler per batch)."""
        a = self.args
        return self._draw_batches(lambda: CategoriesSampler_zero_shot(a.batch_size, a.k_eff, a.n_class, a.n_query,
                                                                      force_query_size=True),
                                  (all_labels_query,), (SamplerQuery_zero_shot,))[0]

    def evaluate_tasks(self, model, all_features_query, all_labels_query, indices=None):
        """`indices`: an index tensor drawn earlier with sample_indices() (bench.py draws it outside its
        timed region); None draws it here, as the reference's loop does.  The feature table and the
        labels may already live on the device."""
        a = self.args
        check_stop_patience(a)
        check_record_objective(a)
        self.logger.info("=> Runnning evaluation with method {} on {} dataset".format(
            a.name_method, getattr(a, 'used_test_set', 'test')))
        dev = torch.device(self.device)
        table = _as_tensor(all_features_query).float().to(dev)
        labels = _as_tensor(all_labels_query).long()
        idx = self.sample_indices(labels.cpu().numpy()) if indices is None else indices   # every rank: the same stream
        n_batches, N, Q = idx.shape
        mine = sharding.my_batches(n_batches)
        K = table.shape[1]
        method = self.get_method_builder(model=model, device=self.device, args=a, log_file=self.log_file)
        timestamps, parts = [], None
        if mine:
            my_idx = idx[mine].reshape(-1)
            x_q = engine.gather_rows(table, my_idx).view(len(mine) * N, Q, K)
            y_q = labels[my_idx.to(labels.device)].view(len(mine) * N, Q)
            method.run_method(query=x_q, y_q=y_q.to(dev), n_batches=len(mine))   # SOFT_KMEANS has no cross-task coupling
            logs = method.get_logs()
            parts = sharding.method_parts(a, method, logs, len(mine), N, Q, dev)
            timestamps = [float(logs['timestamps'])]
        return self._gathered(parts, n_batches, N, Q, method, timestamps)
