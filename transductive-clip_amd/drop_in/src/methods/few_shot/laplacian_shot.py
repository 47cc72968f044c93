"""Few-shot LAPLACIAN_SHOT on probability features, drop-in for the reference's src/methods/few_shot/laplacian_shot.py
(SURVEY.md F4).  Same constructor / run_task / logs contract (`acc` is (n_task, iter): the accuracy after every bound
update, the evaluator reads the last column; `ent_energy` (n_task, iter); `criterions` one [0] per task); normalisation,
prototypes, unary term, kNN graph and the bound updates run in libtclip.so (tclip_laplacian_shot_run), one workgroup per
task instead of the reference's numpy / scipy.sparse / sklearn host loop.  Pinned to reference-made fixtures within a
tolerance (tests/test_laplacian_shot.py).  The reference class itself does not run on numpy >= 1.24
(`dtype=np.float`, laplacian_shot.py:100)."""
import time

import numpy as np
import torch

from src.utils import Logger
from tclip_amd import engine


class LAPLACIAN_SHOT(object):
    def __init__(self, model, device, log_file, args):
        self.device = device
        self.knn = args.knn
        self.norm_type = args.norm_type
        self.iter = args.iter
        self.number_tasks = args.batch_size
        self.model = model
        self.log_file = log_file
        self.logger = Logger(__name__, self.log_file)
        self.shots = args.shots
        self.lmd = args.lmd
        self.temp = args.temp
        self.timestamps = []
        self.criterions = []
        self.ent_energy = []
        self.test_acc = []
        self.args = args

    def __del__(self):
        try:
            self.logger.del_logger()
        except Exception:
            pass

    def get_logs(self):
        self.test_acc = np.asarray(self.test_acc, dtype=np.float32)
        self.ent_energy = np.asarray(self.ent_energy)
        self.timestamps = np.array(self.timestamps).mean()
        return {'timestamps': np.array(self.timestamps).mean(), 'acc': self.test_acc, 'ent_energy': self.ent_energy,
                'criterions': self.criterions}

    def run_task(self, task_dic, shot):
        y_s, y_q = task_dic['y_s'], task_dic['y_q']
        x_s, x_q = task_dic['x_s'], task_dic['x_q']
        self.run_method(support=x_s.to(self.device).float(), query=x_q.to(self.device).float(),
                        y_s=y_s.long().squeeze(2).to(self.device), y_q=y_q.long().squeeze(2).to(self.device))
        return self.get_logs()

    def run_method(self, support, query, y_s, y_q, n_batches=1):
        if query.shape[2] != self.args.num_classes_test:
            raise NotImplementedError("LAPLACIAN_SHOT here takes probability features (use_softmax_feature: True, feature dimension = n_class)")
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("LAPLACIAN_SHOT on MI355X needs device='cuda': there is no CPU fallback in this package")
        self.logger.info(" ==> Executing LAPLACIAN SHOT with lmd = {}".format(self.lmd))
        n_task = query.shape[0]
        torch.cuda.synchronize(dev)
        t0 = time.time()
        self.unary, self.neighbours, self.preds_iter, energies = engine.run_laplacian_shot(
            query, support, y_s, iters=self.iter, knn=self.knn, lmd=self.lmd, norm_type=self.norm_type)
        torch.cuda.synchronize(dev)
        total = time.time() - t0
        self.preds = self.preds_iter[:, -1, :]
        # accuracy after every update, on the host: means of 75 zeros and ones rounded as the reference's CPU op rounds them
        hit = (self.preds_iter.long().cpu() == y_q.cpu().unsqueeze(1)).float()          # (n_task, iter, Q)
        self.test_acc = list(hit.mean(2).numpy())
        self.ent_energy = list(energies.cpu().numpy())
        for i in range(n_task):
            # the reference appends the cumulative wall time after every task (laplacian_shot.py:243-245)
            self.timestamps.append(total * (i + 1) / n_task)
            self.criterions.append([0])
