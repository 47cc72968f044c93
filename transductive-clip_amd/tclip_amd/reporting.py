"""Result files in the reference's format (src/eval_zero_shot.py:189-232, src/eval_few_shot.py:272-338):
the test-mode row per run, and for few-shot runs on the validation split the `val_param<TAB>acc` sweep
file that test runs of a tunable method (PADDLE, BDCSPN) read their parameter from
(eval_few_shot.py:152-187 -> Evaluator_few_shot.set_method_opt_param)."""
import os

# The parameter a validation sweep varies, per method (eval_few_shot.py:130-139).
VAL_PARAM = {"LAPLACIAN_SHOT": "lmd", "ALPHA_TIM": "alpha_value", "PADDLE": "lambd", "BDCSPN": "temp"}


def saved_feature_path(args, split, root="."):
    """data/<dataset>/saved_features/<split>_softmax_<backbone>_T<T>.plk, or <split>_visual_<backbone>.plk
    (src/utils.py:266-267, 324-325)."""
    name = ("{}_softmax_{}_T{}.plk".format(split, args.backbone, args.T) if args.use_softmax_feature
            else "{}_visual_{}.plk".format(split, args.backbone))
    return os.path.join(root, "data", str(args.dataset), "saved_features", name)


def _result_file(args, root, split, dataset, few):
    """results_few_shot/<split>/<dataset>/<METHOD>_<softmax|visual>_s<shots>.txt; zero-shot runs (not `few`):
    results_zero_shot/... and ..._<shots>shot.txt"""
    name = (("{}_s{}.txt" if few else "{}_{}shot.txt")
            .format(args.name_method + ("_softmax" if args.use_softmax_feature else "_visual"), args.shots))
    return os.path.join(root, "results_few_shot" if few else "results_zero_shot", str(split), str(dataset), name)


def validation_file(args, root=".", dataset=None):
    """The sweep file of a tunable few-shot method, always in the few-shot layout: validation runs append their
    `val_param<TAB>acc` rows to it, test runs read their parameter from it.  `dataset`: another dataset's file (imagenet
    borrows caltech101's, eval_few_shot.py:161-166)."""
    return _result_file(args, root, "val", args.dataset if dataset is None else dataset, True)


def _append_row(name_file, header, row):
    os.makedirs(os.path.dirname(name_file), exist_ok=True)
    new = not os.path.isfile(name_file)
    with open(name_file, "w" if new else "a") as f:
        f.write((header if new else "") + row + "\t\n")
    return name_file


def report_results(args, mean_accuracies, mean_times, logger=None, root="."):
    """Appends one row to results_{zero,few}_shot/<used_test_set>/<dataset>/<METHOD>_<softmax|visual>_...txt
    exactly as the reference's Evaluator_*.report_results does when `save_results` is set; returns
    the file path (or None when nothing is written)."""
    few = int(getattr(args, "shots", 0)) > 0
    info = logger.info if logger is not None else (lambda *_: None)
    info("----- Final results -----")
    info("{}-shot mean test accuracy over {} tasks: {}".format(args.shots, args.number_tasks, mean_accuracies))
    if few and args.used_test_set == "val":                 # eval_few_shot.py:282-302: written whatever save_results says
        if args.name_method not in VAL_PARAM:
            raise AttributeError("method {} has no validation parameter".format(args.name_method))  # reference: self.val_param unset
        return _append_row(validation_file(args, root), "val_param\tacc\n",
                           "{}\t{}".format(args[VAL_PARAM[args.name_method]], round(100 * float(mean_accuracies), 2)))
    info("{}-shot mean time over {} tasks: {}".format(args.shots, args.number_tasks, mean_times))
    if not getattr(args, "save_results", False) or (few and args.used_test_set != "test"):
        return None
    names, last = ("shots\tn_query\tk_eff\tacc\n", args.k_eff) if few else ("shots\tn_query\tn_task\tacc\n", args.number_tasks)
    return _append_row(_result_file(args, root, args.used_test_set, args.dataset, few), names + "\t\n",
                       "{}\t{}\t{}\t{}".format(args.shots, args.n_query, last, round(100 * float(mean_accuracies), 1)))
