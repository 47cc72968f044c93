/* tclip.h - C ABI of the MI355X (gfx950) EM-Dirichlet / Hard EM-Dirichlet engine.
 *
 * The reference (SegoleneMartin/transductive-CLIP) has no native layer: its hot path is a chain
 * of PyTorch-eager ops inside four Python method classes.  This header is therefore the FFI a
 * maintainer of the reference would bind (ctypes stub in INTEGRATION.md) to replace, per batch,
 *     src/methods/zero_shot/em_dirichlet.py:179-246        EM_DIRICHLET.run_method
 *     src/methods/zero_shot/hard_em_dirichlet.py:200-271   HARD_EM_DIRICHLET.run_method
 *     src/methods/few_shot/em_dirichlet.py:149-220         EM_DIRICHLET.run_method
 *     src/methods/few_shot/hard_em_dirichlet.py:172-251    HARD_EM_DIRICHLET.run_method
 * and the accuracy tail src/methods/zero_shot/em_dirichlet.py:61-92 + src/utils.py:380-417.
 *
 * Conventions: every pointer marked "device" is a HIP device pointer of a row-major contiguous
 * array; the library never allocates device memory (the caller passes a workspace sized by
 * tclip_workspace_bytes, so PyTorch's caching allocator stays the owner), never synchronises
 * the stream, and keeps no state between calls except a thread-local error string.  All entry
 * points return 0 on success and a non-zero code otherwise (see tclip_last_error()).
 */
#ifndef TCLIP_H
#define TCLIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: tclip_alpha_tim_run, tclip_laplacian_shot_run, tclip_match_clusters_host_strided, tclip_debug_set_mm_split added
 * 3: tclip_em_dirichlet_run_tasks (tclip_task_source) added
 * 4: tclip_check_task_indices, tclip_profile_last_split_sorts, tclip_debug_set_split_keep_placement added
 * 5: TCLIP_ERR_INDEX: tclip_check_task_indices reports an out-of-range VALUE with its own code (bad arguments stay TCLIP_ERR_ARG);
 *    tclip_debug_set_dead_head added
 *    later, without a new number (additions only; a client that needs them looks the symbols up):
 *    tclip_visual_workspace_bytes, tclip_kmeans_visual_run, tclip_cluster_prototypes_visual, tclip_visual_init;
 *    tclip_paddle_visual_workspace_bytes, tclip_paddle_visual_run, tclip_bdcspn_visual_workspace_bytes, tclip_bdcspn_visual_run;
 *    tclip_tim_gd_workspace_bytes, tclip_tim_gd_run;
 *    tclip_alpha_tim_visual_workspace_bytes, tclip_alpha_tim_visual_run, tclip_laplacian_shot_visual_workspace_bytes,
 *    tclip_laplacian_shot_visual_run;
 *    tclip_match_clusters_workspace_bytes, tclip_match_clusters;
 *    tclip_em_gaussian_cov_visual_workspace_bytes, tclip_em_gaussian_cov_visual_run;
 *    tclip_gather_task_rows, tclip_paddle_tasks_workspace_bytes, tclip_paddle_run_tasks,
 *    tclip_paddle_visual_tasks_workspace_bytes, tclip_paddle_visual_run_tasks;
 *    tclip_bdcspn_tasks_workspace_bytes, tclip_bdcspn_run_tasks, tclip_bdcspn_visual_tasks_workspace_bytes,
 *    tclip_bdcspn_visual_run_tasks, tclip_laplacian_shot_tasks_workspace_bytes, tclip_laplacian_shot_run_tasks,
 *    tclip_laplacian_shot_visual_tasks_workspace_bytes, tclip_laplacian_shot_visual_run_tasks;
 *    tclip_alpha_tim_tasks_workspace_bytes, tclip_alpha_tim_run_tasks, tclip_alpha_tim_visual_tasks_workspace_bytes,
 *    tclip_alpha_tim_visual_run_tasks, tclip_tim_gd_tasks_workspace_bytes, tclip_tim_gd_run_tasks;
 *    tclip_paddle_sweep_tasks_workspace_bytes, tclip_paddle_sweep_tasks, tclip_bdcspn_sweep_tasks_workspace_bytes,
 *    tclip_bdcspn_sweep_tasks, tclip_laplacian_shot_sweep_tasks_workspace_bytes, tclip_laplacian_shot_sweep_tasks,
 *    tclip_alpha_tim_sweep_tasks_workspace_bytes, tclip_alpha_tim_sweep_tasks;
 *    tclip_debug_set_mm_reuse, tclip_profile_last_mm_reuse;
 *    tclip_em_dirichlet_score_workspace_bytes, tclip_em_dirichlet_score, tclip_em_dirichlet_score_tasks (tclip_score_problem)
 * (every entry point of an earlier version keeps its signature) */
#define TCLIP_ABI_VERSION 5

enum {
    TCLIP_OK = 0,
    TCLIP_ERR_ARG = 1,        /* bad argument (null pointer, non-positive size, K out of range) */
    TCLIP_ERR_WORKSPACE = 2,  /* workspace too small or misaligned */
    TCLIP_ERR_HIP = 3,        /* a HIP call failed; text in tclip_last_error() */
    TCLIP_ERR_INDEX = 4       /* tclip_check_task_indices: a value of an index tensor lies outside its table (torch: IndexError) */
};

/* One call = n_batches independent reference batches of tasks_per_batch tasks each.  Tasks of
 * one batch are coupled by the majorize-minimize stop test, which the reference evaluates over
 * the whole (n_task, K, K) tensor every 50 inner iterations (em_dirichlet.py:169-175); batches
 * never interact.  Task t = b * tasks_per_batch + n. */
typedef struct tclip_problem {
    int32_t n_batches;        /* B >= 1                                                        */
    int32_t tasks_per_batch;  /* N >= 1   (the reference's batch_size)                         */
    int32_t n_query;          /* Q >= 1   (75 in every reference config)                       */
    int32_t n_class;          /* K, 2..1024: classes == feature dimension (softmax features)   */
    int32_t n_support;        /* S >= 0: support rows per task; 0 selects the zero-shot variant */
    int32_t iters;            /* outer iterations (args.iter: 20 soft / 10 hard)               */
    int32_t iter_mm;          /* inner MM iteration cap (args.iter_mm: 1000)                   */
    int32_t lambd;            /* the reference's integer lambd = int(K/5)*Q or int(K/k_eff)*Q  */
    int32_t hard;             /* 0 = EM_DIRICHLET, 1 = HARD_EM_DIRICHLET                       */
} tclip_problem;

int tclip_abi_version(void);
const char* tclip_last_error(void);

/* Bytes of device workspace tclip_em_dirichlet_run needs for this problem (0 on bad input). */
size_t tclip_workspace_bytes(const tclip_problem* p);

/* Runs the whole loop (A3-A12 of SURVEY.md section 8a) on `stream` and returns without waiting.
 *   x_q   device [B*N, Q, K] f32  probability features of the query set (rows on the simplex)
 *   x_s   device [B*N, S, K] f32  support features, NULL iff S == 0
 *   y_s   device [B*N, S]   i64   support labels in [0, K), NULL iff S == 0
 *   u     device [B*N, Q, K] f32  out: responsibilities after the last E-step (one-hot if hard)
 *   v     device [B*N, K]    f32  out: dual variable / log class proportions
 *   alpha device [B*N, K, K] f32  out: Dirichlet parameters, one K-vector per class
 *   preds device [B*N, Q]    i32  out: argmax_k u (first maximum, as torch.argmax)
 *   criterions device [B, iters] f32 out: per outer iteration, mean_n ||a_old-a||_F/||a_old||_F
 *   mm_iters   device [B, iters] i32 out: MM iterations executed in each outer iteration
 * Inputs are not modified (the few-shot reference logs x_s/x_q in place; this does not). */
int tclip_em_dirichlet_run(const tclip_problem* p, const float* x_q, const float* x_s, const int64_t* y_s,
                           float* u, float* v, float* alpha, int32_t* preds, float* criterions,
                           int32_t* mm_iters, void* workspace, size_t workspace_bytes, void* stream);

/* The same loop fed from the feature TABLES of the task-batch loop instead of per-task tensors: what
 *     src/eval_few_shot.py:233-241            all_features_{support,query}[indices, :]   (zero-shot: eval_zero_shot.py:160-163)
 *     src/task_generator_few_shot.py:41-52    data[:, unique_labels] with unique_labels = flip(unique(labels_support))
 * materialise as x_s (T,S,K) and x_q (T,Q,K) - 16 MB per task at K = 1000, 4 shots - is read in place: row r of task t is
 * table[idx[t,r]], its column d is table column cols[t,d].  Results are those of tclip_em_dirichlet_run on the materialised
 * tensors, bit for bit.
 *   table_q device [rows_q, K] f32, q_idx device [B*N, Q] i64 (rows of table_q)
 *   table_s device [rows_s, K] f32, s_idx device [B*N, S] i64 (rows of table_s); both NULL iff S == 0
 *   cols    device [B*N, K] i32 column permutation per task (applied to both tables), or NULL for the identity
 *   y_s     device [B*N, S] i64 support labels AFTER get_task's re-indexing (new label j = position of the old label in
 *           unique_labels), NULL iff S == 0
 * tclip_em_dirichlet_run_tasks itself does not know the tables' row counts and reads what the index tensors say: call
 * tclip_check_task_indices on them first (the Python binding does, for host and device tensors alike). */
typedef struct tclip_task_source {
    const float* table_q;
    const int64_t* q_idx;
    const float* table_s;
    const int64_t* s_idx;
    const int32_t* cols;
} tclip_task_source;
int tclip_em_dirichlet_run_tasks(const tclip_problem* p, const tclip_task_source* src, const int64_t* y_s,
                                 float* u, float* v, float* alpha, int32_t* preds, float* criterions,
                                 int32_t* mm_iters, void* workspace, size_t workspace_bytes, void* stream);

/* The same two loops, each batch stopped once its argmax assignment stands still (opt-in; the plain entries run every
 * iteration).  After outer iteration `it` (0-based) of batch b
 *     changes[b, it] = number of (task, query) pairs of the batch whose preds differ from those after iteration it - 1,
 *     changes[b, 0]  = N * Q (no iteration precedes it),
 * and the batch is stable after the first `it` with changes[b, it-patience+1 .. it] all 0.  Then outer_iters[b] = it + 1
 * (at least patience + 1) and nothing of batch b is written any more: u, v, alpha and preds keep their values, and
 * criterions[b, j], mm_iters[b, j] and changes[b, j] are 0 for j >= outer_iters[b] (the entry zero-fills the three arrays).  A
 * batch that never qualifies has outer_iters[b] = iters.  The decision is taken on the device (no host synchronisation).
 * Contract: with s = outer_iters[b], the slices u, v, alpha, preds, criterions[b, :s], mm_iters[b, :s] of batch b are bit for
 * bit what the plain entry returns for that batch alone with iters = s - zero-shot and few-shot, soft and hard, dense rows
 * and table rows, whatever other batches share the call and however it is split over stream groups.
 *   patience    >= 1
 *   outer_iters device [B]        i32 out
 *   changes     device [B, iters] i32 out
 * Checks are those of the plain entries; patience < 1, a null outer_iters or changes are TCLIP_ERR_ARG before any launch (the
 * error text names the argument).  Workspace: tclip_em_dirichlet_until_stable_workspace_bytes(p) bytes (0 on bad input),
 * 256-byte aligned; it is tclip_workspace_bytes(p) plus, per stream group, the previous predictions and two words per batch. */
size_t tclip_em_dirichlet_until_stable_workspace_bytes(const tclip_problem* p);
int tclip_em_dirichlet_run_until_stable(const tclip_problem* p, const float* x_q, const float* x_s, const int64_t* y_s,
                                        int32_t patience, float* u, float* v, float* alpha, int32_t* preds, float* criterions,
                                        int32_t* mm_iters, int32_t* outer_iters, int32_t* changes, void* workspace,
                                        size_t workspace_bytes, void* stream);
int tclip_em_dirichlet_run_tasks_until_stable(const tclip_problem* p, const tclip_task_source* src, const int64_t* y_s,
                                              int32_t patience, float* u, float* v, float* alpha, int32_t* preds,
                                              float* criterions, int32_t* mm_iters, int32_t* outer_iters, int32_t* changes,
                                              void* workspace, size_t workspace_bytes, void* stream);

/* The same loops, observed (opt-in): the penalised clustering objective they descend - the reference's objective_function
 * (src/methods/zero_shot/hard_em_dirichlet.py:179-198, few_shot/hard_em_dirichlet.py:149-168), which it defines and never calls -
 * as four float64 terms per task and outer iteration.  After outer iteration `it` of task t, on the state that iteration
 * leaves (alpha after the dead-row revert, u after the E-step - one-hot if hard -, eps = 1e-15):
 *     objective_terms[t, it, 0] = fit_q = sum_n sum_k u[n,k] * logit[n,k]      logit: the E-step's fp32 get_logits(query),
 *                                                                              before lambd * v / Q is added
 *     objective_terms[t, it, 1] = fit_s = sum_s get_logits(support)[s, y_s], from the per-class support sums  (0 in zero-shot)
 *     objective_terms[t, it, 2] = ent   = sum_n sum_k u * log(u + eps)
 *     objective_terms[t, it, 3] = part  = sum_k p_k * log(p_k + eps),  p_k = (sum_n u[n,k]) / n_query
 * and the reference's value is  -(fit_q + fit_s) / 2 + ent - lambd * part;  composing it is the caller's.  The operands are
 * the engine's fp32 values, every product and sum is float64, and the order of each sum is fixed by (n_query, n_class) alone:
 * the terms of a task have the same bits whatever shares the call and however it is split over stream groups, and the first s
 * iterations of a run do not depend on iters.
 *   patience        0: the plain schedule (outer_iters and changes are not written and may be NULL);
 *                   >= 1: the until-stable schedule above; a batch has zeros from its outer_iters[b] on
 *   objective_terms device [B * N, iters, 4] f64 out, zero-filled by the entry
 * Every other output is bit for bit that of the plain entry (patience 0) or of the until-stable entry (patience >= 1).
 * Checks are those entries'; patience < 0 or a null objective_terms are TCLIP_ERR_ARG before any launch (the error text names
 * the argument).  Workspace: tclip_em_dirichlet_objective_workspace_bytes(p, patience) bytes (0 on bad input), 256-byte
 * aligned: the plain or the until-stable workspace plus two doubles per (task, query) row; it does not depend on n_support. */
size_t tclip_em_dirichlet_objective_workspace_bytes(const tclip_problem* p, int32_t patience);
int tclip_em_dirichlet_run_objective(const tclip_problem* p, const float* x_q, const float* x_s, const int64_t* y_s,
                                     int32_t patience, float* u, float* v, float* alpha, int32_t* preds, float* criterions,
                                     int32_t* mm_iters, int32_t* outer_iters, int32_t* changes, double* objective_terms,
                                     void* workspace, size_t workspace_bytes, void* stream);
int tclip_em_dirichlet_run_tasks_objective(const tclip_problem* p, const tclip_task_source* src, const int64_t* y_s,
                                           int32_t patience, float* u, float* v, float* alpha, int32_t* preds, float* criterions,
                                           int32_t* mm_iters, int32_t* outer_iters, int32_t* changes, double* objective_terms,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* Scoring with a fitted model: one E-step of a given (alpha, v) on rows that need not have been queries of the fit - "fit on
 * a sample, label the rest of the table".  A run's alpha [T,K,K] and v [T,K] are a complete mixture model per task (one
 * Dirichlet per class and the penalised class weights); per task t and scored row r, with z the row and eps = 1e-15,
 *     logits[t,r,k] = lgamma(sum_d alpha[t,k,d]) + (-sum_d lgamma(alpha[t,k,d])) + sum_d (alpha[t,k,d] - 1) * log(z[d] + eps)
 *                     the reference's get_logits (src/methods/zero_shot/em_dirichlet.py:35-39), in fp32
 *     u[t,r,:]      = softmax_k(logits[t,r,k] + (lambd * v[t,k]) / (float)n_query)     (:142-143; v == NULL: softmax_k(logits))
 *     preds[t,r]    = first maximum of u[t,r,:], a NaN counting as the maximum (torch.argmax); hard: u is the one-hot of preds
 * with the operations and summation orders of the loop's own E-step.  The reference's loop ends with the dead-row revert, v_update
 * and u_update(query), so scoring a run's x_q with its alpha, v, lambd and n_query returns that run's u and preds bit for bit.
 * The bits of a scored row depend on (its features, alpha[t], v[t], lambd, n_query, n_class) and on nothing else: not on
 * rows_per_task, n_task, the row's position, what shares the call, the dense or the table route, or which outputs were asked for.
 * In zero-shot the classes are clusters; matching clusters to classes stays with the accuracy tail (tclip_match_clusters).
 *   x      device [T,R,K] f32  rows on the simplex (dense entry)
 *   table  device [rows,K] f32, idx device [T,R] i64 rows of it, cols device [T,K] i32 column permutation per task or NULL: row r
 *          of task t is table[idx[t,r]], its column d is table column cols[t,d], read in place as tclip_em_dirichlet_run_tasks reads.
 *          The entry does not know the table's row count: call tclip_check_task_indices first (the Python binding does).
 *   alpha  device [T,K,K] f32, v device [T,K] f32 or NULL
 *   u      device [T,R,K] f32 out, or NULL for labels only (200 MB at R = 50 000, K = 1000)
 *   preds  device [T,R] i32 out;  logits device [T,R,K] f32 out or NULL
 * No allocation, no synchronisation, no state; inputs are not modified.  A null problem, x / table, idx, alpha, preds or workspace,
 * n_task < 1, rows_per_task < 1, n_query < 1, n_class outside 2..1024, n_task * n_class or n_task * rows_per_task beyond int32
 * are TCLIP_ERR_ARG before any launch (the error text names the argument).  Workspace:
 * tclip_em_dirichlet_score_workspace_bytes(p) bytes (0 on bad input), 256-byte aligned: the per-class row constants, T * K
 * floats - O(T K), independent of rows_per_task; the scored rows are staged in LDS only. */
typedef struct tclip_score_problem {
    int32_t n_task;         /* T >= 1 fitted models                                            */
    int32_t rows_per_task;  /* R >= 1 rows scored against each model                           */
    int32_t n_class;        /* K, 2..1024                                                      */
    int32_t lambd;          /* the fit's integer lambd                                         */
    int32_t n_query;        /* the FIT's Q >= 1: the prior term is (lambd * v[k]) / (float)Q   */
    int32_t hard;           /* 1: u is the one-hot of preds                                    */
} tclip_score_problem;
size_t tclip_em_dirichlet_score_workspace_bytes(const tclip_score_problem* p);
int tclip_em_dirichlet_score(const tclip_score_problem* p, const float* x /*[T,R,K]*/, const float* alpha /*[T,K,K]*/,
                             const float* v /*[T,K] or NULL*/, float* u /*[T,R,K] or NULL*/, int32_t* preds /*[T,R]*/,
                             float* logits /*[T,R,K] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);
int tclip_em_dirichlet_score_tasks(const tclip_score_problem* p, const float* table /*[rows,K]*/, const int64_t* idx /*[T,R]*/,
                                   const int32_t* cols /*[T,K] or NULL*/, const float* alpha, const float* v, float* u,
                                   int32_t* preds, float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* Range check of DEVICE-resident index tensors before tclip_em_dirichlet_run_tasks / tclip_gather_rows - what torch's own
 * `all_features_query[indices, :]` (src/eval_zero_shot.py:160-163, src/eval_few_shot.py:233-241) does by raising IndexError:
 *   idx  device [n_idx]  i64, every value must lie in [0, n_rows)         (NULL with n_idx == 0: nothing to check)
 *   cols device [n_cols] i32, every value must lie in [0, n_class)        (NULL with n_cols == 0)
 * One pass over each on `stream`, then the call WAITS for the stream (hipStreamSynchronize: a host sync per call) and returns
 * TCLIP_ERR_INDEX (text in tclip_last_error) when a value is out of range - negative values included: they are rejected, not
 * wrapped as torch wraps them -, TCLIP_ERR_ARG for a null pointer / negative count, TCLIP_OK otherwise.  Negligible next to the loop it protects (a few microseconds per
 * million indices); keeps one int32 of device memory per calling thread. */
int tclip_check_task_indices(const int64_t* idx, int64_t n_idx, int64_t n_rows, const int32_t* cols, int64_t n_cols,
                             int32_t n_class, void* stream);

/* Accuracy tail, device half: per task the clusters present in `preds` in first-appearance order
 * and the mean raw feature of each (compute_acc_clustering, em_dirichlet.py:61-71).
 *   x_q device [T,Q,K] f32, preds device [T,Q] i32
 *   n_clusters device [T] i32 out; cluster_ids device [T, Cmax] i32 out (first-appearance order,
 *   -1 padded); prototypes device [T, Cmax, K] f32 out, with Cmax = min(Q, K)
 *   workspace: tclip_prototype_workspace_bytes(T, Q, K) device bytes */
size_t tclip_prototype_workspace_bytes(int32_t n_task, int32_t n_query, int32_t n_class);
int tclip_cluster_prototypes(int32_t n_task, int32_t n_query, int32_t n_class, const float* x_q,
                             const int32_t* preds, int32_t* n_clusters, int32_t* cluster_ids,
                             float* prototypes, void* workspace, size_t workspace_bytes, void* stream);

/* Accuracy tail, host half (all pointers HOST memory): assigns clusters to classes by a
 * minimum-cost rectangular assignment on cost = -prototype (float64, as utils.py:380-405 feeds
 * scipy.optimize.linear_sum_assignment) when graph_matching != 0, else by argmax of the
 * prototype (utils.py:408-417), relabels preds and scores them against y_q.
 *   new_preds host [T,Q] i32 out, acc host [T] f32 out (mean_q new_pred == y_q) */
int tclip_match_clusters_host(int32_t n_task, int32_t n_query, int32_t n_class, const int32_t* preds,
                              const int32_t* n_clusters, const int32_t* cluster_ids,
                              const float* prototypes, const int64_t* y_q, int32_t graph_matching,
                              int32_t* new_preds, float* acc);
/* The same with an explicit row count per task of cluster_ids / prototypes ([T, c_stride] / [T, c_stride, K]
 * instead of Cmax): lets the caller copy to the host only as many prototype rows as the fullest task uses. */
int tclip_match_clusters_host_strided(int32_t n_task, int32_t n_query, int32_t n_class, const int32_t* preds,
                                      const int32_t* n_clusters, const int32_t* cluster_ids, const float* prototypes,
                                      const int64_t* y_q, int32_t graph_matching, int32_t c_stride, int32_t* new_preds,
                                      float* acc);

/* Accuracy tail, the matching ON THE DEVICE (all pointers DEVICE memory, asynchronous on `stream`): what
 * tclip_match_clusters_host_strided computes, bit for bit - same new_preds, same acc - from what tclip_cluster_prototypes[_visual]
 * (+ tclip_probability_features) leave on the device; no copy to the host, no host threads, no synchronisation.  One
 * wavefront per task runs the host's shortest-augmenting-path solver in fp64 with its scanning order and tie rule
 * (k_match_clusters, csrc/tclip_match.inc); graph_matching == 0 takes the first maximum of each prototype row.
 *   preds [T,Q] i32, n_clusters [T] i32, cluster_ids [T, c_stride] i32, prototypes [T, c_stride, K] f32, y_q [T,Q] i64;
 *   c_stride in 1..min(Q, K) - the full min(Q, K) of the prototype entries: nothing is read back to choose a smaller one;
 *   new_preds [T,Q] i32 out, acc [T] f32 out, status [T] i32 out.
 * Argument checks (T >= 1, Q >= 1, K in 2..1024, c_stride, null pointers) return TCLIP_ERR_ARG before any launch.  What the
 * host entry checks in the DATA is checked per task on the device, and no label is used as an index before it: a task with
 * n_clusters outside 1..c_stride (status 1), a cluster id (2) or a prediction (3) outside 0..K-1, or an infeasible assignment
 * (4: e.g. a NaN prototype row) gets status != 0, acc = NaN and new_preds = -1; the other tasks of the call are unaffected.
 * The kernel keeps a task in LDS (29 K + 13 c_stride bytes) and needs no global workspace: the query returns 0 and
 * `workspace` may be NULL. */
size_t tclip_match_clusters_workspace_bytes(int32_t n_task, int32_t n_query, int32_t n_class, int32_t c_stride);
int tclip_match_clusters(int32_t n_task, int32_t n_query, int32_t n_class, const int32_t* preds, const int32_t* n_clusters,
                         const int32_t* cluster_ids, const float* prototypes, const int64_t* y_q, int32_t graph_matching,
                         int32_t c_stride, int32_t* new_preds, float* acc, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Host threads tclip_match_clusters_host* may start: TCLIP_HOST_THREADS if set, else min(16, cores this process may run
 * on / LOCAL_WORLD_SIZE) - one process per GPU must not oversubscribe the node's cores. */
int tclip_host_threads(void);

/* Task construction for the task-batch loop (eval_zero_shot.py:160-168): gathers rows of a
 * device-resident feature table.  table device [n_rows, K] f32, idx device [n_out] i64,
 * out device [n_out, K] f32. */
int tclip_gather_rows(const float* table, int64_t n_rows, int32_t n_class, const int64_t* idx,
                      int64_t n_out, float* out, void* stream);

/* The fused task builder of the few-shot task-batch loop: the reference's `all_features[indices, :]`
 * (src/eval_few_shot.py:233-241) followed by get_task's `data[:, unique_labels]` (src/task_generator_few_shot.py:41-52) in one
 * pass over the table rows,
 *     out[r, d] = table[idx[r], cols ? cols[(r / rows_per_task) * width + d] : d].
 *   table device [n_rows, width] f32;  idx device [n_out] i64;  cols device [n_out / rows_per_task, width] i32 (one column
 *   permutation per task of rows_per_task rows) or NULL for the identity;  out device [n_out, width] f32.
 * A pure copy: every bit of every float is preserved, NaN payloads included.  An idx value outside [0, n_rows) is never
 * dereferenced and leaves its row of `out` unwritten, as tclip_gather_rows does; the values of cols are the caller's to check
 * (tclip_check_task_indices).  A null table, idx or out, n_rows < 1, width < 1, rows_per_task < 1, n_out < 0, and n_out not a
 * multiple of rows_per_task when cols is given are TCLIP_ERR_ARG before any launch.  Without cols, rows of a multiple of 4
 * floats in 16-byte aligned arrays move in 16-byte words; with cols the stores stay coalesced and the permuted loads hit the
 * row just fetched. */
int tclip_gather_task_rows(const float* table, int64_t n_rows, int32_t width, const int64_t* idx /*[n_out]*/, int32_t rows_per_task,
                           const int32_t* cols /*[n_out/rows_per_task, width] or NULL*/, int64_t n_out, float* out /*[n_out, width]*/,
                           void* stream);

/* SOFT_KMEANS on probability features (reference: src/methods/zero_shot/soft_kmeans.py:105-220;
 * BASELINE config 3's second method).  Uses p->n_batches * p->tasks_per_batch tasks, n_query,
 * n_class and iters; n_support must be 0; the other fields are ignored.  temperature = args.T.
 *   x_q device [T,Q,K] f32;  u device [T,Q,K] out;  w device [T,K,K] out (centroids);
 *   preds device [T,Q] i32 out.  The criterion the reference logs is identically 0. */
size_t tclip_soft_kmeans_workspace_bytes(const tclip_problem* p);
int tclip_soft_kmeans_run(const tclip_problem* p, const float* x_q, float temperature, float* u, float* w,
                          int32_t* preds, void* workspace, size_t workspace_bytes, void* stream);

/* EM_GAUSSIAN on probability features (reference: src/methods/zero_shot/em_gaussian.py:107-229):
 * SOFT_KMEANS with the class-proportion term, u = softmax_k(T * (-1/2 ||w_k - z_q||^2) + lambd v_k / Q),
 * v = log(mean_q u + eps) + 1 (p->lambd as for EM-Dirichlet: int(K/5) * n_query).  Same problem
 * fields and workspace (tclip_soft_kmeans_workspace_bytes) as SOFT_KMEANS; v device [T,K] out. */
int tclip_em_gaussian_run(const tclip_problem* p, const float* x_q, float temperature, float* u, float* v, float* w,
                          int32_t* preds, void* workspace, size_t workspace_bytes, void* stream);

/* EM_GAUSSIAN_COV on probability features (reference: src/methods/zero_shot/em_gaussian_cov.py:106-257):
 * EM_GAUSSIAN with a diagonal inverse covariance per cluster and no temperature,
 *   s = sum_q u / max(sum_q u (w - z_q)^2, eps)   (empty clusters keep w and s),
 *   u = softmax_k(-1/2 sum_d s (w - z)^2 + 1/2 sum_d log(s + eps) + lambd v_k / Q).
 * Same problem fields and workspace (tclip_soft_kmeans_workspace_bytes) as EM_GAUSSIAN;
 * s device [T,K,K] out. */
int tclip_em_gaussian_cov_run(const tclip_problem* p, const float* x_q, float* u, float* v, float* w, float* s,
                              int32_t* preds, void* workspace, size_t workspace_bytes, void* stream);

/* HARD_KMEANS on probability features (reference: src/methods/zero_shot/hard_kmeans.py:26-35,
 * 128-152, 186-204): centroids = means of the members, zero for empty clusters;
 * u = one_hot(argmin_k softmax_k ||w_k - z_q||^2) (first minimum).  Same problem fields as
 * SOFT_KMEANS (iters from p->iters, n_support = 0).
 *   x_q device [T,Q,K] f32;  u device [T,Q,K] out (one-hot);  w device [T,K,K] out;
 *   preds device [T,Q] i32 out;  criterions device [n_batches, iters] out: mean over the batch's
 *   tasks of ||u_old - u||_F (the reference logs each value twice). */
size_t tclip_hard_kmeans_workspace_bytes(const tclip_problem* p);
int tclip_hard_kmeans_run(const tclip_problem* p, const float* x_q, float* u, float* w, int32_t* preds,
                          float* criterions, void* workspace, size_t workspace_bytes, void* stream);

/* KL_KMEANS on probability features (reference: src/methods/zero_shot/kl_kmeans.py:123-189):
 * centroids w = (u^T z) / max(sum_q u, 1) with empty clusters at zero, every query assigned to the
 * centroid of smallest KL(z + eps || w + eps) (first minimum).  Problem fields, outputs and
 * workspace (tclip_hard_kmeans_workspace_bytes) as for HARD_KMEANS. */
int tclip_kl_kmeans_run(const tclip_problem* p, const float* x_q, float* u, float* w, int32_t* preds,
                        float* criterions, void* workspace, size_t workspace_bytes, void* stream);

/* BD-CSPN on probability features (reference: src/methods/few_shot/bdcspn.py:42-200; feature
 * dimension = n_class).  One pass: feature normalisation (norm_type 0 = UN, 1 = L2N, 2 = CL2N with
 * the support mean of the task), support class means, query shift eta = mean(support) - mean(query),
 * soft assignment u' = softmax_k(temp * -1/2 ||w_k/|w_k| - a/|a|||^2) of the support + shifted
 * queries a, rectified prototypes = u'-weighted means of the normalised a, prediction
 * u = softmax_k(temp * -1/2 ||p_k/|p_k| - z_q/|z_q|||^2) (args.temp of bdcspn.yaml).
 * Uses n_batches * tasks_per_batch tasks, n_query, n_class, n_support; iters is ignored.
 *   x_q device [T,Q,K] f32;  x_s device [T,S,K] f32;  y_s device [T,S] i64;
 *   prototypes device [T,K,K] out;  u device [T,Q,K] out;  preds device [T,Q] i32 out (argmax of u). */
size_t tclip_bdcspn_workspace_bytes(const tclip_problem* p);
int tclip_bdcspn_run(const tclip_problem* p, const float* x_q, const float* x_s, const int64_t* y_s, float temp,
                     int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                     size_t workspace_bytes, void* stream);

/* PADDLE on probability features (reference: src/methods/few_shot/paddle.py:94-219; feature
 * dimension = n_class).  Prototypes start as the class means of the support set; each iteration:
 * u = softmax_k(-1/2 ||w_k - z_q||^2 + lambd v_k / Q), v = log(mean_q u + eps) + 1,
 * w = (sum_q u z + support sums) / (sum_q u + support counts).  Uses n_batches * tasks_per_batch
 * tasks, n_query, n_class, n_support and iters; lambd is the method's float (paddle.yaml).
 *   x_q device [T,Q,K] f32;  x_s device [T,S,K] f32;  y_s device [T,S] i64;
 *   u device [T,Q,K] out;  v device [T,K] out;  w device [T,K,K] out;  preds device [T,Q] i32 out
 *   (argmax of u).  The criterion the reference logs is identically 0. */
size_t tclip_paddle_workspace_bytes(const tclip_problem* p);
int tclip_paddle_run(const tclip_problem* p, const float* x_q, const float* x_s, const int64_t* y_s, float lambd,
                     float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes,
                     void* stream);

/* PADDLE fed from the feature TABLES of the task-batch loop (see tclip_em_dirichlet_run_tasks for `src` and `y_s`): row r of
 * task t is table[idx[t,r]], on probability features with its columns permuted by src->cols[t].  The support rows are read in
 * place by the kernel that sums them per class - PADDLE reads them exactly once - and x_s [T,S,D] is never built; the query
 * rows, read in every iteration, are gathered once into the workspace (k_gather_task_rows), so the workspace is that of the
 * dense entry plus [T,Q,D] floats and does not depend on n_support.  Results are those of tclip_paddle_run /
 * tclip_paddle_visual_run on the materialised tensors, bit for bit.
 *   src->table_q device [rows_q, D] f32, src->q_idx device [T, Q] i64;  src->table_s device [rows_s, D] f32, src->s_idx device
 *   [T, S] i64;  D = n_class and src->cols device [T, K] i32 or NULL (probability features), D = dim and src->cols == NULL
 *   (visual features: the reference permutes no columns there, a non-NULL cols is TCLIP_ERR_ARG);
 *   y_s device [T, S] i64: the support labels after get_task's re-indexing (visual features: as they are), in 0..n_class-1;
 *   u, v, w, preds, lambd as for the dense entries (w device [T, K, D]).
 * Limits and checks are the dense entries': n_support >= 1, n_class in 2..1024, dim in 1..1024, null pointers
 * (TCLIP_ERR_ARG), workspace of tclip_paddle[_visual]_tasks_workspace_bytes bytes, 256-byte aligned (TCLIP_ERR_WORKSPACE; the
 * query returns 0 on bad input).  The entries do not know the tables' row counts: call tclip_check_task_indices on the index
 * tensors and cols first (the Python binding does). */
size_t tclip_paddle_tasks_workspace_bytes(const tclip_problem* p);
int tclip_paddle_run_tasks(const tclip_problem* p, const tclip_task_source* src, const int64_t* y_s, float lambd,
                           float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes, void* stream);
size_t tclip_paddle_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_paddle_visual_run_tasks(const tclip_problem* p, int32_t dim, const tclip_task_source* src, const int64_t* y_s,
                                  float lambd, float* u, float* v, float* w, int32_t* preds,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* BD-CSPN and LAPLACIAN_SHOT fed from the feature TABLES of the task-batch loop (`src` and `y_s` exactly as for
 * tclip_paddle_run_tasks): row r of task t is table[idx[t,r]], on probability features with its columns permuted by
 * src->cols[t].  In both methods the first kernels that touch a task row normalise it into the workspace (BD-CSPN's CL2N
 * also takes the support's column means first); those kernels read the table rows in place, so neither x_s [T,S,D] nor x_q
 * [T,Q,D] is ever built.  One output row is computed from one source row by the same operations in the same order: the
 * results are those of the dense entries on the materialised tensors, bit for bit.
 *   src->table_q device [rows_q, D] f32, src->q_idx device [T, Q] i64;  src->table_s device [rows_s, D] f32, src->s_idx device
 *   [T, S] i64;  D = n_class and src->cols device [T, K] i32 or NULL (probability features), D = dim and src->cols == NULL
 *   (visual features: a non-NULL cols is TCLIP_ERR_ARG);  y_s device [T, S] i64 in 0..n_class-1 (after get_task's re-indexing
 *   on probability features);  the other arguments and the outputs as for tclip_bdcspn[_visual]_run /
 *   tclip_laplacian_shot[_visual]_run.
 * Workspace.  BD-CSPN: the dense entry's regions, except that the normalised support rows zs [T,S,D] have none of their own:
 * they lie at the start of the logit region, sized max(T (S+Q) K, T S D) floats (zs is dead before the logits are first
 * written) - the dense workspace minus the smaller of the two.  LAPLACIAN_SHOT: the dense entry's workspace.
 * Limits and checks are the dense entries', all before any launch: n_support >= 1, n_class in 2..1024, dim in 1..1024,
 * norm_type, knn, null pointers - members of src included - (TCLIP_ERR_ARG), workspace of the matching *_tasks_workspace_bytes
 * query, 256-byte aligned (TCLIP_ERR_WORKSPACE; the queries return 0 on bad input).  The entries do not know the tables' row
 * counts: call tclip_check_task_indices on the index tensors and cols first (the Python binding does). */
size_t tclip_bdcspn_tasks_workspace_bytes(const tclip_problem* p);
int tclip_bdcspn_run_tasks(const tclip_problem* p, const tclip_task_source* src, const int64_t* y_s, float temp, int32_t norm_type,
                           float* prototypes, float* u, int32_t* preds, void* workspace, size_t workspace_bytes, void* stream);
size_t tclip_bdcspn_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_bdcspn_visual_run_tasks(const tclip_problem* p, int32_t dim, const tclip_task_source* src, const int64_t* y_s, float temp,
                                  int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                                  size_t workspace_bytes, void* stream);
size_t tclip_laplacian_shot_tasks_workspace_bytes(const tclip_problem* p);
int tclip_laplacian_shot_run_tasks(const tclip_problem* p, const tclip_task_source* src, const int64_t* y_s, int32_t knn, double lmd,
                                   int32_t norm_type, float* unary, int32_t* neighbours, int32_t* preds_iter, double* energies,
                                   void* workspace, size_t workspace_bytes, void* stream);
size_t tclip_laplacian_shot_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_laplacian_shot_visual_run_tasks(const tclip_problem* p, int32_t dim, const tclip_task_source* src, const int64_t* y_s,
                                          int32_t knn, double lmd, int32_t norm_type, float* unary, int32_t* neighbours,
                                          int32_t* preds_iter, double* energies, void* workspace, size_t workspace_bytes, void* stream);

/* ALPHA_TIM on probability features (reference: src/methods/few_shot/tim.py:192-322; feature dimension =
 * n_class).  Weights start as the class means of the support set; each of `iters` iterations takes one
 * torch.optim.Adam step (betas 0.9/0.999, eps 1e-8) of size lr on
 *   loss_weights[0] * CE(support) - (loss_weights[1] * H(mean_q p_q) - loss_weights[2] * mean_q H(p_q)),
 * p = softmax_k(temp * (x.w_k - |w_k|^2/2 - |x|^2/2)), every entropy either Shannon or the alpha-entropy of
 * order alpha_value (tim.py:276-305), with the gradient in closed form instead of autograd.  The reference's
 * matmuls and backward pass have no fixed operation order, so this entry is pinned to the reference within a
 * float tolerance (tests/test_alpha_tim.py), not bit for bit.  Uses n_batches, tasks_per_batch, n_query,
 * n_class, n_support, iters (>= 1).
 *   x_q device [T,Q,K] f32;  x_s device [T,S,K] f32;  y_s device [T,S] i64;
 *   weights device [T,K,K] out (after the last step);  logits_q device [T,Q,K] out and preds device [T,Q] i32
 *   out: the query logits of the LAST iteration's forward pass and their argmax, which is what the reference
 *   scores (tim.py:321);  criterions device [n_batches, iters] out: mean_{task,class} ||w_old - w|| per step. */
#define TCLIP_TIM_SHANNON 0
#define TCLIP_TIM_ALPHA 1
typedef struct tclip_tim_params {
    double lr;               /* lr_alpha_tim */
    float temp;              /* args.temp */
    float alpha_value;       /* order of the alpha-entropies */
    float loss_weights[3];   /* [cross-entropy, marginal entropy, conditional entropy] */
    int32_t entropies[3];    /* TCLIP_TIM_SHANNON / TCLIP_TIM_ALPHA for the same three terms */
} tclip_tim_params;
size_t tclip_alpha_tim_workspace_bytes(const tclip_problem* p);
int tclip_alpha_tim_run(const tclip_problem* p, const tclip_tim_params* prm, const float* x_q, const float* x_s,
                        const int64_t* y_s, float* weights, float* logits_q, int32_t* preds, float* criterions,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ALPHA_TIM on feature rows of `dim` elements, dim independent of n_class (visual features, use_softmax_feature == False; the
 * reference's class never reads that switch and normalises nothing): the loss, the Adam step, the kernels and the per-batch
 * criterion of tclip_alpha_tim_run with W [K, dim] instead of [K, K].  dim in 1..1024, n_class in 2..1024, n_support >= 1,
 * iters >= 1; at dim == n_class the results are those of tclip_alpha_tim_run, bit for bit.  Pinned to reference-made fixtures
 * within bounds derived from the reference's own fp32-against-fp64 gap (tests/test_gpu_visual_alpha_tim.py).
 *   x_q device [T,Q,dim] f32;  x_s device [T,S,dim] f32;  y_s device [T,S] i64 in 0..n_class-1 (a label outside that range is
 *   never used as an index and joins no class; callers reject such labels);
 *   weights device [T,K,dim] out;  logits_q device [T,Q,K] out, preds device [T,Q] i32 out (last iteration's forward pass);
 *   criterions device [n_batches, iters] out;  workspace: tclip_alpha_tim_visual_workspace_bytes(p, dim) bytes, 256-byte
 *   aligned (0 on bad input). */
size_t tclip_alpha_tim_visual_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_alpha_tim_visual_run(const tclip_problem* p, int32_t dim, const tclip_tim_params* prm, const float* x_q /*[T,Q,dim]*/,
                               const float* x_s /*[T,S,dim]*/, const int64_t* y_s /*[T,S]*/, float* weights /*[T,K,dim]*/,
                               float* logits_q /*[T,Q,K]*/, int32_t* preds /*[T,Q]*/, float* criterions /*[n_batches,iters]*/,
                               void* workspace, size_t workspace_bytes, void* stream);

/* TIM_GD (reference: src/methods/few_shot/tim.py:90-189) on feature rows of `dim` elements, dim independent of n_class:
 * dim == n_class is the probability-feature case, anything else in 1..1024 the visual one (use_softmax_feature == False; the
 * class never reads that switch and normalises nothing).  It is ALPHA_TIM with all three entropies Shannon and
 *   - the marginal entropy -(m * log(m + 1e-12)).sum() of m = mean_q p_q (tim.py:171-172; ALPHA_TIM's has no 1e-12),
 *   - the criterion per TASK: mean_class ||w_old - w|| (tim.py:181),
 *   - lr = args.lr_tim, temp and loss_weights [cross-entropy, marginal entropy, conditional entropy] passed directly.
 * Same Adam step, same closed-form gradient and the same GEMM kernels as ALPHA_TIM; like it, the entry has no bit-level
 * target (the reference's matmuls and backward pass have no fixed operation order) and is pinned to reference-made fixtures
 * within bounds derived from the reference's own fp32-against-fp64 gap (tests/test_gpu_tim_gd.py).  Uses n_batches,
 * tasks_per_batch, n_query, n_class, n_support (>= 1), iters (>= 1); T = n_batches * tasks_per_batch.
 *   x_q device [T,Q,dim] f32;  x_s device [T,S,dim] f32;  y_s device [T,S] i64 in 0..n_class-1 (a label outside that range is
 *   never used as an index; callers reject such labels);
 *   weights device [T,K,dim] out (after the last step);  logits_q device [T,Q,K] out and preds device [T,Q] i32 out: the query
 *   logits of the LAST iteration's forward pass and their argmax (tim.py:189);  criterions device [iters, T] out.
 *   workspace: tclip_tim_gd_workspace_bytes(p, dim) bytes, 256-byte aligned (0 on bad input). */
size_t tclip_tim_gd_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_tim_gd_run(const tclip_problem* p, int32_t dim, double lr, float temp, const float loss_weights[3],
                     const float* x_q /*[T,Q,dim]*/, const float* x_s /*[T,S,dim]*/, const int64_t* y_s /*[T,S]*/,
                     float* weights /*[T,K,dim]*/, float* logits_q /*[T,Q,K]*/, int32_t* preds /*[T,Q]*/,
                     float* criterions /*[iters,T]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ALPHA_TIM and TIM_GD fed from the feature TABLES of the task-batch loop (`src` and `y_s` exactly as for
 * tclip_paddle_run_tasks): row r of task t is table[idx[t,r]], on probability features with its columns permuted by
 * src->cols[t].  Unlike the other methods these two read their task rows in EVERY Adam step (both GEMMs), not once: the row
 * norms, the GEMMs and the class sums of the initial weights fetch the table rows in place, step after step, and neither
 * x_s [T,S,D] nor x_q [T,Q,D] is ever built.  Every thread loads the value the dense kernels load at the same position of the
 * same sum: the outputs are those of the dense entries on the materialised tensors, bit for bit.  What the indirection costs in
 * time is measured in DESIGN.md 8j, not promised.
 *   src->table_q device [rows_q, D] f32, src->q_idx device [T, Q] i64;  src->table_s device [rows_s, D] f32, src->s_idx device
 *   [T, S] i64;  src->cols device [T, D] i32 or NULL where D == n_class (tclip_alpha_tim_run_tasks, and tclip_tim_gd_run_tasks
 *   with dim == n_class), NULL otherwise (a non-NULL cols on tclip_alpha_tim_visual_run_tasks, or on tclip_tim_gd_run_tasks with
 *   dim != n_class, is TCLIP_ERR_ARG);  y_s device [T, S] i64 in 0..n_class-1 (after get_task's re-indexing on probability
 *   features);  the other arguments and the outputs as for the dense entries.
 * Workspace: the dense entries' (each *_tasks_workspace_bytes returns what its dense query returns), 256-byte aligned.
 * Limits and checks are the dense entries', all before any launch; a NULL src or a NULL member of it other than cols is
 * TCLIP_ERR_ARG.  The entries do not know the tables' row counts: call tclip_check_task_indices on the index tensors and cols
 * first (the Python binding does).  Interior GEMM tiles keep their 128-bit loads when there is no cols, D is a multiple of 4 and
 * both table pointers are 16-byte aligned; any other table is read element by element, with the same result. */
size_t tclip_alpha_tim_tasks_workspace_bytes(const tclip_problem* p);
int tclip_alpha_tim_run_tasks(const tclip_problem* p, const tclip_tim_params* prm, const tclip_task_source* src, const int64_t* y_s,
                              float* weights, float* logits_q, int32_t* preds, float* criterions, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t tclip_alpha_tim_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_alpha_tim_visual_run_tasks(const tclip_problem* p, int32_t dim, const tclip_tim_params* prm, const tclip_task_source* src,
                                     const int64_t* y_s, float* weights, float* logits_q, int32_t* preds, float* criterions,
                                     void* workspace, size_t workspace_bytes, void* stream);
size_t tclip_tim_gd_tasks_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_tim_gd_run_tasks(const tclip_problem* p, int32_t dim, double lr, float temp, const float loss_weights[3],
                           const tclip_task_source* src, const int64_t* y_s, float* weights, float* logits_q, int32_t* preds,
                           float* criterions, void* workspace, size_t workspace_bytes, void* stream);

/* LAPLACIAN_SHOT on probability features (reference: src/methods/few_shot/laplacian_shot.py:66-249; feature
 * dimension = n_class).  Rows L2-normalised (norm_type 1) or left as they are (0), prototypes = support class
 * means, unary = squared distances query-prototype, a kNN graph over the queries of a task (the knn-1 nearest
 * OTHER queries of each query, as `knnind[:, 1:]`), then `iters` bound updates Y <- softmax_k(-unary + lmd W Y)
 * with the reference's energy and its freeze rule (:162-171).  Host numpy/scipy/sklearn code in the reference,
 * one workgroup per task here; pinned to reference-made fixtures within a tolerance (tests/test_laplacian_shot.py).
 * Uses n_batches * tasks_per_batch tasks, n_query (<= 1024), n_class, n_support, iters (>= 1).
 *   x_q device [T,Q,K] f32;  x_s device [T,S,K] f32;  y_s device [T,S] i64;
 *   unary device [T,Q,K] f32 out;  neighbours device [T,Q,knn-1] i32 out (nearest first);
 *   preds_iter device [T,iters,Q] i32 out (the assignment after every update; the last one is the prediction);
 *   energies device [T,iters] f64 out. */
size_t tclip_laplacian_shot_workspace_bytes(const tclip_problem* p);
int tclip_laplacian_shot_run(const tclip_problem* p, const float* x_q, const float* x_s, const int64_t* y_s, int32_t knn,
                             double lmd, int32_t norm_type, float* unary, int32_t* neighbours, int32_t* preds_iter,
                             double* energies, void* workspace, size_t workspace_bytes, void* stream);

/* LAPLACIAN_SHOT on feature rows of `dim` elements, dim independent of n_class (visual features; the reference's class never
 * reads use_softmax_feature: it normalises rows, takes class means, squared distances and a kNN graph, all defined for any row
 * length).  Rows, prototypes [T,K,dim] and the kNN distances live in dim, unary, Y and the bound updates in n_class.  The
 * queries' pairwise squared distances come from a kernel of their own (k_lshot_pairdist: a [T,Q,Q] fp64 table in the
 * workspace, many workgroups per task), the selection, the updates and the freeze rule are tclip_laplacian_shot_run's.
 * dim in 1..1024, n_class in 2..1024, n_support >= 1, n_query <= 1024, knn in 2..n_query, norm_type 0 or 1, iters >= 1; at
 * dim == n_class the results are those of tclip_laplacian_shot_run, bit for bit.
 *   x_q device [T,Q,dim] f32;  x_s device [T,S,dim] f32;  y_s device [T,S] i64 in 0..n_class-1 (a label outside that range is
 *   never used as an index and joins no class; callers reject such labels);
 *   unary device [T,Q,K] f32 out;  neighbours device [T,Q,knn-1] i32 out;  preds_iter device [T,iters,Q] i32 out;
 *   energies device [T,iters] f64 out;  workspace: tclip_laplacian_shot_visual_workspace_bytes(p, dim) bytes, 256-byte aligned
 *   (0 on bad input). */
size_t tclip_laplacian_shot_visual_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_laplacian_shot_visual_run(const tclip_problem* p, int32_t dim, const float* x_q /*[T,Q,dim]*/, const float* x_s /*[T,S,dim]*/,
                                    const int64_t* y_s /*[T,S]*/, int32_t knn, double lmd, int32_t norm_type,
                                    float* unary /*[T,Q,K]*/, int32_t* neighbours /*[T,Q,knn-1]*/, int32_t* preds_iter /*[T,iters,Q]*/,
                                    double* energies /*[T,iters]*/, void* workspace, size_t workspace_bytes, void* stream);

/* Inductive zero-shot CLIP on probability features (reference: src/methods/zero_shot/inductive_clip.py:45-49,
 * 112-126): the prediction is the arg-max of each query's probability vector, no adaptation.
 *   x device [n_rows, n_class] f32;  labels device [n_rows] i32 out (first maximum, as torch.argmax). */
int tclip_argmax_rows(const float* x, int64_t n_rows, int32_t n_class, int32_t* labels, void* stream);

/* Probability features from visual embeddings (reference: extract_features_softmax,
 * src/utils.py:287-290): out[n,:] = softmax_k(T * (visual[n]/||visual[n]||) . text[k]).
 *   visual device [n_rows, dim] f32 (any norm), text device [n_class, dim] f32 (unit-norm rows, as
 *   clip_weights returns them, src/utils.py:363-377), out device [n_rows, n_class] f32.
 *   text may start at any float: it is read 16 bytes at a time only when dim % 4 == 0 and text is 16-byte aligned, and the
 *   result has the same bits either way.  dim + n_class <= 15000 (TCLIP_ERR_ARG beyond); n_rows = 0 is TCLIP_OK.
 * This is the only reference-consistent way to feed visual features to EM-Dirichlet (which raises
 * ValueError on features outside the simplex, em_dirichlet.py:204-208). */
int tclip_probability_features(const float* visual, const float* text, int64_t n_rows, int32_t dim, int32_t n_class,
                               float temperature, float* out, void* stream);

/* Zero-shot k-means on VISUAL features (the reference's use_softmax_feature == False: raw CLIP image embeddings, e.g.
 * <split>_visual_<backbone>.plk), reference src/methods/zero_shot/soft_kmeans.py:126-220, hard_kmeans.py:137-204,
 * em_gaussian.py:117-229.  The clustering runs in the D-dimensional embedding space, dim = D independent of K = p->n_class:
 * centroids are [T, K, D], the squared distances sum over D in torch's last-dim order (any D in 1..1024) and the centroid
 * statistics over the queries in torch's outer-sum order of K*D columns, so that a run from the reference's own u0 gives its
 * bits.  The loop starts from a given responsibility tensor u0 instead of building it from text prompts: the reference's
 * initialisation u0[t] = softmax_k(T * (x_q[t]/||x_q[t]||) . text_k) is a GEMM (tclip_visual_init).
 *   method TCLIP_VISUAL_SOFT_KMEANS: w_init, then iters x (w_update keeping empty clusters, u = softmax_k(T * -1/2 ||w_k - z||^2))
 *   method TCLIP_VISUAL_HARD_KMEANS: iters x (w = member means with 0 for empty clusters, u = one_hot(argmin_k softmax_k
 *          ||w_k - z||^2)); criterions as tclip_hard_kmeans_run (the reference logs each value twice)
 *   method TCLIP_VISUAL_EM_GAUSSIAN: SOFT_KMEANS with the term lambd v_k / Q in the softmax, v = log(mean_q u + eps) + 1
 *          (p->lambd: int(K/5) * n_query)
 * Uses n_batches, tasks_per_batch, n_query, n_class, iters (n_support must be 0; the other fields are ignored).
 *   x_q device [T,Q,D] f32 raw embeddings (not normalised, as the reference's loop reads them);  u0 device [T,Q,K] f32;
 *   u device [T,Q,K] out (one-hot for HARD_KMEANS);  w device [T,K,D] out;  preds device [T,Q] i32 out (first maximum of u;
 *   HARD_KMEANS: the first minimum of its softmax);  v device [T,K] out (EM_GAUSSIAN only, NULL otherwise);
 *   criterions device [n_batches, iters] out (HARD_KMEANS only, NULL otherwise).  SOFT_KMEANS and EM_GAUSSIAN log 0.
 *   workspace: tclip_visual_workspace_bytes(p, dim) bytes, 256-byte aligned (0 on bad input). */
#define TCLIP_VISUAL_SOFT_KMEANS 0
#define TCLIP_VISUAL_HARD_KMEANS 1
#define TCLIP_VISUAL_EM_GAUSSIAN 2
size_t tclip_visual_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_kmeans_visual_run(const tclip_problem* p, int32_t dim, int32_t method, const float* x_q, const float* u0,
                            float temperature, float* u, float* v, float* w, int32_t* preds, float* criterions, void* workspace,
                            size_t workspace_bytes, void* stream);

/* EM_GAUSSIAN_COV on VISUAL features (use_softmax_feature == False; reference src/methods/zero_shot/em_gaussian_cov.py:106-257,
 * the text-prompt initialisation of :215-227 given as u0, see tclip_visual_init): tclip_em_gaussian_cov_run's op sequence in the
 * D-dimensional embedding space, dim = D independent of K = p->n_class.  Centroids w and inverse variances s are [T, K, D]:
 *   s[t,k,d] = sum_q u / max(sum_q (w[t,k,d] - z[t,q,d])^2 u[t,q,k], eps)      (the sum over q in torch's outer-sum order of K*D columns),
 *   logit[t,q,k] = -1/2 sum_d (w - z)^2 s + 1/2 sum_d log(s + eps)             (both sums in torch's last-dim order, any D in 1..1024),
 *   u = softmax_k(logit + lambd v / Q), v = log(mean_q u + eps) + 1; clusters with sum_q u <= eps keep their w and s.
 * A run from the reference's own u0 gives its bits.  Uses n_batches, tasks_per_batch, n_query, n_class (2..1024), iters, lambd
 * (int(K/5) * n_query); n_support must be 0 and dim in 1..1024, anything else is TCLIP_ERR_ARG before any launch.
 *   x_q device [T,Q,D] f32 raw embeddings;  u0 device [T,Q,K] f32;  u device [T,Q,K] out;  v device [T,K] out;
 *   w, s device [T,K,D] out;  preds device [T,Q] i32 out (first maximum of u);
 *   workspace: tclip_em_gaussian_cov_visual_workspace_bytes(p, dim) bytes, 256-byte aligned (0 on bad input; a short or
 *   misaligned one is TCLIP_ERR_WORKSPACE).  Accuracy tail: tclip_cluster_prototypes_visual and what follows it. */
size_t tclip_em_gaussian_cov_visual_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_em_gaussian_cov_visual_run(const tclip_problem* p, int32_t dim, const float* x_q /*[T,Q,dim]*/, const float* u0 /*[T,Q,K]*/,
                                     float* u /*[T,Q,K]*/, float* v /*[T,K]*/, float* w /*[T,K,dim]*/, float* s /*[T,K,dim]*/,
                                     int32_t* preds /*[T,Q]*/, void* workspace, size_t workspace_bytes, void* stream);

/* Accuracy tail of the visual k-means methods, device half: tclip_cluster_prototypes for D-dim features
 * (soft_kmeans.py:36-44): the clusters present in `preds` in first-appearance order and the mean raw embedding of each.
 *   x_q device [T,Q,dim] f32, preds device [T,Q] i32
 *   n_clusters device [T] i32 out; cluster_ids device [T, Cmax] i32 out (-1 padded); prototypes device [T, Cmax, dim] f32 out
 *   (rows beyond a task's cluster count are not written), Cmax = min(Q, K).  Needs no workspace.
 * The reference then scores softmax_k(T * (p/||p||) . text_k) of each prototype (tclip_probability_features) and matches
 * those rows to classes (tclip_match_clusters_host_strided). */
int tclip_cluster_prototypes_visual(int32_t n_task, int32_t n_query, int32_t n_class, int32_t dim, const float* x_q,
                                    const int32_t* preds, int32_t* n_clusters, int32_t* cluster_ids, float* prototypes, void* stream);

/* The visual k-means initialisation (soft_kmeans.py:185-197, also CLIP's u, inductive_clip.py:115-124):
 * out[n,:] = softmax_k(T * ((visual[n]/||visual[n]||) . text[k])) - the scale AFTER the dot product, where
 * tclip_probability_features scales before it.  Same arguments and limits as tclip_probability_features. */
int tclip_visual_init(const float* visual, const float* text, int64_t n_rows, int32_t dim, int32_t n_class,
                      float temperature, float* out, void* stream);

/* Few-shot PADDLE and BD-CSPN on VISUAL features (use_softmax_feature == False; reference src/methods/few_shot/paddle.py:94-219,
 * bdcspn.py:42-200): tclip_paddle_run / tclip_bdcspn_run with feature rows of `dim` elements, dim independent of n_class.
 * PADDLE needs no text features: the reference's text-prompt u is overwritten by the first u_update before anything reads it
 * (paddle.py:183-203), and w starts from the support class means.
 *   x_q device [T, n_query, dim] f32, x_s device [T, n_support, dim] f32, y_s device [T, n_support] int64 in 0..n_class-1 (a
 *   label outside that range is never used as an index: its row joins no class; callers reject such labels),
 *   T = n_batches * tasks_per_batch.
 *   PADDLE: u [T, n_query, n_class], v [T, n_class], w [T, n_class, dim] the centroids, preds [T, n_query] int32 = argmax_k u;
 *   p->iters iterations, lambd the method's float (paddle.yaml).
 *   BD-CSPN: prototypes [T, n_class, dim] the rectified prototypes, u [T, n_query, n_class], preds; temp and norm_type
 *   (0 UN, 1 L2N, 2 CL2N) as tclip_bdcspn_run.
 *   Limits: dim in 1..1024, n_class in 2..1024, n_support >= 1; anything else is TCLIP_ERR_ARG.
 *   workspace: tclip_*_visual_workspace_bytes(p, dim) bytes, 256-byte aligned (0 on bad input). */
size_t tclip_paddle_visual_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_paddle_visual_run(const tclip_problem* p, int32_t dim, const float* x_q, const float* x_s, const int64_t* y_s,
                            float lambd, float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes,
                            void* stream);
size_t tclip_bdcspn_visual_workspace_bytes(const tclip_problem* p, int32_t dim);
int tclip_bdcspn_visual_run(const tclip_problem* p, int32_t dim, const float* x_q, const float* x_s, const int64_t* y_s, float temp,
                            int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Optional instrumentation used by bench.py (thread-local, off by default).  While enabled,
 * every launch of a live-row majorize-minimize kernel (k_mm_live, k_mm_reuse or k_mm_split, the dominant kernels; the
 * dead-row launches and the probes are not covered) issued by the tclip_em_dirichlet_run* entries on this thread is
 * bracketed by HIP events on the stream it is launched
 * on (independent batches run on a few internal streams, so launches overlap) and the
 * element-updates it executes are counted on the device.  tclip_profile_collect synchronises the device and returns, since the last collection:
 * the time during which at least one such launch was running (union of the intervals), the sum
 * of the individual launch durations, the number of launches and the element-update count. */
int tclip_profile_enable(int on);
int tclip_profile_collect(double* mm_busy_ms, double* mm_launch_ms_sum, int64_t* mm_launches,
                          int64_t* element_updates);
/* The same four figures of the LAST tclip_profile_collect of this thread per kernel: index 0 = k_mm_live plus k_mm_reuse (the
 * first outer iteration, and every launch of row lengths without a split instantiation), 1 = k_mm_split.  Every argument
 * points to two values. */
int tclip_profile_last_kernels(double* busy_ms, double* launch_ms_sum, int64_t* launches, int64_t* element_updates);
/* k_mm_split keeps the placement of a wavefront's elements in its three class queues from one MM iteration to the next and
 * sorts anew only when an element has left its class: the wavefront-iterations the kernel ran in the window of the LAST
 * tclip_profile_collect of this thread, and how many of them ran the full placement (the first of every launch does). */
int tclip_profile_last_split_sorts(int64_t* wave_iterations, int64_t* sorts);
/* Test hook: 0 makes k_mm_split sort its class queues in every MM iteration (what rounds 3-4 did), non-zero restores the default
 * (the placement of an iteration is kept for the next one and checked by the dense passes).  Process-wide; results do not
 * depend on it (tests/test_gpu_round5.py::test_kept_placement_is_invisible). */
int tclip_debug_set_split_keep_placement(int32_t on);

/* Dead rows are spared the rest of their schedule once a limit-cycle probe (run after each of the
 * first `chunks` 50-iteration chunks) finds them on a cycle of the fp32 map - an exact shortcut.
 * For tests: 0 disables the probe (every dead row iterates its whole schedule once), negative
 * restores the default.  Process-wide; results do not depend on it. */
int tclip_debug_set_probe_chunks(int32_t chunks);

/* Rows that have just died run only their first `iterations` MM iterations (default 12) before an early probe looks for
 * the limit cycle from there on (further snapshots 8 and 32 iterations later find rows that were still approaching their cycle);
 * rows it cannot finish take the path above from the start.  For tests: 0 disables the early probe (the path above for
 * every dead row), negative restores the default, more than 18 is refused (TCLIP_ERR_ARG).  Also off while
 * tclip_debug_set_probe_chunks(0) is in force.  Process-wide; results do not depend on it. */
int tclip_debug_set_dead_head(int32_t iterations);

/* Rows of up to 256 elements are spread over 16 lanes in the MM kernels (4 rows per wavefront), longer ones
 * over 32.  For tests: 0 forces the 32-lane layout for every row length, negative restores the default rule.
 * Process-wide; results do not depend on it. */
int tclip_debug_set_rowset_min_rows(int32_t rows);

/* From the second outer iteration on the live rows run through the class-split MM kernel (k_mm_split: every element
 * executes only what its value class a+1 < 2.3 / [2.3, 10) / >= 10 needs).  For tests: 0 never uses it, 1 uses it from
 * the first iteration on, 100 + n from outer iteration n on, negative restores the default rule (n = 1).  Process-wide;
 * results do not depend on it. */
int tclip_debug_set_mm_split(int32_t mode);

/* In the first outer iteration the live rows' MM iterations from 51 on run through k_mm_reuse: digamma and lgamma are
 * evaluated at fl(a + 1), and an element whose fl(a + 1) the last iteration left unchanged keeps both values (two LDS words
 * per element) instead of evaluating them again.  Only under tclip_debug_set_mm_split's default rule.  For tests: 0 runs
 * k_mm_live for the whole first outer iteration, 1 is the default, 2 is the default with the kernel's index queue cut to 64
 * entries (its overflow path on small problems); anything else is refused (TCLIP_ERR_ARG).  Process-wide; results do not
 * depend on it. */
int tclip_debug_set_mm_reuse(int32_t mode);
/* k_mm_reuse in the window of the LAST tclip_profile_collect of this thread: out[0] = entries whose special functions it
 * evaluated, out[1] = element-updates it executed (these are also part of tclip_profile_last_kernels' k_mm_live figures). */
int tclip_profile_last_mm_reuse(uint64_t out[2]);

/* The MM kernels are also compiled with the row length as a constant for the class counts of the reference's datasets that
 * BASELINE.json runs (1000, 397, 100): same layout and operations as the run-time-K kernel of the row length's bucket.  For
 * tests: 0 launches the run-time-K kernels for every row length, anything else restores the default.  Process-wide; results
 * do not depend on it. */
int tclip_debug_set_fixed_k_kernels(int32_t on);

/* The squared distances of the k-means family (SOFT/HARD_KMEANS, EM_GAUSSIAN, PADDLE, BD-CSPN) and KL_KMEANS's divergences run one
 * lane per class on a 64-centroid tile staged in LDS for rows of 32 .. 511 elements (k_kmeans_logits_tile, k_kl_divergences_tile),
 * 32 lanes per class otherwise; the centroid statistics of 75-query problems stage 64 feature columns per block (k_mstats_cols75).  For
 * tests: 0 uses the round-3 kernels for every shape, negative restores the default rule.  Process-wide; results do not
 * depend on it. */
int tclip_debug_set_kmeans_tile(int32_t mode);

/* Device self-test (used by tests/test_gpu_primitives.py).  out host [14]:
 *   [0] 1/x: fast exact reciprocal vs IEEE quotient, every float of a binade at 3 exponents
 *   [1] a/b: 2^29 operand pairs            [2] fused digamma(a+1), digamma of row sums vs generic
 *   [3] fused lgamma(a+1) vs generic        [4] whole MM update, branch-free vs generic (2^24 each)
 *   [5] 1/x with two correction steps (informational)
 *   [6..13] 64-bit checksums of the restated library routines (digamma, lgamma, sqrt, exp, log,
 *           fused psi, fused lgamma, digamma_pos) over the argument streams of
 *           csrc/tclip_selftest_inputs.h; oracle/mathcheck.cpp computes the host values.
 * [0]..[4] must be 0.  Allocates (and frees) 112 bytes of device memory for the counters. */
int tclip_selftest_primitives(uint64_t* mismatches);

/* Value sweeps: the four tunable few-shot methods (PADDLE: lambd, BD-CSPN: temp, LAPLACIAN_SHOT: lmd, ALPHA_TIM: alpha_value)
 * solved for a LIST of values on the same tasks in one call - what the reference's scripts/opt_parameters.sh does with one
 * process per value.  `src`, `y_s` and every argument not named here are those of the method's *_run_tasks entry.
 *   dim       0: probability features (rows of n_class elements, src->cols allowed) - the problem of <method>_run_tasks;
 *             1..1024: visual features (rows of dim elements, src->cols must be NULL) - that of <method>_visual_run_tasks
 *   values    HOST array [n_values] of finite doubles, n_values >= 1; value i is converted as the single-value entry converts
 *             its scalar ((float) for lambd, temp and alpha_value; lmd stays double).  Read before the call returns.
 * Outputs that depend on the value are value-major, [n_values] in front of the single-value entry's layout; LAPLACIAN_SHOT's
 * unary and neighbours do not depend on it and are written once:
 *   PADDLE          u [P,T,Q,K], v [P,T,K], w [P,T,K,D], preds [P,T,Q]
 *   BD-CSPN         prototypes [P,T,K,D], u [P,T,Q,K], preds [P,T,Q]
 *   LAPLACIAN_SHOT  unary [T,Q,K], neighbours [T,Q,knn-1], preds_iter [P,T,iters,Q], energies [P,T,iters]
 *   ALPHA_TIM       weights [P,T,K,D], logits_q [P,T,Q,K], preds [P,T,Q], criterions [P,B,iters]; prm->alpha_value is not read
 *                   (each value must differ from 1 where an entropy is TCLIP_TIM_ALPHA)
 * Slice i of every such output holds the bits the single-value entry returns for values[i] on the same source; repeated values
 * give repeated slices.  What does not read the value runs once per task: PADDLE's support class sums; BD-CSPN up to and
 * including its augmented set; LAPLACIAN_SHOT's normalisation, prototypes, unary term and kNN graph.  PADDLE and BD-CSPN then
 * run their values one after the other on the stream, reusing one value's scratch; LAPLACIAN_SHOT runs its updates on a grid of
 * (task, value); ALPHA_TIM runs its Adam loop over n_values * T solves in one set of launches per step, solve p T + t reading
 * the rows of task t in place.
 * Limits and checks are the single-value entry's, all before any launch, and: dim outside 0..1024, n_values < 1, a NULL or
 * non-finite value, n_values * T > 65535 (TCLIP_ERR_ARG).  Workspace: <entry>_workspace_bytes(p, dim, n_values) bytes (0 on
 * bad input), 256-byte aligned; it grows with n_values for LAPLACIAN_SHOT (the fp64 assignments, 16 T Q K bytes per value)
 * and ALPHA_TIM (everything but the support class sums), not for PADDLE and BD-CSPN. */
size_t tclip_paddle_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values);
int tclip_paddle_sweep_tasks(const tclip_problem* p, int32_t dim, const tclip_task_source* src, const int64_t* y_s, const double* values,
                             int32_t n_values, float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes,
                             void* stream);
size_t tclip_bdcspn_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values);
int tclip_bdcspn_sweep_tasks(const tclip_problem* p, int32_t dim, const tclip_task_source* src, const int64_t* y_s, const double* values,
                             int32_t n_values, int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                             size_t workspace_bytes, void* stream);
size_t tclip_laplacian_shot_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values);
int tclip_laplacian_shot_sweep_tasks(const tclip_problem* p, int32_t dim, const tclip_task_source* src, const int64_t* y_s, int32_t knn,
                                     const double* values, int32_t n_values, int32_t norm_type, float* unary, int32_t* neighbours,
                                     int32_t* preds_iter, double* energies, void* workspace, size_t workspace_bytes, void* stream);
size_t tclip_alpha_tim_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values);
int tclip_alpha_tim_sweep_tasks(const tclip_problem* p, int32_t dim, const tclip_tim_params* prm, const tclip_task_source* src,
                                const int64_t* y_s, const double* values, int32_t n_values, float* weights, float* logits_q,
                                int32_t* preds, float* criterions, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TCLIP_H */
