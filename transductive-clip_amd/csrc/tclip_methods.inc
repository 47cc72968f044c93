// Host drivers of the k-means family and of few-shot PADDLE / BD-CSPN, one per algorithm for both feature kinds: included
// last by tclip_kernels.hip, after the kernels and launchers of tclip_visual.inc / tclip_visual_fs.inc.
//
// Probability features (the reference's use_softmax_feature == True) have rows of K = n_class elements; visual features (raw
// CLIP embeddings) rows of D elements, D independent of K.  The op sequences are the same; a FeatureSpace picks the
// launchers whose work depends on the row length (three, and EM_GAUSSIAN_COV's two), everything else ([T, Q, K] / [T, K]
// tensors: the softmax, the cluster sizes, v, the first-minimum one-hot, the criterion) is shared as it stands.  KL_KMEANS
// exists on probability features only and keeps its own loop below.  EM-Dirichlet does not come through here.
// PADDLE and BD-CSPN also run from the feature tables (tclip_*_run_tasks): PADDLE's class sums and BD-CSPN's normalisations
// read the task rows in place through a RowSrc.
// Host side, in this order: the FeatureSpace, one layout function per method (typed views over the one WsCursor), the loops,
// then one entry function per method for all its call forms (kmeans_entry, em_gaussian_cov_entry, paddle_entry, bdcspn_entry;
// the form as a Rows of tclip_tim.inc, the checks in the one order of DESIGN.md, "The method host drivers") and the extern "C"
// functions, each an adaptor call and that one call.

namespace tclip {

// which rows the centroid statistics write and what they divide by (the values are k_vis_mstats's modes)
enum class Mstats {
    LiveOnly = 0,        // quotient by clamp(cs, eps); rows `live` does not mark keep their value   (SOFT_KMEANS, EM_GAUSSIAN)
    HardZeroDead = 1,    // the same quotient; rows that are not live get it times 0                 (HARD_KMEANS)
    PaddleAdd = 2,       // (sum + support class sums) / (cs + support counts), every row           (PADDLE's w_update)
    PlainQuotient = 3,   // sum / cs, every row                                                      (BD-CSPN's rectified prototypes)
};

struct FeatureSpace {
    int D;               // elements of a feature row; n_class for probability features
    bool visual;

    // out[t,r,k] = temperature * (pre * ||w[t,k,:] - z[t,r,:]||^2) for the classes `need` marks
    int dist(int T, hipStream_t st, const float* w, const float* z, const uint8_t* need, int R, int K, float pre, float temperature,
             float* out) const {
        if (visual) return launch_vis_dist(T, st, w, z, need, R, K, D, pre, temperature, out);
        launch_kmeans_logits(T, st, w, z, need, R, K, pre, temperature, out);
        return TCLIP_OK;
    }

    // y[t,k,:] = sum_r u[t,r,k] z[t,r,:] over R rows, divided as `kind` says; `dense` (probability features only): the caller
    // expects nearly every class alive
    void mstats(hipStream_t st, const float* u, const float* z, const float* cs, const uint8_t* live, int T, int R, int K, Mstats kind,
                float* y, const float* sup, const float* cnt, bool dense) const {
        if (visual) {
            launch_vis_mstats(st, u, z, cs, live, T, R, K, D, (int)kind, y, sup, cnt);
            return;
        }
        launch_mstats(st, u, z, cs, live, sup, cnt, T, R, K, y, kind == Mstats::PaddleAdd ? 1 : kind == Mstats::PlainQuotient ? 2 : 0, dense);
        if (kind == Mstats::HardZeroDead) {
            const int TK = T * K;
            hipLaunchKernelGGL(k_zero_dead_rows, dim3(ew_grid((size_t)TK * K)), dim3(256), 0, st, live, TK, K, y);
        }
    }

    // EM_GAUSSIAN_COV: s[t,k,:] = cs[t,k] / max(sum_q (w[t,k,:] - z[t,q,:])^2 u[t,q,k], eps) for the rows `live` marks
    void cov_stats(hipStream_t st, const float* u, const float* z, const float* cs, const uint8_t* live, const float* w, int T, int Q,
                   int K, float* s) const {
        if (visual) launch_vis_cov_stats(st, u, z, cs, live, w, T, Q, K, D, s);
        else launch_cov_stats(st, u, z, cs, live, w, T, Q, K, s);
    }

    // EM_GAUSSIAN_COV: out[t,q,k] = -1/2 sum_d (w - z)^2 s + 1/2 sum_d log(s + eps) for the classes `need` marks; det [T, K] is
    // room for the half log-determinants (visual features only: the probability kernel keeps them in registers)
    int cov_logits(int T, hipStream_t st, const float* w, const float* s, const float* z, const uint8_t* need, int Q, int K, float* det,
                   float* out) const {
        if (visual) return launch_vis_cov_logits(T, st, w, s, z, need, Q, K, D, det, out);
        dispatch_E<LaunchCovLogitsRows>(K, T, st, w, s, z, need, Q, K, out);
        return TCLIP_OK;
    }

    // sup[t,k,:] = sum of the support rows of class k, cnt[t,k] = their number; the rows a dense [T, S, D] tensor or table
    // rows read in place (visual features: x_s.cols is not read)
    void support_stats(hipStream_t st, const RowSrc& x_s, const int64_t* y_s, int T, int S, int K, float* sup, float* cnt) const {
        if (visual) launch_vis_support_stats(st, x_s, y_s, T, S, K, D, sup, cnt);
        else hipLaunchKernelGGL(k_support_stats, dim3(K, T), dim3(128), (size_t)S * sizeof(int), st, x_s, y_s, S, K, 0, sup, cnt);
    }
};

// ---- workspace layouts: one function per method that returns typed pointers to 256-byte aligned regions and `bytes`, their
// sum; a null `base` gives `bytes` alone ---------------------------------------------------------------------------------------
// The k-means loops hold no feature rows of their own: no region depends on the row length.
// det (EM_GAUSSIAN_COV on visual features): the half log-determinants [T, K] f32, behind the k-means regions
struct KmeansWs {
    float* cs;
    uint8_t *live, *ones;
    float *logit, *change, *det;      // change [T] f32: HARD_KMEANS and KL_KMEANS only
    size_t bytes;
};
static KmeansWs kmeans_ws(const tclip_problem& p, bool det, char* base) {
    const size_t T = (size_t)p.n_batches * p.tasks_per_batch, K = p.n_class, Q = p.n_query;
    KmeansWs w;
    WsCursor c{base};
    c.take(w.cs, T * K * 4);
    c.take(w.live, T * K);
    c.take(w.ones, T * K);
    c.take(w.logit, T * Q * K * 4);
    c.take(w.change, T * 4);
    c.take(w.det, T * K * 4, det);
    w.bytes = c.bytes;
    return w;
}

// tables (PADDLE fed from the feature tables): the query rows [T, Q, D] follow, gathered once; nothing depends on n_support
struct PaddleWs {
    float *sup, *cnt, *cs;
    uint8_t* live;
    float *logit, *xq;
    size_t bytes;
};
static PaddleWs paddle_ws(const tclip_problem& p, int dim, bool tables, char* base) {
    const size_t T = (size_t)p.n_batches * p.tasks_per_batch, K = p.n_class, Q = p.n_query, D = dim;
    PaddleWs w;
    WsCursor c{base};
    c.take(w.sup, T * K * D * 4);
    c.take(w.cnt, T * K * 4);
    c.take(w.cs, T * K * 4);
    c.take(w.live, T * K);
    c.take(w.logit, T * Q * K * 4);
    c.take(w.xq, T * Q * D * 4, tables);
    w.bytes = c.bytes;
    return w;
}

// tables (BD-CSPN fed from the feature tables, bdcspn_pass with indexed sources): zs has no region of its own - it lies at the
// start of the logit region, which then holds max(T R K, T S D) floats.  Their lifetimes in bdcspn_pass do not overlap: zs is
// written by the first normalisation and last read by the normalisation that builds aug (after the support statistics and
// k_bdcspn_eta); logit is first written by the sp.dist that follows it, on the same stream, and nothing after that reads zs.
// sweep (tclip_bdcspn_sweep_tasks): the normalised initial prototypes get a region of their own, wn0 - every value reads
// them, and wn is overwritten by each value's rectified prototypes; otherwise wn0 is wn itself.  No region depends on the
// number of values.
struct BdcspnWs {
    float *zs, *zq, *zqn, *mean, *eta, *sup, *cnt, *wn, *aug, *logit, *cs;
    uint8_t* live;
    int32_t* dummy;
    float* wn0;
    size_t bytes;
};
static BdcspnWs bdcspn_ws(const tclip_problem& p, int dim, bool tables, bool sweep, char* base) {
    const size_t T = (size_t)p.n_batches * p.tasks_per_batch, K = p.n_class, Q = p.n_query, S = p.n_support, R = S + Q, D = dim;
    BdcspnWs w;
    WsCursor c{base};
    c.take(w.zs, T * S * D * 4, !tables);
    c.take(w.zq, T * Q * D * 4);
    c.take(w.zqn, T * Q * D * 4);
    c.take(w.mean, T * D * 4);
    c.take(w.eta, T * D * 4);
    c.take(w.sup, T * K * D * 4);
    c.take(w.cnt, T * K * 4);
    c.take(w.wn, T * K * D * 4);
    c.take(w.aug, T * R * D * 4);
    c.take(w.logit, (tables && S * D >= R * K ? T * S * D : T * R * K) * 4);
    if (tables) w.zs = w.logit;
    c.take(w.cs, T * K * 4);
    c.take(w.live, T * K);
    c.take(w.dummy, T * R * 4);
    c.take(w.wn0, T * K * D * 4, sweep);
    if (!sweep) w.wn0 = w.wn;
    w.bytes = c.bytes;
    return w;
}

// ---- SOFT_KMEANS, EM_GAUSSIAN, HARD_KMEANS (SURVEY.md section 8f, F1; BASELINE config 3's second method) ----------------
// Soft and EmGaussian share everything but the class-proportion term lambd * v / Q in the softmax and the v update
// (em_gaussian.py:129-143).  u_init: the features themselves for probability features, the text-prompt u0 for visual ones.
// Kl: the checks and outputs of Hard and a loop of its own.  kmeans_entry is the only place that turns a Kmeans into a loop and
// sends Kl to kl_kmeans_loop: kmeans_loop never receives it (it has no branch for it and would run it as Soft).
enum class Kmeans { Soft, EmGaussian, Hard, Kl };

static int kmeans_loop(const FeatureSpace& sp, Kmeans kind, const tclip_problem& p, const float* x_q, const float* u_init,
                       float temperature, float* u, float* v, float* w, int32_t* preds, float* criterions, const KmeansWs& ws,
                       hipStream_t st) {
    const bool hard = kind == Kmeans::Hard, emg = kind == Kmeans::EmGaussian;
    const int Q = p.n_query, K = p.n_class, B = p.n_batches, N = p.tasks_per_batch, T = B * N, TK = T * K;
    const size_t TQK = (size_t)T * Q * K;
    float *const cs = ws.cs, *const logit0 = ws.logit, *const change = ws.change;
    uint8_t *const live = ws.live, *const ones = ws.ones;
    hipLaunchKernelGGL(k_copy, dim3(ew_grid(TQK)), dim3(256), 0, st, u_init, u, TQK);       // u = z / u = u0
    TCLIP_HIP(hipMemsetAsync(ones, 1, (size_t)TK, st));                                     // HARD_KMEANS: every centroid moves every iteration
    if (emg) hipLaunchKernelGGL(k_fill, dim3(ew_grid(TK)), dim3(256), 0, st, v, 0.0f, (size_t)TK);
    if (!hard) {
        // w_init: every centroid = u^T z / clamp(sum u)                  (soft_kmeans.py:126-149, em_gaussian.py:145-155)
        hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 1, cs, live,
                           (float*)nullptr, (int32_t*)nullptr);
        sp.mstats(st, u, x_q, cs, ones, T, Q, K, Mstats::LiveOnly, w, nullptr, nullptr, true);
    }
    // SOFT_KMEANS keeps its clusters alive (every query spreads its responsibility over all of them); EM_GAUSSIAN's class-proportion
    // term leaves a handful per task after two iterations (profiles/r05_kmeans_live_clusters.txt): only the former is "dense"
    const bool dense = kind == Kmeans::Soft;
    for (int it = 0; it < p.iters; it++) {
        // w_update: live clusters get the new mean; empty ones keep their centroid (soft_kmeans.py:151-168) or, HARD_KMEANS, become
        // zero (hard_kmeans.py:138-152).  EM_GAUSSIAN: the same pass over u also yields v of the previous iteration's v_update
        // (v stays 0 before the first)
        hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 1, cs, live,
                           (emg && it > 0) ? v : (float*)nullptr, (int32_t*)nullptr);
        sp.mstats(st, u, x_q, cs, live, T, Q, K, hard ? Mstats::HardZeroDead : Mstats::LiveOnly, w, nullptr, nullptr, dense);
        if (hard) {
            // u_update + hard assignment: softmax of the squared distances, first minimum      (hard_kmeans.py:128-136, :193-195)
            if (int rc = sp.dist(T, st, w, x_q, ones, Q, K, 1.0f, 1.0f, logit0)) return rc;
            hipLaunchKernelGGL(k_softmax, dim3((T * Q * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit0,
                               (const float*)nullptr, T * Q, Q, K, 0.0f, 0, 1, logit0, preds);
            // criterion mean_n ||u_old - u||_F, u <- one-hot                                                      (:197-199)
            hipLaunchKernelGGL(k_hard_assign, dim3(T), dim3(256), 0, st, (const int32_t*)preds, Q, K, u, change);
            hipLaunchKernelGGL(k_criterion_mean, dim3(B), dim3(64), 0, st, (const float*)change, N, 0, criterions + it, p.iters);
        } else {
            // distances only for centroids that moved (all of them in the first iteration), E-step softmax
            if (int rc = sp.dist(T, st, w, x_q, it == 0 ? ones : live, Q, K, -0.5f, temperature, logit0)) return rc;
            hipLaunchKernelGGL(k_softmax, dim3((T * Q * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit0,
                               (const float*)v, T * Q, Q, K, (float)p.lambd, 0, 0, u, preds);
        }
    }
    if (emg)      // the last v_update
        hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 1, cs, live, v,
                           (int32_t*)nullptr);
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

// ---- EM_GAUSSIAN_COV (SURVEY.md F1): EM_GAUSSIAN with a diagonal inverse covariance per cluster; no temperature -----------
// ws.det: room for [T, K] floats on visual features, null (unused) on probability features.
static int em_gaussian_cov_loop(const FeatureSpace& sp, const tclip_problem& p, const float* x_q, const float* u_init, float* u, float* v,
                                float* w, float* s, int32_t* preds, const KmeansWs& ws, hipStream_t st) {
    const int Q = p.n_query, K = p.n_class, T = p.n_batches * p.tasks_per_batch, TK = T * K;
    const size_t TQK = (size_t)T * Q * K;
    float *const cs = ws.cs, *const logit0 = ws.logit, *const det = ws.det;
    uint8_t *const live = ws.live, *const ones = ws.ones;
    hipLaunchKernelGGL(k_copy, dim3(ew_grid(TQK)), dim3(256), 0, st, u_init, u, TQK);       // u = z / u = u0
    TCLIP_HIP(hipMemsetAsync(ones, 1, (size_t)TK, st));
    hipLaunchKernelGGL(k_fill, dim3(ew_grid(TK)), dim3(256), 0, st, v, 0.0f, (size_t)TK);
    // w_init, s_init: every cluster                                                (em_gaussian_cov.py:146-180)
    hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 1, cs, live,
                       (float*)nullptr, (int32_t*)nullptr);
    sp.mstats(st, u, x_q, cs, ones, T, Q, K, Mstats::LiveOnly, w, nullptr, nullptr, false);
    sp.cov_stats(st, u, x_q, cs, ones, w, T, Q, K, s);
    for (int it = 0; it < p.iters; it++) {
        // w_update, s_update: non-empty clusters move, empty ones keep w and s        (:160-193); v of the previous v_update
        hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 1, cs,
                           live, it > 0 ? v : (float*)nullptr, (int32_t*)nullptr);
        sp.mstats(st, u, x_q, cs, live, T, Q, K, Mstats::LiveOnly, w, nullptr, nullptr, false);
        sp.cov_stats(st, u, x_q, cs, live, w, T, Q, K, s);
        // u_update: Mahalanobis distances + log-determinants of the clusters that moved, softmax with lambd v / Q   (:106-129)
        if (int rc = sp.cov_logits(T, st, w, s, x_q, it == 0 ? ones : live, Q, K, det, logit0)) return rc;
        hipLaunchKernelGGL(k_softmax, dim3((T * Q * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit0,
                           (const float*)v, T * Q, Q, K, (float)p.lambd, 0, 0, u, preds);
    }
    hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 1, cs, live, v,
                       (int32_t*)nullptr);                                              // the last v_update
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

// ---- PADDLE (SURVEY.md section 8f, F4): few-shot soft k-means with the class-proportion penalty -------------------------
// The support set is read exactly once, for the class sums: `x_s` is a dense tensor or table rows read in place.
// values != nullptr (tclip_paddle_sweep_tasks): the loop runs once per value, one after the other on the stream, with
// lambd = (float)values[i] and slice i of u [P,T,Q,K], v [P,T,K], w [P,T,K,D], preds [P,T,Q].  The class sums - the one launch
// that reads the support set, and the only one before the loop that is more than a fill - are taken once; cs, live and the
// logits are scratch every value reuses.  Each value sees the launches of a single-value call with the same arguments.
static int paddle_loop(const FeatureSpace& sp, const tclip_problem& p, const float* x_q, const RowSrc& x_s, const int64_t* y_s,
                       float lambd, float* u, float* v, float* w, int32_t* preds, const PaddleWs& ws, hipStream_t st,
                       const double* values = nullptr, int n_values = 0) {
    const int Q = p.n_query, K = p.n_class, D = sp.D, S = p.n_support, T = p.n_batches * p.tasks_per_batch, TK = T * K;
    const size_t TQ = (size_t)T * Q;
    float *const sup = ws.sup, *const cnt = ws.cnt, *const cs = ws.cs, *const logit0 = ws.logit;
    uint8_t* const live = ws.live;
    // init (paddle.py:180-197): v = 0, w = class means of the support set (on visual features the text-prompt u is overwritten
    // before it is read); every centroid moves every iteration
    for (int i = 0; i < (values ? n_values : 1); i++, u += TQ * K, v += TK, w += (size_t)TK * D, preds += TQ) {
        if (values) lambd = (float)values[i];
        hipLaunchKernelGGL(k_fill, dim3(ew_grid(TK)), dim3(256), 0, st, v, 0.0f, (size_t)TK);
        if (i == 0) sp.support_stats(st, x_s, y_s, T, S, K, sup, cnt);
        hipLaunchKernelGGL(k_div_rows, dim3(ew_grid((size_t)TK * D)), dim3(256), 0, st, (const float*)sup, (const float*)cnt,
                           (size_t)TK * D, D, w);
        TCLIP_HIP(hipMemsetAsync(live, 1, (size_t)TK, st));
        for (int it = 0; it < p.iters; it++) {
            // u_update (:105-116): softmax_k(-1/2 ||w_k - z_q||^2 + lambd v_k / Q)
            if (int rc = sp.dist(T, st, w, x_q, live, Q, K, -0.5f, 1.0f, logit0)) return rc;
            hipLaunchKernelGGL(k_softmax, dim3((T * Q * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit0, (const float*)v,
                               T * Q, Q, K, lambd, 0, 0, u, preds);
            // v_update (:118-124) and w_update (:142-158)
            hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 0, cs, live, v,
                               (int32_t*)nullptr);
            sp.mstats(st, u, x_q, cs, live, T, Q, K, Mstats::PaddleAdd, w, sup, cnt, false);
        }
    }
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

// ---- BD-CSPN (SURVEY.md F4): one pass, no loop ------------------------------------------------------------------------
// k_col_mean, k_bdcspn_normalize, k_bdcspn_eta and k_div_rows take the row length where their signatures say K.
// x_q / x_s: dense tensors, or table rows read in place by the only three launches that touch them (the train mean and the
// two normalisations into zs / zq); `ws`: bdcspn_ws of the form (table rows: zs inside logit).
// values != nullptr (tclip_bdcspn_sweep_tasks; ws.wn0 a region of its own): everything up to and including the augmented set
// reads no temp and runs once; from the first soft assignment on the pass runs once per value, one after the other on the
// stream, with temp = (float)values[i] and slice i of prototypes [P,T,K,D], u [P,T,Q,K], preds [P,T,Q].  Each value sees the
// launches of a single-value call with the same arguments.
static int bdcspn_pass(const FeatureSpace& sp, const tclip_problem& p, const BdcspnWs& ws, const RowSrc& x_q, const RowSrc& x_s,
                       const int64_t* y_s, float temp, int norm_type, float* prototypes, float* u, int32_t* preds, hipStream_t st,
                       const double* values = nullptr, int n_values = 0) {
    const int Q = p.n_query, K = p.n_class, D = sp.D, S = p.n_support, R = S + Q, T = p.n_batches * p.tasks_per_batch, TK = T * K;
    const int TD = T * D;
    float *const zs = ws.zs, *const zq = ws.zq, *const zqn = ws.zqn, *const mean = ws.mean, *const eta = ws.eta, *const sup = ws.sup;
    float *const cnt = ws.cnt, *const wn = ws.wn, *const aug = ws.aug, *const logit = ws.logit, *const cs = ws.cs;
    float* const wn0 = ws.wn0;                                        // the normalised initial prototypes: wn itself but in a sweep
    uint8_t* const live = ws.live;
    int32_t* const dummy = ws.dummy;
    auto rows_grid = [](int n_rows) { return dim3((unsigned)(((size_t)n_rows * 8 + 255) / 256)); };
    auto normalize = [&](const float* x, const float* x2, int R0, int Rr, int mode, const float* mn, const float* sh, float* out) {
        hipLaunchKernelGGL(k_bdcspn_normalize<false>, rows_grid(T * Rr), dim3(256), 0, st, dense_rows(x), x2, R0, Rr, D, mode, mn, sh,
                           T * Rr, out);
    };
    // the task rows: one source of Rr rows per task
    auto normalize_rows = [&](const RowSrc& x, int Rr, float* out) {
        if (x.idx)
            hipLaunchKernelGGL(k_bdcspn_normalize<true>, rows_grid(T * Rr), dim3(256), 0, st, x, (const float*)nullptr, Rr, Rr, D,
                               norm_type, (const float*)mean, (const float*)nullptr, T * Rr, out);
        else
            normalize(x.base, x.base, Rr, Rr, norm_type, (const float*)mean, (const float*)nullptr, out);
    };
    // normalization (bdcspn.py:77-100, :165-166): train_mean = support.mean(1), an outer sum over D columns; CL2N / L2N / none
    if (norm_type == 2) {
        if (x_s.idx) hipLaunchKernelGGL(k_col_mean<true>, dim3((TD + 255) / 256), dim3(256), 0, st, x_s, T, S, D, mean);
        else hipLaunchKernelGGL(k_col_mean<false>, dim3((TD + 255) / 256), dim3(256), 0, st, x_s, T, S, D, mean);
    }
    normalize_rows(x_s, S, zs);
    normalize_rows(x_q, Q, zq);
    // initial prototypes: support class means (:117-120), L2-normalised for get_logits (:50)
    sp.support_stats(st, dense_rows(zs), y_s, T, S, K, sup, cnt);
    hipLaunchKernelGGL(k_div_rows, dim3(ew_grid((size_t)TK * D)), dim3(256), 0, st, (const float*)sup, (const float*)cnt,
                       (size_t)TK * D, D, prototypes);
    normalize((const float*)prototypes, (const float*)prototypes, K, K, 1, (const float*)nullptr, (const float*)nullptr, wn0);
    // augmented set: support rows, then query rows shifted by eta = mean(support) - mean(query); normalised (:127-131, :51, :137)
    hipLaunchKernelGGL(k_bdcspn_eta, dim3((TD + 255) / 256), dim3(256), 0, st, (const float*)zs, (const float*)zq, T, S, Q, D, eta);
    normalize((const float*)zs, (const float*)zq, S, R, 1, (const float*)nullptr, (const float*)eta, aug);
    for (int i = 0; i < (values ? n_values : 1); i++, prototypes += (size_t)TK * D, u += (size_t)T * Q * K, preds += (size_t)T * Q) {
        if (values) temp = (float)values[i];
        // soft assignment of the augmented set to the initial prototypes (:133-134)
        TCLIP_HIP(hipMemsetAsync(live, 1, (size_t)TK, st));
        if (int rc = sp.dist(T, st, wn0, aug, live, R, K, -0.5f, temp, logit)) return rc;
        hipLaunchKernelGGL(k_softmax, dim3((T * R * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit, (const float*)nullptr,
                           T * R, R, K, 0.0f, 0, 0, logit, dummy);
        // rectified prototypes = assignment-weighted means of the normalised augmented set (:137-141)
        hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)logit, T, R, K, 0, cs, live,
                           (float*)nullptr, (int32_t*)nullptr);
        sp.mstats(st, logit, aug, cs, live, T, R, K, Mstats::PlainQuotient, prototypes, nullptr, nullptr, false);
        // prediction (:190-193): softmax(temp * get_logits(prototypes, query)), argmax
        normalize((const float*)prototypes, (const float*)prototypes, K, K, 1, (const float*)nullptr, (const float*)nullptr, wn);
        normalize((const float*)zq, (const float*)zq, Q, Q, 1, (const float*)nullptr, (const float*)nullptr, zqn);
        if (int rc = sp.dist(T, st, wn, zqn, live, Q, K, -0.5f, temp, logit)) return rc;
        hipLaunchKernelGGL(k_softmax, dim3((T * Q * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit, (const float*)nullptr,
                           T * Q, Q, K, 0.0f, 0, 0, u, preds);
    }
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

// ---- KL_KMEANS: HARD_KMEANS's outputs with KL centroids and divergences; probability features only.  The 75-column split below
// is its own arithmetic, not launch_mstats_mode's.  The loop stands behind bdcspn_pass, where the entry that held it stood: the
// kernel templates of a translation unit are emitted in the order of their first use, and the device code keeps that order.
static int kl_kmeans_loop(const tclip_problem& p, const float* x_q, float* u, float* w, int32_t* preds, float* criterions,
                          const KmeansWs& ws, hipStream_t st) {
    const int Q = p.n_query, K = p.n_class, B = p.n_batches, N = p.tasks_per_batch, T = B * N, TK = T * K;
    const size_t TQK = (size_t)T * Q * K;
    float *const cs = ws.cs, *const divs = ws.logit, *const change = ws.change;
    uint8_t* const live = ws.live;
    hipLaunchKernelGGL(k_copy, dim3(ew_grid(TQK)), dim3(256), 0, st, x_q, u, TQK);          // u = z
    for (int it = 0; it < p.iters; it++) {
        hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 1, cs,
                           live, (float*)nullptr, (int32_t*)nullptr);
        if (Q == kColsQ && K >= kColsChunk && g_knobs.kmeans_tile != 0) {
            const int dtiles = (K + 63) / 64;
            int splits = (int)((8192 + (long)T * dtiles - 1) / ((long)T * dtiles));
            if (splits > K / (kColsWaves * kColsChunk)) splits = K / (kColsWaves * kColsChunk);
            if (splits < 1) splits = 1;
            const int rows_per_block = ((K + splits - 1) / splits + kColsChunk - 1) / kColsChunk * kColsChunk;
            const int ksplits = (K + rows_per_block - 1) / rows_per_block;
            hipLaunchKernelGGL(k_kl_centroids_cols75, dim3(task_tile_grid(dtiles, ksplits, T)), dim3(64 * kColsWaves), 0,
                               st, (const float*)u, x_q, (const float*)cs, K, rows_per_block, w, T, dtiles, ksplits);
        } else {
            hipLaunchKernelGGL(k_kl_centroids, dim3((K + 63) / 64, (K + kMstatsRows - 1) / kMstatsRows, T), dim3(64), 0, st,
                               (const float*)u, x_q, (const float*)cs, Q, K, w);
        }
        if (g_knobs.kmeans_tile != 0 && K >= 32 && K <= 511 && kmeans_tile_lds_raised((const void*)k_kl_divergences_tile)) {
            const int stride = K | 1;
            hipLaunchKernelGGL(k_kl_divergences_tile, dim3((K + kKmeansTile - 1) / kKmeansTile, T), dim3(kKmeansTileThreads),
                               (size_t)kKmeansTile * stride * sizeof(float), st, (const float*)w, x_q, Q, K, stride, divs);
        } else {
            dispatch_E<LaunchKlDivergences>(K, T, st, (const float*)w, x_q, Q, K, divs);
        }
        hipLaunchKernelGGL(k_argmin_rows, dim3((T * Q + 255) / 256), dim3(256), 0, st, (const float*)divs, T * Q, K, preds);
        hipLaunchKernelGGL(k_hard_assign, dim3(T), dim3(256), 0, st, (const int32_t*)preds, Q, K, u, change);
        hipLaunchKernelGGL(k_criterion_mean, dim3(B), dim3(64), 0, st, (const float*)change, N, 0, criterions + it, p.iters);
    }
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

// ---- the entries: one function per method for all its call forms (`r`: tclip_tim.inc), the checks in the one order of
// DESIGN.md ("The method host drivers"), then the loop; ws_query: the workspace query the entry's caller was told to use ------
static const MethodRule kSoftKmeans{"SOFT_KMEANS", false, kZeroShotOnly, nullptr, Limits::None};
static const MethodRule kEmGaussian{"EM_GAUSSIAN", false, kZeroShotOnly, nullptr, Limits::None};
static const MethodRule kHardKmeans{"HARD_KMEANS", false, kZeroShotOnly, nullptr, Limits::None};
static const MethodRule kKlKmeans{"KL_KMEANS", false, kZeroShotOnly, nullptr, Limits::None};
static const MethodRule kEmGaussianCov{"EM_GAUSSIAN_COV", false, kZeroShotOnly, nullptr, Limits::None};
static const MethodRule kVisualKmeans{"", false, "the visual k-means methods are zero-shot: n_support must be 0", nullptr, Limits::None};
static const MethodRule kPaddle{"PADDLE", true, kFewShotOnly, nullptr, Limits::Rows16};
static const MethodRule kBdcspn{"BDCSPN", true, kFewShotOnly, nullptr, Limits::Rows16};

// SOFT_KMEANS, EM_GAUSSIAN, HARD_KMEANS on either feature kind and KL_KMEANS (probability features); `known`: the visual
// entry's method code names one of them; u0: the text-prompt assignment of visual features.  v and criterions are needed by the
// methods that write them.
static int kmeans_entry(const tclip_problem* pp, const Rows& r, const MethodRule& m, Kmeans kind, bool known, const float* u0,
                        float temperature, float* u, float* v, float* w, int32_t* preds, float* criterions, void* workspace,
                        size_t workspace_bytes, void* stream, const char* ws_query) {
    if (int rc = check_method_problem(pp, r, m)) return rc;
    if (!known) return fail(TCLIP_ERR_ARG, "unknown method");
    const bool hard = kind == Kmeans::Hard || kind == Kmeans::Kl;
    if (int rc = check_pointers(r, m, (u0 || !r.visual) && u && w && preds && workspace && (criterions || !hard) &&
                                          (v || kind != Kmeans::EmGaussian)))
        return rc;
    const tclip_problem p = *pp;
    if (int rc = check_workspace(workspace, workspace_bytes, kmeans_ws(p, false, nullptr).bytes, ws_query)) return rc;
    const KmeansWs ws = kmeans_ws(p, false, (char*)workspace);
    if (kind == Kmeans::Kl) return kl_kmeans_loop(p, r.x_q, u, w, preds, criterions, ws, (hipStream_t)stream);
    return kmeans_loop(FeatureSpace{r.D(p), r.visual}, kind, p, r.x_q, r.visual ? u0 : r.x_q, temperature, u, v, w, preds, criterions, ws,
                       (hipStream_t)stream);
}

static int em_gaussian_cov_entry(const tclip_problem* pp, const Rows& r, const float* u0, float* u, float* v, float* w, float* s,
                                 int32_t* preds, void* workspace, size_t workspace_bytes, void* stream, const char* ws_query) {
    if (int rc = check_method_problem(pp, r, kEmGaussianCov)) return rc;
    if (int rc = check_pointers(r, kEmGaussianCov, (u0 || !r.visual) && u && v && w && s && preds && workspace)) return rc;
    const tclip_problem p = *pp;
    if (int rc = check_workspace(workspace, workspace_bytes, kmeans_ws(p, r.visual, nullptr).bytes, ws_query)) return rc;
    return em_gaussian_cov_loop(FeatureSpace{r.D(p), r.visual}, p, r.x_q, r.visual ? u0 : r.x_q, u, v, w, s, preds,
                                kmeans_ws(p, r.visual, (char*)workspace), (hipStream_t)stream);
}

// PADDLE.  From the feature tables the queries are gathered (and, probability features, permuted) once into the workspace and
// the support rows are read in place by the support statistics; then paddle_loop as it stands.
static int paddle_entry(const tclip_problem* pp, const Rows& r, const int64_t* y_s, float lambd, float* u, float* v, float* w,
                        int32_t* preds, void* workspace, size_t workspace_bytes, void* stream, const char* ws_query) {
    if (int rc = check_method_problem(pp, r, kPaddle)) return rc;
    if (int rc = check_pointers(r, kPaddle, y_s && u && v && w && preds && workspace)) return rc;
    if (int rc = check_values(pp, r)) return rc;
    const tclip_problem p = *pp;
    const int D = r.D(p);
    if (int rc = check_workspace(workspace, workspace_bytes, paddle_ws(p, D, r.tables, nullptr).bytes, ws_query)) return rc;
    const PaddleWs ws = paddle_ws(p, D, r.tables, (char*)workspace);
    hipStream_t st = (hipStream_t)stream;
    // every q_idx value has been checked by the caller (tclip_check_task_indices): no row of ws.xq stays unwritten
    if (r.tables)
        launch_gather_task_rows(st, r.src->table_q, INT64_MAX, D, r.src->q_idx, p.n_query, r.src->cols,
                                (int64_t)p.n_batches * p.tasks_per_batch * p.n_query, ws.xq);
    return paddle_loop(FeatureSpace{D, r.visual}, p, r.tables ? ws.xq : r.x_q, r.s(), y_s, lambd, u, v, w, preds, ws, st, r.values,
                       r.n_sweep());
}
static size_t paddle_bytes(const tclip_problem* p, const Rows& r) {
    return query_accepts(p, r, kPaddle) ? paddle_ws(*p, r.D(*p), r.tables, nullptr).bytes : 0;
}

// BD-CSPN.  From the feature tables bdcspn_pass reads both row sets in place, neither x_s nor x_q is built.
static int bdcspn_entry(const tclip_problem* pp, const Rows& r, const int64_t* y_s, float temp, int32_t norm_type, float* prototypes,
                        float* u, int32_t* preds, void* workspace, size_t workspace_bytes, void* stream, const char* ws_query) {
    if (int rc = check_method_problem(pp, r, kBdcspn)) return rc;
    if (int rc = check_pointers(r, kBdcspn, y_s && prototypes && u && preds && workspace)) return rc;
    if (norm_type < 0 || norm_type > 2) return fail(TCLIP_ERR_ARG, "norm_type must be 0 (UN), 1 (L2N) or 2 (CL2N)");
    if (int rc = check_values(pp, r)) return rc;
    const tclip_problem p = *pp;
    const int D = r.D(p);
    if (int rc = check_workspace(workspace, workspace_bytes, bdcspn_ws(p, D, r.tables, r.sweep, nullptr).bytes, ws_query)) return rc;
    return bdcspn_pass(FeatureSpace{D, r.visual}, p, bdcspn_ws(p, D, r.tables, r.sweep, (char*)workspace), r.q(), r.s(), y_s, temp,
                       norm_type, prototypes, u, preds, (hipStream_t)stream, r.values, r.n_sweep());
}
static size_t bdcspn_bytes(const tclip_problem* p, const Rows& r) {
    return query_accepts(p, r, kBdcspn) ? bdcspn_ws(*p, r.D(*p), r.tables, r.sweep, nullptr).bytes : 0;
}

}  // namespace tclip

extern "C" {

// ---- zero-shot, probability features: the two queries do not look at n_support ------------------------------------------------
size_t tclip_soft_kmeans_workspace_bytes(const tclip_problem* p) {
    return query_accepts(p, rows_dense(nullptr, nullptr, kAnySupport), kSoftKmeans) ? kmeans_ws(*p, false, nullptr).bytes : 0;
}

size_t tclip_hard_kmeans_workspace_bytes(const tclip_problem* p) { return tclip_soft_kmeans_workspace_bytes(p); }

int tclip_soft_kmeans_run(const tclip_problem* pp, const float* x_q, float temperature, float* u, float* w,
                          int32_t* preds, void* workspace, size_t workspace_bytes, void* stream) {
    return kmeans_entry(pp, rows_dense(x_q, nullptr), kSoftKmeans, Kmeans::Soft, true, nullptr, temperature, u, nullptr, w, preds, nullptr,
                        workspace, workspace_bytes, stream, "tclip_soft_kmeans_workspace_bytes");
}

int tclip_em_gaussian_run(const tclip_problem* pp, const float* x_q, float temperature, float* u, float* v, float* w,
                          int32_t* preds, void* workspace, size_t workspace_bytes, void* stream) {
    return kmeans_entry(pp, rows_dense(x_q, nullptr), kEmGaussian, Kmeans::EmGaussian, true, nullptr, temperature, u, v, w, preds, nullptr,
                        workspace, workspace_bytes, stream, "tclip_soft_kmeans_workspace_bytes");
}

int tclip_hard_kmeans_run(const tclip_problem* pp, const float* x_q, float* u, float* w, int32_t* preds,
                          float* criterions, void* workspace, size_t workspace_bytes, void* stream) {
    return kmeans_entry(pp, rows_dense(x_q, nullptr), kHardKmeans, Kmeans::Hard, true, nullptr, 1.0f, u, nullptr, w, preds, criterions,
                        workspace, workspace_bytes, stream, "tclip_hard_kmeans_workspace_bytes");
}

// KL_KMEANS: HARD_KMEANS's arguments and outputs, with KL centroids and divergences
int tclip_kl_kmeans_run(const tclip_problem* pp, const float* x_q, float* u, float* w, int32_t* preds,
                        float* criterions, void* workspace, size_t workspace_bytes, void* stream) {
    return kmeans_entry(pp, rows_dense(x_q, nullptr), kKlKmeans, Kmeans::Kl, true, nullptr, 1.0f, u, nullptr, w, preds, criterions,
                        workspace, workspace_bytes, stream, "tclip_hard_kmeans_workspace_bytes");
}

int tclip_em_gaussian_cov_run(const tclip_problem* pp, const float* x_q, float* u, float* v, float* w, float* s,
                              int32_t* preds, void* workspace, size_t workspace_bytes, void* stream) {
    return em_gaussian_cov_entry(pp, rows_dense(x_q, nullptr), nullptr, u, v, w, s, preds, workspace, workspace_bytes, stream,
                                 "tclip_soft_kmeans_workspace_bytes");
}

// ---- zero-shot, visual features: the k-means query does not look at n_support, EM_GAUSSIAN_COV's does --------------------------
size_t tclip_visual_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return query_accepts(p, rows_visual(dim, nullptr, nullptr, kAnySupport), kVisualKmeans) ? kmeans_ws(*p, false, nullptr).bytes : 0;
}

int tclip_kmeans_visual_run(const tclip_problem* pp, int32_t dim, int32_t method, const float* x_q, const float* u0,
                            float temperature, float* u, float* v, float* w, int32_t* preds, float* criterions, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const bool known = method == TCLIP_VISUAL_SOFT_KMEANS || method == TCLIP_VISUAL_HARD_KMEANS || method == TCLIP_VISUAL_EM_GAUSSIAN;
    const Kmeans kind = method == TCLIP_VISUAL_HARD_KMEANS ? Kmeans::Hard : method == TCLIP_VISUAL_EM_GAUSSIAN ? Kmeans::EmGaussian : Kmeans::Soft;
    return kmeans_entry(pp, rows_visual(dim, x_q, nullptr), kVisualKmeans, kind, known, u0, temperature, u, v, w, preds, criterions,
                        workspace, workspace_bytes, stream, "tclip_visual_workspace_bytes");
}

size_t tclip_em_gaussian_cov_visual_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return query_accepts(p, rows_visual(dim, nullptr, nullptr), kEmGaussianCov) ? kmeans_ws(*p, true, nullptr).bytes : 0;
}

int tclip_em_gaussian_cov_visual_run(const tclip_problem* pp, int32_t dim, const float* x_q, const float* u0, float* u, float* v,
                                     float* w, float* s, int32_t* preds, void* workspace, size_t workspace_bytes, void* stream) {
    return em_gaussian_cov_entry(pp, rows_visual(dim, x_q, nullptr), u0, u, v, w, s, preds, workspace, workspace_bytes, stream,
                                 "tclip_em_gaussian_cov_visual_workspace_bytes");
}

// ---- PADDLE: the dense probability query does not look at n_support -----------------------------------------------------------
size_t tclip_paddle_workspace_bytes(const tclip_problem* p) { return paddle_bytes(p, rows_dense(nullptr, nullptr, kAnySupport)); }
size_t tclip_paddle_tasks_workspace_bytes(const tclip_problem* p) { return paddle_bytes(p, rows_tables(nullptr)); }
size_t tclip_paddle_visual_workspace_bytes(const tclip_problem* p, int32_t dim) { return paddle_bytes(p, rows_visual(dim, nullptr, nullptr)); }
size_t tclip_paddle_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return paddle_bytes(p, rows_visual_tables(dim, nullptr));
}
size_t tclip_paddle_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values) {
    return paddle_bytes(p, rows_sweep(dim, nullptr, nullptr, n_values));
}

int tclip_paddle_run(const tclip_problem* pp, const float* x_q, const float* x_s, const int64_t* y_s, float lambd,
                     float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes,
                     void* stream) {
    return paddle_entry(pp, rows_dense(x_q, x_s), y_s, lambd, u, v, w, preds, workspace, workspace_bytes, stream,
                        "tclip_paddle_workspace_bytes");
}

int tclip_paddle_visual_run(const tclip_problem* pp, int32_t dim, const float* x_q, const float* x_s, const int64_t* y_s,
                            float lambd, float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes,
                            void* stream) {
    return paddle_entry(pp, rows_visual(dim, x_q, x_s), y_s, lambd, u, v, w, preds, workspace, workspace_bytes, stream,
                        "tclip_paddle_visual_workspace_bytes");
}

int tclip_paddle_run_tasks(const tclip_problem* pp, const tclip_task_source* src, const int64_t* y_s, float lambd, float* u, float* v,
                           float* w, int32_t* preds, void* workspace, size_t workspace_bytes, void* stream) {
    return paddle_entry(pp, rows_tables(src), y_s, lambd, u, v, w, preds, workspace, workspace_bytes, stream,
                        "tclip_paddle_tasks_workspace_bytes");
}

int tclip_paddle_visual_run_tasks(const tclip_problem* pp, int32_t dim, const tclip_task_source* src, const int64_t* y_s, float lambd,
                                  float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes, void* stream) {
    return paddle_entry(pp, rows_visual_tables(dim, src), y_s, lambd, u, v, w, preds, workspace, workspace_bytes, stream,
                        "tclip_paddle_visual_tasks_workspace_bytes");
}

// for a list of lambd values on the same tasks (paddle_loop with `values`)
int tclip_paddle_sweep_tasks(const tclip_problem* pp, int32_t dim, const tclip_task_source* src, const int64_t* y_s, const double* values,
                             int32_t n_values, float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return paddle_entry(pp, rows_sweep(dim, src, values, n_values), y_s, 0.0f, u, v, w, preds, workspace, workspace_bytes, stream,
                        "tclip_paddle_sweep_tasks_workspace_bytes");
}

// ---- BD-CSPN: the dense probability query does not look at n_support ----------------------------------------------------------
size_t tclip_bdcspn_workspace_bytes(const tclip_problem* p) { return bdcspn_bytes(p, rows_dense(nullptr, nullptr, kAnySupport)); }
size_t tclip_bdcspn_tasks_workspace_bytes(const tclip_problem* p) { return bdcspn_bytes(p, rows_tables(nullptr)); }
size_t tclip_bdcspn_visual_workspace_bytes(const tclip_problem* p, int32_t dim) { return bdcspn_bytes(p, rows_visual(dim, nullptr, nullptr)); }
size_t tclip_bdcspn_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return bdcspn_bytes(p, rows_visual_tables(dim, nullptr));
}
size_t tclip_bdcspn_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values) {
    return bdcspn_bytes(p, rows_sweep(dim, nullptr, nullptr, n_values));
}

int tclip_bdcspn_run(const tclip_problem* pp, const float* x_q, const float* x_s, const int64_t* y_s, float temp,
                     int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return bdcspn_entry(pp, rows_dense(x_q, x_s), y_s, temp, norm_type, prototypes, u, preds, workspace, workspace_bytes, stream,
                        "tclip_bdcspn_workspace_bytes");
}

int tclip_bdcspn_visual_run(const tclip_problem* pp, int32_t dim, const float* x_q, const float* x_s, const int64_t* y_s, float temp,
                            int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return bdcspn_entry(pp, rows_visual(dim, x_q, x_s), y_s, temp, norm_type, prototypes, u, preds, workspace, workspace_bytes, stream,
                        "tclip_bdcspn_visual_workspace_bytes");
}

int tclip_bdcspn_run_tasks(const tclip_problem* pp, const tclip_task_source* src, const int64_t* y_s, float temp, int32_t norm_type,
                           float* prototypes, float* u, int32_t* preds, void* workspace, size_t workspace_bytes, void* stream) {
    return bdcspn_entry(pp, rows_tables(src), y_s, temp, norm_type, prototypes, u, preds, workspace, workspace_bytes, stream,
                        "tclip_bdcspn_tasks_workspace_bytes");
}

int tclip_bdcspn_visual_run_tasks(const tclip_problem* pp, int32_t dim, const tclip_task_source* src, const int64_t* y_s, float temp,
                                  int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return bdcspn_entry(pp, rows_visual_tables(dim, src), y_s, temp, norm_type, prototypes, u, preds, workspace, workspace_bytes, stream,
                        "tclip_bdcspn_visual_tasks_workspace_bytes");
}

// for a list of temp values on the same tasks (bdcspn_pass with `values`)
int tclip_bdcspn_sweep_tasks(const tclip_problem* pp, int32_t dim, const tclip_task_source* src, const int64_t* y_s, const double* values,
                             int32_t n_values, int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return bdcspn_entry(pp, rows_sweep(dim, src, values, n_values), y_s, 0.0f, norm_type, prototypes, u, preds, workspace, workspace_bytes,
                        stream, "tclip_bdcspn_sweep_tasks_workspace_bytes");
}

}  // extern "C"
