// Few-shot PADDLE and BD-CSPN on VISUAL features (the reference's use_softmax_feature == False; src/methods/few_shot/paddle.py:94-219,
// bdcspn.py:42-200): included at the end of tclip_kernels.hip after tclip_visual.inc, uses its k_vis_dist / k_vis_mstats and
// the library's helpers (fail, check_problem, align_up, ew_grid, k_fill, k_div_rows, k_cluster_sizes, k_softmax, k_col_mean,
// k_bdcspn_normalize, k_bdcspn_eta, SparseCascade, outer_column_is_cascade).
//
// The op sequences are the ones of tclip_paddle_run / tclip_bdcspn_run; what changes is that a feature row has D elements,
// D independent of the class count K: prototypes and centroids are [T, K, D], support rows [T, S, D], query rows [T, Q, D],
// the responsibilities stay [T, Q, K].  k_col_mean, k_bdcspn_normalize, k_bdcspn_eta and k_div_rows only ever used their K
// argument as the row length and take D in its place; the softmax, the cluster sizes and v only see [*, K] rows.  The support
// class sums are new here; the centroid statistics are k_vis_mstats's few-shot modes (tclip_visual.inc).

namespace tclip {

// ---- support class sums ------------------------------------------------------------------------------------------------
// sup[t,k,d] = sum_s 1[y_s = k] x_s[t,s,d] in the order of torch's (support.unsqueeze(2) * y_s_one_hot.unsqueeze(3)).sum(1): an
// outer sum over S rows of K*D contiguous columns, so the cascade levels follow S and the last K*D mod 32 columns take the
// 4-way row sum.  cnt[t,k] = the number of members (y_s_one_hot.sum(1): a sum of zeros and ones, exact in any order).
// One block per (class, task): the members of the class are compacted in order into LDS and only they are visited; the dumps
// that fall between two members are replayed (SparseCascade), since the zero products of the other rows only matter through
// the positions of the dumps.  A label outside 0..K-1 matches no block and is never used as an index.
__global__ __launch_bounds__(256) void k_vis_support_stats(const float* __restrict__ xs, const int64_t* __restrict__ ys, int S, int K,
                                                           int D, float* __restrict__ sup, float* __restrict__ cnt) {
    extern __shared__ int vis_members[];           // indices s with ys == k, ascending
    __shared__ int n_members;
    __shared__ int wave_count[4];
    const int t = blockIdx.y, k = blockIdx.x;
    const int64_t* yt = ys + (size_t)t * S;
    if (threadIdx.x == 0) n_members = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63, n_waves = blockDim.x >> 6;
    for (int s0 = 0; s0 < S; s0 += blockDim.x) {   // order-preserving compaction of {s : y_s == k}
        const int s = s0 + threadIdx.x;
        const bool m = s < S && yt[s] == k;
        const unsigned long long bal = __ballot(m);
        if (wl == 0) wave_count[wave] = __popcll(bal);
        __syncthreads();
        int off = n_members;
        for (int w = 0; w < wave; w++) off += wave_count[w];
        if (m) vis_members[off + __popcll(bal & ((1ull << wl) - 1ull))] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < n_waves; w++) tot += wave_count[w];
            n_members += tot;
        }
        __syncthreads();
    }
    const int nm = n_members;
    const float* xt = xs + (size_t)t * S * D;
    const long ncols = (long)K * D;
    const int size_ilp = S >> 2;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const long col = (long)k * D + d;
        float r;
        if (outer_column_is_cascade(col, ncols)) {
            SparseCascade c(S);
            for (int i = 0; i < nm; i++) c.add(vis_members[i], xt[(size_t)vis_members[i] * D + d]);
            r = c.finish();
        } else {   // 4 interleaved cascades over s/4; the leftovers (s >= 4*(S/4)) join partial 0 after its cascade is complete
            SparseCascade c0(size_ilp), c1(size_ilp), c2(size_ilp), c3(size_ilp);
            bool has_extra = false;
            float p0 = 0.f;
            for (int i = 0; i < nm; i++) {
                const int s = vis_members[i];
                const float v = xt[(size_t)s * D + d];
                if (s >= size_ilp * 4) {
                    if (!has_extra) { p0 = c0.finish(); has_extra = true; }
                    p0 += v;
                } else {
                    const int m = s >> 2;
                    switch (s & 3) {
                        case 0: c0.add(m, v); break;
                        case 1: c1.add(m, v); break;
                        case 2: c2.add(m, v); break;
                        default: c3.add(m, v); break;
                    }
                }
            }
            if (!has_extra) p0 = c0.finish();
            p0 += c1.finish();
            p0 += c2.finish();
            p0 += c3.finish();
            r = p0;
        }
        sup[((size_t)t * K + k) * D + d] = r;
    }
    if (threadIdx.x == 0) cnt[(size_t)t * K + k] = (float)nm;
}

static void launch_vis_support_stats(hipStream_t st, const float* xs, const int64_t* ys, int T, int S, int K, int D, float* sup,
                                     float* cnt) {
    hipLaunchKernelGGL(k_vis_support_stats, dim3(K, T), dim3(256), (size_t)S * sizeof(int), st, xs, ys, S, K, D, sup, cnt);
}

static int check_visual_fs(const tclip_problem* p, int32_t dim, const char* who) {
    if (int rc = check_problem(p)) return rc;
    if (dim < 1 || dim > 1024) return fail(TCLIP_ERR_ARG, "dim must be in 1..1024");
    if (p->n_support < 1) return fail(TCLIP_ERR_ARG, "%s is a few-shot method: n_support must be positive", who);
    const size_t T = (size_t)p->n_batches * p->tasks_per_batch, R = (size_t)p->n_support + p->n_query;
    if (T * R * 16 > 0x7fffffffu || T * (size_t)dim > 0x7fffffffu)
        return fail(TCLIP_ERR_ARG, "%s: tasks * (n_support + n_query) * 16 and tasks * dim must fit in int32", who);
    return TCLIP_OK;
}

struct PaddleVisWs { size_t sup, cnt, cs, live, logit, total; };
static PaddleVisWs paddle_visual_ws(const tclip_problem& p, int D) {
    const size_t T = (size_t)p.n_batches * p.tasks_per_batch, K = p.n_class, Q = p.n_query;
    PaddleVisWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
    w.sup = take(T * K * D * 4);
    w.cnt = take(T * K * 4);
    w.cs = take(T * K * 4);
    w.live = take(T * K);
    w.logit = take(T * Q * K * 4);
    w.total = o;
    return w;
}

struct BdcspnVisWs { size_t zs, zq, zqn, mean, eta, sup, cnt, wn, aug, logit, cs, live, dummy, total; };
static BdcspnVisWs bdcspn_visual_ws(const tclip_problem& p, int dim) {
    const size_t T = (size_t)p.n_batches * p.tasks_per_batch, K = p.n_class, Q = p.n_query, S = p.n_support, R = S + Q, D = dim;
    BdcspnVisWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
    w.zs = take(T * S * D * 4);
    w.zq = take(T * Q * D * 4);
    w.zqn = take(T * Q * D * 4);
    w.mean = take(T * D * 4);
    w.eta = take(T * D * 4);
    w.sup = take(T * K * D * 4);
    w.cnt = take(T * K * 4);
    w.wn = take(T * K * D * 4);
    w.aug = take(T * R * D * 4);
    w.logit = take(T * R * K * 4);
    w.cs = take(T * K * 4);
    w.live = take(T * K);
    w.dummy = take(T * R * 4);
    w.total = o;
    return w;
}

}  // namespace tclip

extern "C" {

size_t tclip_paddle_visual_workspace_bytes(const tclip_problem* p, int32_t dim) {
    if (check_visual_fs(p, dim, "PADDLE") != TCLIP_OK) return 0;
    return paddle_visual_ws(*p, dim).total;
}

int tclip_paddle_visual_run(const tclip_problem* pp, int32_t dim, const float* x_q, const float* x_s, const int64_t* y_s,
                            float lambd, float* u, float* v, float* w, int32_t* preds, void* workspace, size_t workspace_bytes,
                            void* stream) {
    if (int rc = check_visual_fs(pp, dim, "PADDLE")) return rc;
    const tclip_problem p = *pp;
    if (!x_q || !x_s || !y_s || !u || !v || !w || !preds || !workspace) return fail(TCLIP_ERR_ARG, "null pointer argument");
    const PaddleVisWs o = paddle_visual_ws(p, dim);
    if (workspace_bytes < o.total) return fail(TCLIP_ERR_WORKSPACE, "workspace smaller than tclip_paddle_visual_workspace_bytes()");
    if (((uintptr_t)workspace & 255) != 0) return fail(TCLIP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int Q = p.n_query, K = p.n_class, D = dim, S = p.n_support, T = p.n_batches * p.tasks_per_batch, TK = T * K;
    float* sup = (float*)(ws + o.sup);
    float* cnt = (float*)(ws + o.cnt);
    float* cs = (float*)(ws + o.cs);
    uint8_t* live = (uint8_t*)(ws + o.live);
    float* logit0 = (float*)(ws + o.logit);
    // init (paddle.py:180-197): v = 0, w = class means of the support set (the text-prompt u is overwritten before it is read)
    hipLaunchKernelGGL(k_fill, dim3(ew_grid(TK)), dim3(256), 0, st, v, 0.0f, (size_t)TK);
    launch_vis_support_stats(st, x_s, y_s, T, S, K, D, sup, cnt);
    hipLaunchKernelGGL(k_div_rows, dim3(ew_grid((size_t)TK * D)), dim3(256), 0, st, (const float*)sup, (const float*)cnt,
                       (size_t)TK * D, D, w);
    TCLIP_HIP(hipMemsetAsync(live, 1, (size_t)TK, st));
    for (int it = 0; it < p.iters; it++) {
        // u_update (:105-116): softmax_k(-1/2 ||w_k - z_q||^2 + lambd v_k / Q); every centroid moves every iteration
        if (int rc = launch_vis_dist(T, st, w, x_q, live, Q, K, D, -0.5f, 1.0f, logit0)) return rc;
        hipLaunchKernelGGL(k_softmax, dim3((T * Q * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit0, (const float*)v,
                           T * Q, Q, K, lambd, 0, 0, u, preds);
        // v_update (:118-124) and w_update (:142-158)
        hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)u, T, Q, K, 0, cs, live, v,
                           (int32_t*)nullptr);
        launch_vis_mstats(st, u, x_q, cs, live, T, Q, K, D, 2, w, sup, cnt);
    }
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

size_t tclip_bdcspn_visual_workspace_bytes(const tclip_problem* p, int32_t dim) {
    if (check_visual_fs(p, dim, "BDCSPN") != TCLIP_OK) return 0;
    return bdcspn_visual_ws(*p, dim).total;
}

int tclip_bdcspn_visual_run(const tclip_problem* pp, int32_t dim, const float* x_q, const float* x_s, const int64_t* y_s, float temp,
                            int32_t norm_type, float* prototypes, float* u, int32_t* preds, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (int rc = check_visual_fs(pp, dim, "BDCSPN")) return rc;
    const tclip_problem p = *pp;
    if (!x_q || !x_s || !y_s || !prototypes || !u || !preds || !workspace) return fail(TCLIP_ERR_ARG, "null pointer argument");
    if (norm_type < 0 || norm_type > 2) return fail(TCLIP_ERR_ARG, "norm_type must be 0 (UN), 1 (L2N) or 2 (CL2N)");
    const BdcspnVisWs o = bdcspn_visual_ws(p, dim);
    if (workspace_bytes < o.total) return fail(TCLIP_ERR_WORKSPACE, "workspace smaller than tclip_bdcspn_visual_workspace_bytes()");
    if (((uintptr_t)workspace & 255) != 0) return fail(TCLIP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int Q = p.n_query, K = p.n_class, D = dim, S = p.n_support, R = S + Q, T = p.n_batches * p.tasks_per_batch, TK = T * K;
    const int TD = T * D;
    float* zs = (float*)(ws + o.zs);
    float* zq = (float*)(ws + o.zq);
    float* zqn = (float*)(ws + o.zqn);
    float* mean = (float*)(ws + o.mean);
    float* eta = (float*)(ws + o.eta);
    float* sup = (float*)(ws + o.sup);
    float* cnt = (float*)(ws + o.cnt);
    float* wn = (float*)(ws + o.wn);
    float* aug = (float*)(ws + o.aug);
    float* logit = (float*)(ws + o.logit);
    float* cs = (float*)(ws + o.cs);
    uint8_t* live = (uint8_t*)(ws + o.live);
    int32_t* dummy = (int32_t*)(ws + o.dummy);
    auto rows_grid = [](int n_rows) { return dim3((unsigned)(((size_t)n_rows * 8 + 255) / 256)); };
    auto normalize = [&](const float* x, const float* x2, int R0, int Rr, int mode, const float* mn, const float* sh, float* out) {
        hipLaunchKernelGGL(k_bdcspn_normalize, rows_grid(T * Rr), dim3(256), 0, st, x, x2, R0, Rr, D, mode, mn, sh, T * Rr, out);
    };
    // normalization (bdcspn.py:77-100, :165-166): train_mean = support.mean(1), an outer sum over D columns; CL2N / L2N / none
    if (norm_type == 2) hipLaunchKernelGGL(k_col_mean, dim3((TD + 255) / 256), dim3(256), 0, st, x_s, T, S, D, mean);
    normalize(x_s, x_s, S, S, norm_type, (const float*)mean, (const float*)nullptr, zs);
    normalize(x_q, x_q, Q, Q, norm_type, (const float*)mean, (const float*)nullptr, zq);
    // initial prototypes: support class means (:117-120), L2-normalised for get_logits (:50)
    launch_vis_support_stats(st, zs, y_s, T, S, K, D, sup, cnt);
    hipLaunchKernelGGL(k_div_rows, dim3(ew_grid((size_t)TK * D)), dim3(256), 0, st, (const float*)sup, (const float*)cnt,
                       (size_t)TK * D, D, prototypes);
    normalize((const float*)prototypes, (const float*)prototypes, K, K, 1, (const float*)nullptr, (const float*)nullptr, wn);
    // augmented set: support rows, then query rows shifted by eta = mean(support) - mean(query); normalised (:127-131, :51, :137)
    hipLaunchKernelGGL(k_bdcspn_eta, dim3((TD + 255) / 256), dim3(256), 0, st, (const float*)zs, (const float*)zq, T, S, Q, D, eta);
    normalize((const float*)zs, (const float*)zq, S, R, 1, (const float*)nullptr, (const float*)eta, aug);
    // soft assignment of the augmented set to the initial prototypes (:133-134)
    TCLIP_HIP(hipMemsetAsync(live, 1, (size_t)TK, st));
    if (int rc = launch_vis_dist(T, st, wn, aug, live, R, K, D, -0.5f, temp, logit)) return rc;
    hipLaunchKernelGGL(k_softmax, dim3((T * R * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit, (const float*)nullptr,
                       T * R, R, K, 0.0f, 0, 0, logit, dummy);
    // rectified prototypes = assignment-weighted means of the normalised augmented set (:137-141)
    hipLaunchKernelGGL(k_cluster_sizes, dim3((TK + 255) / 256), dim3(256), 0, st, (const float*)logit, T, R, K, 0, cs, live,
                       (float*)nullptr, (int32_t*)nullptr);
    launch_vis_mstats(st, logit, aug, cs, live, T, R, K, D, 3, prototypes);
    // prediction (:190-193): softmax(temp * get_logits(prototypes, query)), argmax
    normalize((const float*)prototypes, (const float*)prototypes, K, K, 1, (const float*)nullptr, (const float*)nullptr, wn);
    normalize((const float*)zq, (const float*)zq, Q, Q, 1, (const float*)nullptr, (const float*)nullptr, zqn);
    if (int rc = launch_vis_dist(T, st, wn, zqn, live, Q, K, D, -0.5f, temp, logit)) return rc;
    hipLaunchKernelGGL(k_softmax, dim3((T * Q * 16 + 255) / 256), dim3(256), 0, st, (const float*)logit, (const float*)nullptr,
                       T * Q, Q, K, 0.0f, 0, 0, u, preds);
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

}  // extern "C"
