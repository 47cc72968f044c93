// Device half of the cluster-to-class matching (include/tclip.h: tclip_match_clusters): included at the end of
// tclip_kernels.hip, uses its helpers (fail, TCLIP_HIP).  A restatement for one wavefront of assign_rows + match_range of
// tclip_host.cpp - the shortest-augmenting-path solver of D. F. Crouse, "On implementing 2D rectangular assignment
// algorithms", IEEE TAES 52(4), 2016, as scipy.optimize.linear_sum_assignment runs it - with the host's bits:
//   - the arithmetic is fp64 additions and comparisons on -(double)prototype in the host's expression order
//     ((min_val + cost) - u[i]) - v[j]; every dist / u / v element is computed by one lane from the same operands, so
//     spreading the columns over the lanes changes no bit;
//   - the one order-dependent step is the pick of the next column.  The host scans the CURRENT order of its `todo` list
//     (cols-1 .. 0 at the start of a row, permuted by swap-with-last on removal) and keeps, among the columns at the minimum
//     dist, the LAST unassigned one in scan order if one is unassigned and the FIRST column otherwise.  The list lives in LDS,
//     is removed from exactly as the host removes, and the wavefront reduces the key (dist, unassigned, position) under that
//     rule - a total order, so the shape of the reduction tree does not matter.
// One task per workgroup of ONE wavefront: the inner step (scan the remaining columns, reduce, remove one) runs up to C^2/2
// times per task and needs the lanes to agree after every one of them; within a wavefront that agreement is a cross-lane
// reduction and an LDS wait, across wavefronts it would be a workgroup barrier per step.  Calls carry hundreds to thousands of
// tasks, so the machine is filled across tasks.  The cost row of the current cluster is read from `prototypes` in global
// memory (the remaining columns are a permutation of a contiguous range: whole cache lines are used); it is not staged.
//
// No label is used as an index unchecked: a cluster count outside 1..c_stride, a cluster id or a prediction outside 0..K-1
// and an infeasible assignment (minimum dist == INFINITY, e.g. a NaN prototype row) fail THAT task - status != 0, acc = NaN,
// new_preds = -1 - where the host entry returns TCLIP_ERR_ARG for the whole call.

namespace tclip {

constexpr int kMatchBadCount = 1, kMatchBadId = 2, kMatchBadPred = 3, kMatchInfeasible = 4;     // status[t]

// LDS of one task: v, dist [K] f64 and u [Cs] f64; pred, row_of_col, todo [K] i32 and col_of_row [Cs] i32; col_seen [K] and
// row_seen [Cs] bytes (Cs = c_stride).  29 K + 13 Cs bytes: 42 KB at K = Cs = 1024, 30.6 KB at K = 1024 with 75 queries.
static size_t match_lds_bytes(int K, int Cs) { return (size_t)29 * K + (size_t)13 * Cs; }

__device__ __forceinline__ int match_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(64) void k_match_clusters(int Q, int K, int Cs, const int32_t* __restrict__ preds,
                                                       const int32_t* __restrict__ n_clusters,
                                                       const int32_t* __restrict__ cluster_ids,
                                                       const float* __restrict__ prototypes, const int64_t* __restrict__ y_q,
                                                       int graph_matching, int32_t* __restrict__ new_preds,
                                                       float* __restrict__ acc, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char match_smem[];
    double* v = (double*)match_smem;
    double* dist = v + K;
    double* u = dist + K;
    int* pred = (int*)(u + Cs);
    int* row_of_col = pred + K;
    int* todo = row_of_col + K;
    int* col_of_row = todo + K;
    unsigned char* col_seen = (unsigned char*)(col_of_row + Cs);
    unsigned char* row_seen = col_seen + K;

    const int t = blockIdx.x, lane = threadIdx.x;
    const int32_t* p_t = preds + (size_t)t * Q;
    const int32_t* ids = cluster_ids + (size_t)t * Cs;
    const float* pr = prototypes + (size_t)t * Cs * K;
    const int C = n_clusters[t];

    // the host's checks (match_range), every one uniform over the wavefront
    int bad = (C < 1 || C > Cs) ? kMatchBadCount : 0;
    if (!bad) {
        bool b = false;
        for (int c = lane; c < C; c += 64) b |= ids[c] < 0 || ids[c] >= K;
        if (__ballot(b) != 0ull) bad = kMatchBadId;
    }
    if (!bad) {
        bool b = false;
        for (int q = lane; q < Q; q += 64) b |= p_t[q] < 0 || p_t[q] >= K;
        if (__ballot(b) != 0ull) bad = kMatchBadPred;
    }

    if (!bad && graph_matching) {
        for (int j = lane; j < K; j += 64) { v[j] = 0.0; row_of_col[j] = -1; }
        for (int r = lane; r < C; r += 64) { u[r] = 0.0; col_of_row[r] = -1; }
        for (int cur = 0; cur < C && !bad; cur++) {
            for (int j = lane; j < K; j += 64) { todo[j] = K - j - 1; dist[j] = INFINITY; col_seen[j] = 0; }
            for (int r = lane; r < C; r += 64) row_seen[r] = 0;
            __syncthreads();
            int n_todo = K, i = cur, sink = -1;
            double min_val = 0.0;
            while (sink < 0) {
                const double ui = u[i];
                const float* row = pr + (size_t)i * K;
                // key of the pick: dist, then s = K + position for an unassigned column (the last one wins), K - 1 - position
                // for an assigned one (the first one wins, and any unassigned column beats it); larger s is better
                double bd = INFINITY;
                int bs = -1;
                for (int it = lane; it < n_todo; it += 64) {
                    const int j = todo[it];
                    const double r = ((min_val + (-(double)row[j])) - ui) - v[j];
                    double dj = dist[j];
                    if (r < dj) { pred[j] = i; dist[j] = r; dj = r; }
                    const int s = row_of_col[j] == -1 ? K + it : K - 1 - it;
                    if (dj < bd || (dj == bd && s > bs)) { bd = dj; bs = s; }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const double od = __shfl_xor(bd, o);
                    const int os = __shfl_xor(bs, o);
                    if (od < bd || (od == bd && os > bs)) { bd = od; bs = os; }
                }
                // every lane holds the same key now; through scalar registers, so that the loop's control flow is scalar too
                bs = __builtin_amdgcn_readfirstlane(bs);
                bd = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(bd)),
                                      __builtin_amdgcn_readfirstlane(__double2loint(bd)));
                min_val = bd;
                if (!(bd < INFINITY)) { bad = kMatchInfeasible; break; }
                const int pick = bs >= K ? bs - K : K - 1 - bs;
                const int j = __builtin_amdgcn_readfirstlane(todo[pick]), owner = __builtin_amdgcn_readfirstlane(row_of_col[j]);
                const int last = todo[n_todo - 1];
                __syncthreads();                                  // every lane has read todo[pick] and its dist / pred are written
                if (lane == 0) { row_seen[i] = 1; col_seen[j] = 1; todo[pick] = last; }
                n_todo--;
                if (owner == -1) sink = j;
                else i = owner;
                __syncthreads();
            }
            if (bad) break;
            // dual updates, as written on the host
            for (int r = lane; r < C; r += 64) {
                if (r == cur) u[r] += min_val;
                else if (row_seen[r]) u[r] += min_val - dist[col_of_row[r]];
            }
            for (int j = lane; j < K; j += 64)
                if (col_seen[j]) v[j] -= min_val - dist[j];
            __syncthreads();
            if (lane == 0) {                                      // augment: at most cur + 1 rows lie on the path
                int j = sink;
                for (int step = 0; step <= cur; step++) {
                    const int r = pred[j];
                    row_of_col[j] = r;
                    const int old = col_of_row[r];
                    col_of_row[r] = j;
                    j = old;
                    if (r == cur) break;
                }
            }
            __syncthreads();
        }
    } else if (!bad) {
        // compute_basic_matching: the first maximum of the cluster's prototype row, by the host's scan (`>` from element 0:
        // a NaN never replaces the running best, and a NaN in element 0 is never replaced)
        for (int c = 0; c < C; c++) {
            const float* row = pr + (size_t)c * K;
            float bv = -INFINITY;
            int bi = K;
            for (int d = lane; d < K; d += 64) {
                const float x = row[d];
                if (x > bv || (x == bv && d < bi)) { bv = x; bi = d; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            const float first = row[0];
            if (first != first || bi >= K) bi = 0;
            if (lane == 0) col_of_row[c] = bi;
        }
        __syncthreads();
    }

    if (bad) {
        for (int q = lane; q < Q; q += 64) new_preds[(size_t)t * Q + q] = -1;
        if (lane == 0) { acc[t] = __builtin_nanf(""); status[t] = bad; }
        return;
    }

    // look-up table label -> class; labels that name no cluster map to 0 and a repeated id keeps its last cluster, as the
    // host's sequential fill does
    int* lut = todo;
    int* last_cluster = pred;
    for (int j = lane; j < K; j += 64) { lut[j] = 0; last_cluster[j] = -1; }
    __syncthreads();
    for (int c = lane; c < C; c += 64) atomicMax(&last_cluster[ids[c]], c);
    __syncthreads();
    for (int c = lane; c < C; c += 64)
        if (last_cluster[ids[c]] == c) lut[ids[c]] = col_of_row[c];
    __syncthreads();
    int hit = 0;
    for (int q = lane; q < Q; q += 64) {
        const int np = lut[p_t[q]];
        new_preds[(size_t)t * Q + q] = np;
        hit += (int64_t)np == y_q[(size_t)t * Q + q];
    }
    hit = match_wave_sum(hit);
    // torch: (new == y).float().mean(1): sum of 0/1 floats (exact) divided by Q in fp32
    if (lane == 0) { acc[t] = (float)hit / (float)Q; status[t] = 0; }
}

}  // namespace tclip

extern "C" {

size_t tclip_match_clusters_workspace_bytes(int32_t T, int32_t Q, int32_t K, int32_t c_stride) {
    (void)T; (void)Q; (void)K; (void)c_stride;
    return 0;                                  // everything a task needs lives in LDS
}

int tclip_match_clusters(int32_t T, int32_t Q, int32_t K, const int32_t* preds, const int32_t* n_clusters,
                         const int32_t* cluster_ids, const float* prototypes, const int64_t* y_q, int32_t graph_matching,
                         int32_t c_stride, int32_t* new_preds, float* acc, int32_t* status, void* workspace,
                         size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;    // tclip_match_clusters_workspace_bytes() == 0: nothing to check
    if (T < 1 || Q < 1) return fail(TCLIP_ERR_ARG, "tclip_match_clusters: n_task and n_query must be >= 1");
    if (K < 2 || K > 1024) return fail(TCLIP_ERR_ARG, "tclip_match_clusters: n_class must be in 2..1024");
    if (c_stride < 1 || c_stride > (Q < K ? Q : K))
        return fail(TCLIP_ERR_ARG, "tclip_match_clusters: c_stride must be in 1..min(n_query, n_class)");
    if (!preds || !n_clusters || !cluster_ids || !prototypes || !y_q || !new_preds || !acc || !status)
        return fail(TCLIP_ERR_ARG, "tclip_match_clusters: null pointer");
    hipLaunchKernelGGL(k_match_clusters, dim3(T), dim3(64), match_lds_bytes(K, c_stride), (hipStream_t)stream, Q, K, c_stride,
                       preds, n_clusters, cluster_ids, prototypes, y_q, graph_matching != 0 ? 1 : 0, new_preds, acc, status);
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

}  // extern "C"
