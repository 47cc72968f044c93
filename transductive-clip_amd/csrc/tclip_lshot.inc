// LAPLACIAN_SHOT (SURVEY.md F4; reference: src/methods/few_shot/laplacian_shot.py) on probability features: included at
// the end of tclip_kernels.hip, uses its helpers (fail, check_problem, align_up, k_support_stats, k_div_rows).
//
// Per task: L2-normalised features, prototypes = support class means, unary[q][k] = ||proto_k - z_q||^2, a kNN graph
// over the task's queries (W[i][j] = 1 for the knn-1 nearest other queries j of i), then `iter` bound updates
//   Y <- softmax_k(-unary + lmd * W Y)            (fp64 after the first, fp32 start: laplacian_shot.py:142-154)
// with the energy  sum Y log max(Y, 1e-20) + unary Y - lmd (W Y) Y  and the reference's freeze rule
// (|E - E_old| <= 1e-6 |E_old| after the third update: the assignment and the energy are repeated from then on).
// The reference computes this with numpy / scipy.sparse / sklearn on the host, one task after the other; here a
// workgroup owns a task.  numpy's pairwise sums, its exp and sklearn's distance kernels are not reproduced bit for bit:
// like ALPHA_TIM this method is pinned to reference-made fixtures through its assignments, neighbour lists and
// energies within a tolerance.

namespace tclip {

constexpr int kLshotWaves = 8;
constexpr int kLshotMaxQ = 1024;          // a lane keeps ceil(Q / 64) distances while it selects neighbours

__device__ __forceinline__ double lshot_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// out = x / ||x||_2 row by row (mode 1, laplacian_shot.py:83-85) or a plain copy (mode 0, 'UN').
__global__ void k_lshot_normalize(const float* __restrict__ x, int n_rows, int K, int mode, float* __restrict__ out) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const float* r = x + (size_t)row * K;
    float nrm = 1.0f;
    if (mode == 1) {
        double s = 0.0;
        for (int d = lane; d < K; d += 64) s += (double)r[d] * (double)r[d];
        s = lshot_wave_sum(s);
        nrm = (float)sqrt(s);
    }
    for (int d = lane; d < K; d += 64) out[(size_t)row * K + d] = mode == 1 ? r[d] / nrm : r[d];
}

// unary[t][q][k] = ||proto[t][k] - z[t][q]||^2 (the reference squares LA.norm's fp32 square root, :236-238).
// One workgroup per query (its row staged in LDS), one class per wavefront at a time, lanes over the features
// (coalesced prototype reads, fp64 accumulation, one wavefront reduction per class).
__global__ __launch_bounds__(256) void k_lshot_unary(const float* __restrict__ proto, const float* __restrict__ zq, int Q, int K,
                                                     float* __restrict__ unary) {
    extern __shared__ float zrow[];                                  // the query row, K floats
    const int t = blockIdx.y, q = blockIdx.x;
    const float* z = zq + ((size_t)t * Q + q) * K;
    for (int d = threadIdx.x; d < K; d += blockDim.x) zrow[d] = z[d];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
    for (int k = wave; k < K; k += n_waves) {                         // one class per wavefront, lanes over features
        const float* p = proto + ((size_t)t * K + k) * K;
        double s = 0.0;
        for (int d = lane; d < K; d += 64) {
            const float diff = p[d] - zrow[d];
            s += (double)diff * (double)diff;
        }
        s = lshot_wave_sum(s);
        if (lane == 0) {
            const float dist = (float)sqrt(s);
            unary[((size_t)t * Q + q) * K + k] = dist * dist;
        }
    }
}

struct LshotArgs {
    const float* zq;          // [T][Q][K] normalised queries
    const float* unary;       // [T][Q][K]
    double* ybuf;             // [T][2][Q][K]
    int32_t* neighbours;      // [T][Q][knn-1] out
    int32_t* preds_iter;      // [T][iters][Q] out
    double* energies;         // [T][iters] out
    int Q, K, knn, iters;
    double lmd;
};

// One workgroup per task: kNN graph, then the bound updates.
__global__ __launch_bounds__(64 * kLshotWaves) void k_lshot_task(LshotArgs a) {
    extern __shared__ char lshot_smem[];
    const int Q = a.Q, K = a.K, nn = a.knn - 1, t = blockIdx.x;
    int* nbr = reinterpret_cast<int*>(lshot_smem);                     // [Q][nn]
    double* row_e = reinterpret_cast<double*>(lshot_smem + (((size_t)Q * nn * sizeof(int) + 7) & ~(size_t)7));   // [Q]
    __shared__ int frozen;
    __shared__ double e_old;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* zq = a.zq + (size_t)t * Q * K;
    const float* unary = a.unary + (size_t)t * Q * K;
    double* y0 = a.ybuf + (size_t)t * 2 * Q * K;
    double* y1 = y0 + (size_t)Q * K;

    // ---- kNN over the task's queries (create_affinity, :91-101): squared distances in fp64, the nn nearest others,
    // ties to the lower index (exact ties do not occur between distinct images)
    for (int i = wave; i < Q; i += kLshotWaves) {
        double d2[kLshotMaxQ / 64];
        const float* zi = zq + (size_t)i * K;
#pragma unroll
        for (int e = 0; e < kLshotMaxQ / 64; e++) {
            const int j = e * 64 + lane;
            d2[e] = INFINITY;
            if (e * 64 < Q && j < Q && j != i) {
                const float* zj = zq + (size_t)j * K;
                double s = 0.0;
                for (int d = 0; d < K; d++) {
                    const double diff = (double)zi[d] - (double)zj[d];
                    s += diff * diff;
                }
                d2[e] = s;
            }
        }
        for (int r = 0; r < nn; r++) {
            double best = INFINITY;
            int arg = 0x7fffffff;
#pragma unroll
            for (int e = 0; e < kLshotMaxQ / 64; e++)
                if (d2[e] < best) { best = d2[e]; arg = e * 64 + lane; }
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o);
                const int oa = __shfl_xor(arg, o);
                if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
            }
#pragma unroll
            for (int e = 0; e < kLshotMaxQ / 64; e++)
                if (e * 64 + lane == arg) d2[e] = INFINITY;
            if (arg >= Q) arg = i;                                    // only with NaN features: stay inside the task
            if (lane == 0) {
                nbr[i * nn + r] = arg;
                a.neighbours[((size_t)t * Q + i) * nn + r] = arg;
            }
        }
    }
    // ---- Y = normalize(-unary), fp32 as in the reference (:143)
    for (int q = wave; q < Q; q += kLshotWaves) {
        const float* u = unary + (size_t)q * K;
        float mx = -INFINITY;
        for (int k = lane; k < K; k += 64) mx = fmaxf(mx, -u[k]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float s = 0.0f;
        for (int k = lane; k < K; k += 64) s += expf(-u[k] - mx);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        for (int k = lane; k < K; k += 64) y0[(size_t)q * K + k] = (double)(expf(-u[k] - mx) / s);
    }
    if (threadIdx.x == 0) {
        frozen = 0;
        e_old = INFINITY;
    }
    __syncthreads();

    double* yold = y0;
    double* ynew = y1;
    int it = 0;
    for (; it < a.iters; it++) {
        // Y_new[q] = softmax_k(-unary[q] + lmd * sum_{j in nbr(q)} Y_old[j])                                (:150-154)
        for (int q = wave; q < Q; q += kLshotWaves) {
            const float* u = unary + (size_t)q * K;
            double mx = -INFINITY;
            int arg = 0x7fffffff;
            for (int k = lane; k < K; k += 64) {
                double m = 0.0;
                for (int r = 0; r < nn; r++) m += yold[(size_t)nbr[q * nn + r] * K + k];
                const double add = -(double)u[k] - (-a.lmd * m);
                ynew[(size_t)q * K + k] = add;
                if (add > mx) { mx = add; arg = k; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double om = __shfl_xor(mx, o);
                const int oa = __shfl_xor(arg, o);
                if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
            }
            double s = 0.0;
            for (int k = lane; k < K; k += 64) {
                const double e = exp(ynew[(size_t)q * K + k] - mx);
                ynew[(size_t)q * K + k] = e;
                s += e;
            }
            s = lshot_wave_sum(s);
            for (int k = lane; k < K; k += 64) ynew[(size_t)q * K + k] /= s;
            if (lane == 0) a.preds_iter[((size_t)t * a.iters + it) * Q + q] = arg < K ? arg : 0;   // argmax of Y = argmax of its logits (0 for a NaN row)
        }
        __syncthreads();
        // E = sum Y log max(Y, 1e-20) + unary Y - lmd (W Y) Y, with the NEW Y on both sides of W                 (:120-126)
        for (int q = wave; q < Q; q += kLshotWaves) {
            const float* u = unary + (size_t)q * K;
            double e = 0.0;
            for (int k = lane; k < K; k += 64) {
                const double y = ynew[(size_t)q * K + k];
                double m = 0.0;
                for (int r = 0; r < nn; r++) m += ynew[(size_t)nbr[q * nn + r] * K + k];
                e += y * log(fmax(y, 1e-20)) + ((double)u[k] * y + (-a.lmd * m * y));
            }
            e = lshot_wave_sum(e);
            if (lane == 0) row_e[q] = e;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double e = 0.0;
            for (int q = 0; q < Q; q++) e += row_e[q];
            a.energies[(size_t)t * a.iters + it] = e;
            if (it > 1 && fabs(e - e_old) <= 1e-6 * fabs(e_old)) frozen = 1;          // (:162)
            else e_old = e;
        }
        __syncthreads();
        double* sw = yold;
        yold = ynew;
        ynew = sw;
        if (frozen) break;
    }
    // frozen: the assignment and the energy of update `it` are repeated for the remaining entries               (:164-171)
    if (it < a.iters) {
        for (int j = it + 1; j < a.iters; j++) {
            for (int q = threadIdx.x; q < Q; q += blockDim.x)
                a.preds_iter[((size_t)t * a.iters + j) * Q + q] = a.preds_iter[((size_t)t * a.iters + it) * Q + q];
            if (threadIdx.x == 0) a.energies[(size_t)t * a.iters + j] = a.energies[(size_t)t * a.iters + it];
        }
    }
}

struct LshotWs { size_t zs, zq, sup, cnt, proto, ybuf, total; };
static LshotWs lshot_ws(const tclip_problem& p) {
    const size_t T = (size_t)p.n_batches * p.tasks_per_batch, K = p.n_class, Q = p.n_query, S = p.n_support;
    LshotWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
    w.zs = take(T * S * K * 4);
    w.zq = take(T * Q * K * 4);
    w.sup = take(T * K * K * 4);
    w.cnt = take(T * K * 4);
    w.proto = take(T * K * K * 4);
    w.ybuf = take(T * 2 * Q * K * 8);
    w.total = o;
    return w;
}

}  // namespace tclip

extern "C" {

size_t tclip_laplacian_shot_workspace_bytes(const tclip_problem* p) {
    if (check_problem(p) != TCLIP_OK) return 0;
    return lshot_ws(*p).total;
}

int tclip_laplacian_shot_run(const tclip_problem* pp, const float* x_q, const float* x_s, const int64_t* y_s, int32_t knn,
                             double lmd, int32_t norm_type, float* unary, int32_t* neighbours, int32_t* preds_iter,
                             double* energies, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_problem(pp)) return rc;
    const tclip_problem p = *pp;
    if (p.iters < 1) return fail(TCLIP_ERR_ARG, "LAPLACIAN_SHOT needs iters >= 1");
    if (!x_q || !x_s || !y_s || !unary || !neighbours || !preds_iter || !energies || !workspace)
        return fail(TCLIP_ERR_ARG, "null pointer argument");
    if (p.n_support < 1) return fail(TCLIP_ERR_ARG, "LAPLACIAN_SHOT is a few-shot method: n_support must be positive");
    if (norm_type != 0 && norm_type != 1) return fail(TCLIP_ERR_ARG, "norm_type must be 0 (UN) or 1 (L2N); CL2N needs a train mean the reference never passes");
    if (knn < 2 || knn > p.n_query) return fail(TCLIP_ERR_ARG, "knn must be in 2..n_query (the nearest neighbour of a query is the query itself)");
    if (p.n_query > kLshotMaxQ) return fail(TCLIP_ERR_ARG, "n_query must be <= 1024 for LAPLACIAN_SHOT");
    const LshotWs o = lshot_ws(p);
    if (int rc = check_workspace(workspace, workspace_bytes, o.total, "tclip_laplacian_shot_workspace_bytes")) return rc;
    const size_t smem = (((size_t)p.n_query * (knn - 1) * sizeof(int) + 7) & ~(size_t)7) + (size_t)p.n_query * sizeof(double);
    if (smem > 60000) return fail(TCLIP_ERR_ARG, "n_query * knn too large for the neighbour lists in LDS");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int Q = p.n_query, K = p.n_class, S = p.n_support, T = p.n_batches * p.tasks_per_batch, TK = T * K;
    float* zs = (float*)(ws + o.zs);
    float* zq = (float*)(ws + o.zq);
    float* sup = (float*)(ws + o.sup);
    float* cnt = (float*)(ws + o.cnt);
    float* proto = (float*)(ws + o.proto);
    // normalization (:66-89), prototypes = class means of the normalised support (:201-205)
    hipLaunchKernelGGL(k_lshot_normalize, dim3((T * S + 3) / 4), dim3(256), 0, st, x_s, T * S, K, norm_type, zs);
    hipLaunchKernelGGL(k_lshot_normalize, dim3((T * Q + 3) / 4), dim3(256), 0, st, x_q, T * Q, K, norm_type, zq);
    hipLaunchKernelGGL(k_support_stats, dim3(K, T), dim3(128), (size_t)S * sizeof(int), st, dense_rows(zs), y_s, S, K, 0, sup, cnt);
    hipLaunchKernelGGL(k_div_rows, dim3(ew_grid((size_t)TK * K)), dim3(256), 0, st, (const float*)sup, (const float*)cnt,
                       (size_t)TK * K, K, proto);
    hipLaunchKernelGGL(k_lshot_unary, dim3(Q, T), dim3(256), (size_t)K * sizeof(float), st, (const float*)proto, (const float*)zq, Q, K, unary);
    const LshotArgs a{zq, unary, (double*)(ws + o.ybuf), neighbours, preds_iter, energies, Q, K, knn, p.iters, lmd};
    hipLaunchKernelGGL(k_lshot_task, dim3(T), dim3(64 * kLshotWaves), smem, st, a);
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

}  // extern "C"
