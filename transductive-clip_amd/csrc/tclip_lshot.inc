// LAPLACIAN_SHOT (SURVEY.md F4; reference: src/methods/few_shot/laplacian_shot.py) on rows of any length: included at
// the end of tclip_kernels.hip after tclip_tim.inc, uses its helpers (fail, check_problem, align_up, k_support_stats, k_div_rows)
// and launch_vis_support_stats of tclip_visual_fs.inc.  A feature row has D elements, D carried separately from the class
// count K: rows, prototypes and the kNN distances live in D, the unary term, Y and everything after the kNN step in K.
// tclip_laplacian_shot_run is the probability-feature entry (D = K, distances inside k_lshot_task as before),
// tclip_laplacian_shot_visual_run the one for D-dim embeddings (any D in 1..1024; distances by k_lshot_pairdist).
// tclip_laplacian_shot[_visual]_run_tasks are the same two fed from the feature tables: k_lshot_normalize reads the task rows
// in place through a RowSrc, everything after it is shared.
// tclip_laplacian_shot_sweep_tasks solves the same tasks for a list of lmd values: everything up to the kNN graph once per task
// (k_lshot_knn), the updates on a grid of (task, value) (k_lshot_sweep_updates); lshot_knn_rows and lshot_solve are the code
// k_lshot_task runs, so every value's slice holds the single-value entry's bits.
// Host side: lshot_ws lays the workspace out for every form, lshot_entry is the one function behind the five entries (their
// form as a Rows of tclip_tim.inc; DESIGN.md, "The method host drivers"), lshot_run the launch sequence.
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
// kIdx: row `row` is table row x.idx[row], its element d table column x.cols[(row / rows_per_task) D + d] (x.cols == nullptr:
// d) - the task rows read in place.  A lane still owns the elements d = lane, lane + 64, ...: same values, same sums; the
// permuted loads stay inside one table row of at most 4 KB and the stores stay coalesced.
template <bool kIdx>
__global__ void k_lshot_normalize(RowSrc x, int rows_per_task, int n_rows, int D, int mode, float* __restrict__ out) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const float* r = kIdx ? x.base + (size_t)x.idx[row] * D : x.base + (size_t)row * D;
    const int32_t* c = (kIdx && x.cols) ? x.cols + (size_t)(row / rows_per_task) * D : nullptr;
    auto get = [&](int d) { return r[(kIdx && c) ? c[d] : d]; };
    float nrm = 1.0f;
    if (mode == 1) {
        double s = 0.0;
        for (int d = lane; d < D; d += 64) s += (double)get(d) * (double)get(d);
        s = lshot_wave_sum(s);
        nrm = (float)sqrt(s);
    }
    for (int d = lane; d < D; d += 64) out[(size_t)row * D + d] = mode == 1 ? get(d) / nrm : get(d);
}

// unary[t][q][k] = ||proto[t][k] - z[t][q]||^2 (the reference squares LA.norm's fp32 square root, :236-238).
// proto [T][K][D], zq [T][Q][D] -> unary [T][Q][K].
// One workgroup per query (its row staged in LDS), one class per wavefront at a time, lanes over the features
// (coalesced prototype reads, fp64 accumulation, one wavefront reduction per class).
__global__ __launch_bounds__(256) void k_lshot_unary(const float* __restrict__ proto, const float* __restrict__ zq, int Q, int K,
                                                     int D, float* __restrict__ unary) {
    extern __shared__ float zrow[];                                  // the query row, D floats
    const int t = blockIdx.y, q = blockIdx.x;
    const float* z = zq + ((size_t)t * Q + q) * D;
    for (int d = threadIdx.x; d < D; d += blockDim.x) zrow[d] = z[d];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
    for (int k = wave; k < K; k += n_waves) {                         // one class per wavefront, lanes over features
        const float* p = proto + ((size_t)t * K + k) * D;
        double s = 0.0;
        for (int d = lane; d < D; d += 64) {
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

// d2[t][i][j] = sum_d ((double)z[t][i][d] - (double)z[t][j][d])^2 over a task's queries, +inf on the diagonal: the distances the
// kNN selection of k_lshot_task reads when rows are long (the visual entry; at D = 512..1024 the per-lane serial loop inside
// the one workgroup that owns a task is the method's hot path, with uncoalesced reads).
// Grid (row tile, task): a task's Q x Q distances spread over ceil(Q / 32) workgroups.  A block owns 32 rows i and walks the
// column tiles of 32 rows j; per column tile both 32-row tiles are staged in LDS in chunks of 64 features (row-contiguous,
// coalesced; one 128-bit load per thread and tile where D is a multiple of 4: every row then starts 16-byte aligned, zq being a
// 256-byte aligned workspace offset).  The 16 x 16 threads each own a 2 x 2 register tile (i = ty + 16 a, j = tx + 16 b) and
// accumulate in fp64 in ascending d - the operation order of k_lshot_task's own loop, so both give the same bits.
// LDS rows are padded to 65 floats: the 16 rows j a wavefront reads at one d fall into 16 different banks, its 4 rows i
// are broadcasts.  2 x 32 x 65 x 4 = 16640 bytes of LDS, 4 fp64 accumulators, no scratch.
constexpr int kLshotPdTile = 32, kLshotPdChunk = 64, kLshotPdStride = kLshotPdChunk + 1;

__global__ __launch_bounds__(256) void k_lshot_pairdist(const float* __restrict__ zq, int Q, int D, double* __restrict__ d2) {
    __shared__ float zi[kLshotPdTile][kLshotPdStride];
    __shared__ float zj[kLshotPdTile][kLshotPdStride];
    const int t = blockIdx.y, i0 = blockIdx.x * kLshotPdTile, id = threadIdx.x, tx = id & 15, ty = id >> 4;
    const float* z = zq + (size_t)t * Q * D;
    double* out = d2 + (size_t)t * Q * Q;
    const bool vec = (D & 3) == 0;                                    // block-uniform
    // a 32 x 64 tile of rows r0.. and features d0..: rows past Q and features past D read as zero (never stored, never summed)
    auto stage = [&](float (*dst)[kLshotPdStride], int r0, int d0) {
        if (vec) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int idx = id + 256 * h, r = idx >> 4, c = (idx & 15) * 4;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (r0 + r < Q && d0 + c < D) v = *reinterpret_cast<const float4*>(z + (size_t)(r0 + r) * D + d0 + c);
                dst[r][c] = v.x; dst[r][c + 1] = v.y; dst[r][c + 2] = v.z; dst[r][c + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int h = 0; h < 8; h++) {
                const int idx = id + 256 * h, r = idx >> 6, c = idx & 63;
                dst[r][c] = (r0 + r < Q && d0 + c < D) ? z[(size_t)(r0 + r) * D + d0 + c] : 0.0f;
            }
        }
    };
    for (int j0 = 0; j0 < Q; j0 += kLshotPdTile) {
        double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;
        for (int d0 = 0; d0 < D; d0 += kLshotPdChunk) {
            __syncthreads();                                          // the previous chunk has been read
            stage(zi, i0, d0);
            stage(zj, j0, d0);
            __syncthreads();
            const int dn = min(kLshotPdChunk, D - d0);
            for (int d = 0; d < dn; d++) {
                const double a0 = (double)zi[ty][d], a1 = (double)zi[ty + 16][d];
                const double b0 = (double)zj[tx][d], b1 = (double)zj[tx + 16][d];
                double diff = a0 - b0;
                s00 += diff * diff;
                diff = a0 - b1;
                s01 += diff * diff;
                diff = a1 - b0;
                s10 += diff * diff;
                diff = a1 - b1;
                s11 += diff * diff;
            }
        }
        const int ia = i0 + ty, ib = ia + 16, ja = j0 + tx, jb = ja + 16;
        if (ia < Q && ja < Q) out[(size_t)ia * Q + ja] = ia == ja ? (double)INFINITY : s00;
        if (ia < Q && jb < Q) out[(size_t)ia * Q + jb] = ia == jb ? (double)INFINITY : s01;
        if (ib < Q && ja < Q) out[(size_t)ib * Q + ja] = ib == ja ? (double)INFINITY : s10;
        if (ib < Q && jb < Q) out[(size_t)ib * Q + jb] = ib == jb ? (double)INFINITY : s11;
    }
}

struct LshotArgs {
    const float* zq;          // [T][Q][D] normalised queries
    const double* d2;         // [T][Q][Q] from k_lshot_pairdist, or nullptr: the distances are computed in k_lshot_task
    const float* unary;       // [T][Q][K]
    double* ybuf;             // [T][2][Q][K]
    int32_t* neighbours;      // [T][Q][knn-1] out
    int32_t* preds_iter;      // [T][iters][Q] out
    double* energies;         // [T][iters] out
    int Q, K, D, knn, iters;
    double lmd;
};

// The kNN lists of the query rows i = first, first + step, ... of one task, one wavefront per row (create_affinity, :91-101):
// squared distances in fp64 (computed here, or read from k_lshot_pairdist's table `pd`: coalesced, a lane's 64-strided columns
// of row i), the nn nearest others, ties to the lower index (exact ties do not occur between distinct images).  A row's list
// depends on that row alone, so which wavefront of which block takes it changes nothing.  nbr_lds [Q][nn] (or nullptr) and
// nbr_out [Q][nn] are this task's lists.
__device__ __forceinline__ void lshot_knn_rows(const float* zq, const double* pd, int Q, int D, int nn, int first, int step, int lane,
                                               int* nbr_lds, int32_t* nbr_out) {
    for (int i = first; i < Q; i += step) {
        double d2[kLshotMaxQ / 64];
        const float* zi = zq + (size_t)i * D;
#pragma unroll
        for (int e = 0; e < kLshotMaxQ / 64; e++) {
            const int j = e * 64 + lane;
            d2[e] = INFINITY;
            if (e * 64 < Q && j < Q && j != i) {
                if (pd) {
                    d2[e] = pd[(size_t)i * Q + j];
                    continue;
                }
                const float* zj = zq + (size_t)j * D;
                double s = 0.0;
                for (int d = 0; d < D; d++) {
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
                if (nbr_lds) nbr_lds[i * nn + r] = arg;
                nbr_out[(size_t)i * nn + r] = arg;
            }
        }
    }
}

// One solve by one workgroup of kLshotWaves wavefronts, the neighbour lists nbr [Q][nn] already in LDS: Y = normalize(-unary),
// then the bound updates with their energies, the freeze rule and the tail fill.  k_lshot_task (one value) and
// k_lshot_sweep_updates (a list of values) both call this, so both compile the same expressions.
// unary [Q][K], y0 / y1 [Q][K] each, preds_iter [iters][Q] and energies [iters] are this solve's; row_e [Q], frozen and e_old
// are the block's LDS.
__device__ __forceinline__ void lshot_solve(const float* unary, const int* nbr, double* row_e, int* frozen, double* e_old, double* y0,
                                            double* y1, int32_t* preds_iter, double* energies, int Q, int K, int nn, int iters,
                                            double lmd) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
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
        *frozen = 0;
        *e_old = INFINITY;
    }
    __syncthreads();

    double* yold = y0;
    double* ynew = y1;
    int it = 0;
    for (; it < iters; it++) {
        // Y_new[q] = softmax_k(-unary[q] + lmd * sum_{j in nbr(q)} Y_old[j])                                (:150-154)
        for (int q = wave; q < Q; q += kLshotWaves) {
            const float* u = unary + (size_t)q * K;
            double mx = -INFINITY;
            int arg = 0x7fffffff;
            for (int k = lane; k < K; k += 64) {
                double m = 0.0;
                for (int r = 0; r < nn; r++) m += yold[(size_t)nbr[q * nn + r] * K + k];
                const double add = -(double)u[k] - (-lmd * m);
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
            if (lane == 0) preds_iter[(size_t)it * Q + q] = arg < K ? arg : 0;   // argmax of Y = argmax of its logits (0 for a NaN row)
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
                e += y * log(fmax(y, 1e-20)) + ((double)u[k] * y + (-lmd * m * y));
            }
            e = lshot_wave_sum(e);
            if (lane == 0) row_e[q] = e;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double e = 0.0;
            for (int q = 0; q < Q; q++) e += row_e[q];
            energies[it] = e;
            if (it > 1 && fabs(e - *e_old) <= 1e-6 * fabs(*e_old)) *frozen = 1;          // (:162)
            else *e_old = e;
        }
        __syncthreads();
        double* sw = yold;
        yold = ynew;
        ynew = sw;
        if (*frozen) break;
    }
    // frozen: the assignment and the energy of update `it` are repeated for the remaining entries               (:164-171)
    if (it < iters) {
        for (int j = it + 1; j < iters; j++) {
            for (int q = threadIdx.x; q < Q; q += blockDim.x) preds_iter[(size_t)j * Q + q] = preds_iter[(size_t)it * Q + q];
            if (threadIdx.x == 0) energies[j] = energies[it];
        }
    }
}

// One workgroup per task: kNN graph, then the bound updates.
__global__ __launch_bounds__(64 * kLshotWaves) void k_lshot_task(LshotArgs a) {
    extern __shared__ char lshot_smem[];
    const int Q = a.Q, K = a.K, D = a.D, nn = a.knn - 1, t = blockIdx.x;
    int* nbr = reinterpret_cast<int*>(lshot_smem);                     // [Q][nn]
    double* row_e = reinterpret_cast<double*>(lshot_smem + (((size_t)Q * nn * sizeof(int) + 7) & ~(size_t)7));   // [Q]
    __shared__ int frozen;
    __shared__ double e_old;
    double* y0 = a.ybuf + (size_t)t * 2 * Q * K;
    lshot_knn_rows(a.zq + (size_t)t * Q * D, a.d2 ? a.d2 + (size_t)t * Q * Q : nullptr, Q, D, nn, threadIdx.x >> 6, kLshotWaves,
                   threadIdx.x & 63, nbr, a.neighbours + (size_t)t * Q * nn);
    lshot_solve(a.unary + (size_t)t * Q * K, nbr, row_e, &frozen, &e_old, y0, y0 + (size_t)Q * K, a.preds_iter + (size_t)t * a.iters * Q,
                a.energies + (size_t)t * a.iters, Q, K, nn, a.iters, a.lmd);
}

// ---- the value sweep (tclip_laplacian_shot_sweep_tasks): the graph once per task, the updates once per (task, value) -------
// The neighbour lists of every task into global memory: grid (ceil(Q / kLshotWaves), T), one wavefront per query row.
__global__ __launch_bounds__(64 * kLshotWaves) void k_lshot_knn(const float* __restrict__ zq, const double* __restrict__ d2, int Q, int D,
                                                                int nn, int32_t* __restrict__ neighbours) {
    const int t = blockIdx.y, i = blockIdx.x * kLshotWaves + (threadIdx.x >> 6);
    if (i >= Q) return;
    lshot_knn_rows(zq + (size_t)t * Q * D, d2 ? d2 + (size_t)t * Q * Q : nullptr, Q, D, nn, i, Q, threadIdx.x & 63, nullptr,
                   neighbours + (size_t)t * Q * nn);
}

// Grid (task, value): block (t, p) solves task t of T with lmd[p].  It reads the task's unary term and neighbour lists (into
// LDS, as k_lshot_task keeps them) and owns slice p T + t of ybuf [P][T][2][Q][K], preds_iter [P][T][iters][Q] and
// energies [P][T][iters].
__global__ __launch_bounds__(64 * kLshotWaves) void k_lshot_sweep_updates(LshotArgs a, const double* __restrict__ lmd, int T) {
    extern __shared__ char lshot_smem[];
    const int Q = a.Q, K = a.K, nn = a.knn - 1, t = blockIdx.x, p = blockIdx.y;
    int* nbr = reinterpret_cast<int*>(lshot_smem);                     // [Q][nn]
    double* row_e = reinterpret_cast<double*>(lshot_smem + (((size_t)Q * nn * sizeof(int) + 7) & ~(size_t)7));   // [Q]
    __shared__ int frozen;
    __shared__ double e_old;
    const int32_t* lists = a.neighbours + (size_t)t * Q * nn;
    for (int i = threadIdx.x; i < Q * nn; i += blockDim.x) nbr[i] = lists[i];
    __syncthreads();
    const size_t vt = (size_t)p * T + t;                              // < P T
    double* y0 = a.ybuf + vt * 2 * Q * K;
    lshot_solve(a.unary + (size_t)t * Q * K, nbr, row_e, &frozen, &e_old, y0, y0 + (size_t)Q * K, a.preds_iter + vt * a.iters * Q,
                a.energies + vt * a.iters, Q, K, nn, a.iters, lmd[p]);
}

// The workspace as typed pointers; a null `base` gives `bytes` alone.
// rows of `dim` elements; pairdist: room for k_lshot_pairdist's [T][Q][Q] fp64 table (the visual entries); n_values > 0 (the
// sweep entry): ybuf for every (value, task) - the only region that grows with the values - and the values themselves; both
// take a whole number of 256-byte units PER VALUE, so that the total is affine in n_values
struct LshotWs {
    float *zs, *zq, *sup, *cnt, *proto;
    double *ybuf, *d2, *vals;
    size_t bytes;
};
static LshotWs lshot_ws(const tclip_problem& p, int dim, bool pairdist, int n_values, char* base) {
    const size_t T = (size_t)p.n_batches * p.tasks_per_batch, K = p.n_class, Q = p.n_query, S = p.n_support, D = dim;
    LshotWs w;
    WsCursor c{base};
    c.take(w.zs, T * S * D * 4);
    c.take(w.zq, T * Q * D * 4);
    c.take(w.sup, T * K * D * 4);
    c.take(w.cnt, T * K * 4);
    c.take(w.proto, T * K * D * 4);
    c.take(w.ybuf, (n_values > 0 ? (size_t)n_values : 1) * align_up(T * 2 * Q * K * 8));
    c.take(w.d2, T * Q * Q * 8, pairdist);
    c.take(w.vals, (size_t)n_values * align_up(8), n_values > 0);
    w.bytes = c.bytes;
    return w;
}

// what every entry checks of knn / norm_type on a checked problem
static int check_lshot(const tclip_problem& p, int32_t knn, int32_t norm_type) {
    if (norm_type != 0 && norm_type != 1) return fail(TCLIP_ERR_ARG, "norm_type must be 0 (UN) or 1 (L2N); CL2N needs a train mean the reference never passes");
    if (knn < 2 || knn > p.n_query) return fail(TCLIP_ERR_ARG, "knn must be in 2..n_query (the nearest neighbour of a query is the query itself)");
    if (p.n_query > kLshotMaxQ) return fail(TCLIP_ERR_ARG, "n_query must be <= 1024 for LAPLACIAN_SHOT");
    return TCLIP_OK;
}

// The launch sequence of both entries on rows of D elements: the support class sums of k_support_stats at D = K and of
// k_vis_support_stats otherwise; pairdist = false (probability features): the distances inside k_lshot_task, true (visual
// features): k_lshot_pairdist's table.
// values == nullptr: one solve per task with `lmd` (k_lshot_task; preds_iter [T][iters][Q], energies [T][iters]).  Otherwise the
// sweep: everything up to the distances runs once per task as it stands - none of it reads lmd -, k_lshot_knn writes the
// neighbour lists and k_lshot_sweep_updates solves every (task, value) (preds_iter [P][T][iters][Q], energies [P][T][iters]).
static int lshot_run(const tclip_problem& p, int D, bool pairdist, const RowSrc& x_q, const RowSrc& x_s, const int64_t* y_s,
                     int32_t knn, double lmd, int32_t norm_type, float* unary, int32_t* neighbours, int32_t* preds_iter,
                     double* energies, const LshotWs& ws, hipStream_t st, const double* values = nullptr, int n_values = 0) {
    const size_t smem = (((size_t)p.n_query * (knn - 1) * sizeof(int) + 7) & ~(size_t)7) + (size_t)p.n_query * sizeof(double);
    if (smem > 60000) return fail(TCLIP_ERR_ARG, "n_query * knn too large for the neighbour lists in LDS");
    const int Q = p.n_query, K = p.n_class, S = p.n_support, T = p.n_batches * p.tasks_per_batch, TK = T * K;
    float *const zs = ws.zs, *const zq = ws.zq, *const sup = ws.sup, *const cnt = ws.cnt, *const proto = ws.proto;
    double* const d2 = ws.d2;                                         // null without pairdist
    // normalization (:66-89), prototypes = class means of the normalised support (:201-205); the only launches that read the
    // task rows: a dense tensor, or table rows in place (x.idx != nullptr)
    auto normalize = [&](const RowSrc& x, int rows_per_task, float* out) {
        const int n_rows = T * rows_per_task;
        if (x.idx)
            hipLaunchKernelGGL(k_lshot_normalize<true>, dim3((n_rows + 3) / 4), dim3(256), 0, st, x, rows_per_task, n_rows, D, norm_type, out);
        else
            hipLaunchKernelGGL(k_lshot_normalize<false>, dim3((n_rows + 3) / 4), dim3(256), 0, st, x, rows_per_task, n_rows, D, norm_type, out);
    };
    normalize(x_s, S, zs);
    normalize(x_q, Q, zq);
    if (D != K)                                                       // as tim_loop: D = K keeps the probability entry's sums
        launch_vis_support_stats(st, zs, y_s, T, S, K, D, sup, cnt);
    else
        hipLaunchKernelGGL(k_support_stats, dim3(K, T), dim3(128), (size_t)S * sizeof(int), st, dense_rows(zs), y_s, S, K, 0, sup, cnt);
    hipLaunchKernelGGL(k_div_rows, dim3(ew_grid((size_t)TK * D)), dim3(256), 0, st, (const float*)sup, (const float*)cnt,
                       (size_t)TK * D, D, proto);
    hipLaunchKernelGGL(k_lshot_unary, dim3(Q, T), dim3(256), (size_t)D * sizeof(float), st, (const float*)proto, (const float*)zq, Q, K, D,
                       unary);
    if (pairdist)
        hipLaunchKernelGGL(k_lshot_pairdist, dim3((Q + kLshotPdTile - 1) / kLshotPdTile, T), dim3(256), 0, st, (const float*)zq, Q, D, d2);
    const LshotArgs a{zq, d2, unary, ws.ybuf, neighbours, preds_iter, energies, Q, K, D, knn, p.iters, lmd};
    if (!values) {
        hipLaunchKernelGGL(k_lshot_task, dim3(T), dim3(64 * kLshotWaves), smem, st, a);
    } else {
        double* lmds = ws.vals;
        launch_sweep_values(st, values, n_values, lmds, nullptr);
        hipLaunchKernelGGL(k_lshot_knn, dim3((Q + kLshotWaves - 1) / kLshotWaves, T), dim3(64 * kLshotWaves), 0, st, (const float*)zq,
                           (const double*)d2, Q, D, knn - 1, neighbours);
        hipLaunchKernelGGL(k_lshot_sweep_updates, dim3(T, n_values), dim3(64 * kLshotWaves), smem, st, a, (const double*)lmds, T);
    }
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

static const MethodRule kLshot{"LAPLACIAN_SHOT", true, kFewShotOnly, "%s needs iters >= 1", Limits::None};

// All five forms (ws_query: the workspace query to name): the checks in the one order of DESIGN.md ("The method host drivers"),
// then lshot_run.  The table forms read the task rows in place in the two normalisations; x_s and x_q are never built.  The
// pairwise-distance table goes with the visual rows.
static int lshot_entry(const tclip_problem* pp, const Rows& r, const int64_t* y_s, int32_t knn, double lmd, int32_t norm_type,
                       float* unary, int32_t* neighbours, int32_t* preds_iter, double* energies, void* workspace, size_t workspace_bytes,
                       void* stream, const char* ws_query) {
    if (int rc = check_method_problem(pp, r, kLshot)) return rc;
    const tclip_problem p = *pp;
    if (int rc = check_lshot(p, knn, norm_type)) return rc;
    if (int rc = check_pointers(r, kLshot, y_s && unary && neighbours && preds_iter && energies && workspace)) return rc;
    if (int rc = check_values(pp, r)) return rc;
    const int D = r.D(p);
    if (int rc = check_workspace(workspace, workspace_bytes, lshot_ws(p, D, r.visual, r.n_sweep(), nullptr).bytes, ws_query)) return rc;
    return lshot_run(p, D, r.visual, r.q(), r.s(), y_s, knn, lmd, norm_type, unary, neighbours, preds_iter, energies,
                     lshot_ws(p, D, r.visual, r.n_sweep(), (char*)workspace), (hipStream_t)stream, r.values, r.n_sweep());
}
static size_t lshot_bytes(const tclip_problem* p, const Rows& r) {
    return query_accepts(p, r, kLshot) ? lshot_ws(*p, r.D(*p), r.visual, r.n_sweep(), nullptr).bytes : 0;
}

}  // namespace tclip

extern "C" {

// No query looks at iters; the two dense ones do not look at n_support either.
size_t tclip_laplacian_shot_workspace_bytes(const tclip_problem* p) {
    return lshot_bytes(p, rows_dense(nullptr, nullptr, kAnyIters | kAnySupport));
}
size_t tclip_laplacian_shot_visual_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return lshot_bytes(p, rows_visual(dim, nullptr, nullptr, kAnyIters | kAnySupport));
}
size_t tclip_laplacian_shot_tasks_workspace_bytes(const tclip_problem* p) { return lshot_bytes(p, rows_tables(nullptr, kAnyIters)); }
size_t tclip_laplacian_shot_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return lshot_bytes(p, rows_visual_tables(dim, nullptr, kAnyIters));
}
size_t tclip_laplacian_shot_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values) {
    return lshot_bytes(p, rows_sweep(dim, nullptr, nullptr, n_values, kAnyIters));
}

int tclip_laplacian_shot_run(const tclip_problem* pp, const float* x_q, const float* x_s, const int64_t* y_s, int32_t knn,
                             double lmd, int32_t norm_type, float* unary, int32_t* neighbours, int32_t* preds_iter,
                             double* energies, void* workspace, size_t workspace_bytes, void* stream) {
    return lshot_entry(pp, rows_dense(x_q, x_s), y_s, knn, lmd, norm_type, unary, neighbours, preds_iter, energies, workspace,
                       workspace_bytes, stream, "tclip_laplacian_shot_workspace_bytes");
}

int tclip_laplacian_shot_visual_run(const tclip_problem* pp, int32_t dim, const float* x_q, const float* x_s, const int64_t* y_s,
                                    int32_t knn, double lmd, int32_t norm_type, float* unary, int32_t* neighbours,
                                    int32_t* preds_iter, double* energies, void* workspace, size_t workspace_bytes, void* stream) {
    return lshot_entry(pp, rows_visual(dim, x_q, x_s), y_s, knn, lmd, norm_type, unary, neighbours, preds_iter, energies, workspace,
                       workspace_bytes, stream, "tclip_laplacian_shot_visual_workspace_bytes");
}

int tclip_laplacian_shot_run_tasks(const tclip_problem* pp, const tclip_task_source* src, const int64_t* y_s, int32_t knn, double lmd,
                                   int32_t norm_type, float* unary, int32_t* neighbours, int32_t* preds_iter, double* energies,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return lshot_entry(pp, rows_tables(src), y_s, knn, lmd, norm_type, unary, neighbours, preds_iter, energies, workspace,
                       workspace_bytes, stream, "tclip_laplacian_shot_tasks_workspace_bytes");
}

int tclip_laplacian_shot_visual_run_tasks(const tclip_problem* pp, int32_t dim, const tclip_task_source* src, const int64_t* y_s,
                                          int32_t knn, double lmd, int32_t norm_type, float* unary, int32_t* neighbours,
                                          int32_t* preds_iter, double* energies, void* workspace, size_t workspace_bytes, void* stream) {
    return lshot_entry(pp, rows_visual_tables(dim, src), y_s, knn, lmd, norm_type, unary, neighbours, preds_iter, energies, workspace,
                       workspace_bytes, stream, "tclip_laplacian_shot_visual_tasks_workspace_bytes");
}

// LAPLACIAN_SHOT for a list of lmd values on the same tasks (see lshot_run)
int tclip_laplacian_shot_sweep_tasks(const tclip_problem* pp, int32_t dim, const tclip_task_source* src, const int64_t* y_s, int32_t knn,
                                     const double* values, int32_t n_values, int32_t norm_type, float* unary, int32_t* neighbours,
                                     int32_t* preds_iter, double* energies, void* workspace, size_t workspace_bytes, void* stream) {
    return lshot_entry(pp, rows_sweep(dim, src, values, n_values), y_s, knn, 0.0, norm_type, unary, neighbours, preds_iter, energies,
                       workspace, workspace_bytes, stream, "tclip_laplacian_shot_sweep_tasks_workspace_bytes");
}

}  // extern "C"
