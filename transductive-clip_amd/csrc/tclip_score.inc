// Scoring with a fitted EM-Dirichlet model (include/tclip.h: tclip_em_dirichlet_score, tclip_em_dirichlet_score_tasks): one
// E-step of a given alpha (T,K,K), v (T,K) on R rows per task that need not have been queries of the fit.  Included at the end of
// tclip_kernels.hip, uses its helpers (fail, TCLIP_HIP, check_workspace, dispatch_E, RowSrc) and the device functions the loop's
// E-step is made of (dirichlet_row_const, dirichlet_dot, softmax_row16, log_f32): the same operations in the same order, so a row
// scored here has the bits the loop gives it as a query.  DESIGN.md 8q has the budget and the reasons.
//
//   k_score_row_consts   rowc[t,k] = lgamma(sum_d alpha) - sum_d lgamma(alpha) for ALL T K model rows (no row list: nothing is
//                        known to be unchanged), one 32-lane group per row - the only workspace, T K floats
//   k_score              a block owns a tile of RT consecutive scored rows of one task:
//                          1. their log(z + eps) goes to LDS once (dense rows, or table rows through idx / cols as RowSrc reads),
//                             padded with zeros to E x 32 floats;
//                          2. the task's K alpha rows stream past them: each of the block's eight 32-lane groups holds RA rows of
//                             alpha - 1 in registers (element d in register d / 32 of lane d % 32, the layout of k_logits), takes
//                             the tile's rows from LDS one after the other and leaves rowc + dot in the tile's logits, in LDS;
//                          3. each of the sixteen 16-lane groups finishes rows of the tile: optional copy of the logits, softmax
//                             with the prior term (lambd v) / Q, argmax, optional one-hot, optional copy of u - all on the LDS row.
//                        No logits round trip through memory, no (T,R,K) scratch, and nothing a row's result could take from its
//                        neighbours: the tile only decides which block computes the row.
// A tile never crosses a task, and the grid is the number of tiles, T x ceil(R / RT) (strided beyond 65536 blocks): 1250 blocks
// for 125 tasks x 75 rows at K = 1000, 6250 for one task x 50 000 rows.

namespace tclip {

constexpr int score_tile_rows(int E) { return E <= 4 ? 32 : (E <= 16 ? 16 : 8); }      // RT: 2 x RT x 32 E floats of LDS <= 64 KB
constexpr int score_alpha_rows(int E) { return E <= 16 ? 4 : 2; }                       // RA: k_logits' choice, RA x E registers
constexpr int kScoreMaxGrid = 65536;

template <int E>
__global__ __launch_bounds__(256) void k_score_row_consts(const float* __restrict__ alpha, int n_rows, int K, float* __restrict__ rowc) {
    const int lane = threadIdx.x & (kGroup - 1);
    constexpr int kGroups = 256 / kGroup;
    for (long long row = (long long)blockIdx.x * kGroups + threadIdx.x / kGroup; row < n_rows; row += (long long)gridDim.x * kGroups) {
        const float c = dirichlet_row_const<E>(alpha + (size_t)row * K, K, lane);
        if (lane == 0) rowc[row] = c;
    }
}

template <int E>
__global__ __launch_bounds__(256) void k_score(RowSrc src, const float* __restrict__ alpha, const float* __restrict__ rowc,
                                               const float* __restrict__ v, int T, int R, int K, float lambd, float qf, int hard,
                                               float* __restrict__ u, int32_t* __restrict__ preds, float* __restrict__ logits) {
    constexpr int RT = score_tile_rows(E), RA = score_alpha_rows(E), KP = E * kGroup, kGroups = 256 / kGroup;
    constexpr int kFull = logits_full_regs(E);
    __shared__ float lz[RT * KP];        // log(z + eps) of the tile's rows, zeros past K
    __shared__ float lg[RT * KP];        // their logits, then their u
    const int lane = threadIdx.x & (kGroup - 1), group = threadIdx.x / kGroup;
    const int l16 = threadIdx.x & 15, g16 = threadIdx.x >> 4;
    const int tiles_per_task = (R + RT - 1) / RT;
    const long long n_tiles = (long long)T * tiles_per_task;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int t = (int)(tile / tiles_per_task), r0 = (int)(tile % tiles_per_task) * RT;
        const int nr = R - r0 < RT ? R - r0 : RT;
        const size_t row0 = (size_t)t * R + r0;
        const int32_t* c = src.cols ? src.cols + (size_t)t * K : nullptr;
        for (int r = group; r < nr; r += kGroups) {
            const float* xr = src.base + (src.idx ? (size_t)src.idx[row0 + r] : row0 + r) * K;
#pragma unroll
            for (int e = 0; e < E; e++) {
                const int d = e * kGroup + lane;
                lz[r * KP + d] = d < K ? log_f32(xr[c ? c[d] : d] + kEpsF) : 0.0f;
            }
        }
        __syncthreads();
        for (int k0 = group * RA; k0 < K; k0 += kGroups * RA) {
            float am1[RA][E], rc[RA];
#pragma unroll
            for (int a = 0; a < RA; a++) {
                const int k = k0 + a < K ? k0 + a : K - 1;          // past the last class: its row again, never written
                const float* ar = alpha + ((size_t)t * K + k) * K + lane;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    if (e < kFull) am1[a][e] = ar[e * kGroup] - 1.0f;
                    else am1[a][e] = e * kGroup + lane < K ? ar[e * kGroup] - 1.0f : 0.0f;
                }
                rc[a] = rowc[(size_t)t * K + k];
            }
            for (int r = 0; r < nr; r++) {
                float lv[E];
#pragma unroll
                for (int e = 0; e < E; e++) lv[e] = lz[r * KP + e * kGroup + lane];
#pragma unroll
                for (int a = 0; a < RA; a++) {
                    const float l3 = dirichlet_dot<E>(am1[a], lv, K, lane);
                    if (lane == 0 && k0 + a < K) lg[r * KP + k0 + a] = rc[a] + l3;
                }
            }
        }
        __syncthreads();
        for (int r = g16; r < nr; r += 16) {
            float* xr = lg + r * KP;
            const size_t out = (row0 + r) * K;
            if (logits)
                for (int k = l16; k < K; k += 16) logits[out + k] = xr[k];
            const int best_k = softmax_row16(xr, v ? v + (size_t)t * K : nullptr, K, lambd, qf, hard, 0, xr, l16);
            if (u)
                for (int k = l16; k < K; k += 16) u[out + k] = xr[k];
            if (l16 == 0) preds[row0 + r] = best_k;
        }
        __syncthreads();                 // the next tile of this block overwrites lz and lg
    }
}

template <int E> struct LaunchScoreRowConsts {
    static void run(hipStream_t st, const float* alpha, int n_rows, int K, float* rowc) {
        const int grid = (n_rows + 7) / 8 > kScoreMaxGrid ? kScoreMaxGrid : (n_rows + 7) / 8;
        hipLaunchKernelGGL(k_score_row_consts<E>, dim3(grid), dim3(256), 0, st, alpha, n_rows, K, rowc);
    }
};
template <int E> struct LaunchScore {
    static void run(hipStream_t st, RowSrc src, const float* alpha, const float* rowc, const float* v, int T, int R, int K,
                    float lambd, float qf, int hard, float* u, int32_t* preds, float* logits) {
        constexpr int RT = score_tile_rows(E);
        const long long tiles = (long long)T * ((R + RT - 1) / RT);
        hipLaunchKernelGGL(k_score<E>, dim3((unsigned)(tiles > kScoreMaxGrid ? kScoreMaxGrid : tiles)), dim3(256), 0, st, src, alpha,
                           rowc, v, T, R, K, lambd, qf, hard, u, preds, logits);
    }
};

static int check_score_problem(const tclip_score_problem* p) {
    if (!p) return fail(TCLIP_ERR_ARG, "tclip_score_problem is null");
    if (p->n_task < 1) return fail(TCLIP_ERR_ARG, "n_task must be >= 1");
    if (p->rows_per_task < 1) return fail(TCLIP_ERR_ARG, "rows_per_task must be >= 1");
    if (p->n_class < 2 || p->n_class > 1024) return fail(TCLIP_ERR_ARG, "n_class must be in 2..1024");
    if (p->n_query < 1) return fail(TCLIP_ERR_ARG, "n_query must be >= 1");
    if ((long long)p->n_task * p->n_class > 0x7fffffffLL) return fail(TCLIP_ERR_ARG, "n_task*n_class must fit in int32");
    if ((long long)p->n_task * p->rows_per_task > 0x7fffffffLL) return fail(TCLIP_ERR_ARG, "n_task*rows_per_task must fit in int32");
    return TCLIP_OK;
}

static int score(const tclip_score_problem* p, RowSrc src, const float* alpha, const float* v, float* u, int32_t* preds,
                 float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_workspace(workspace, workspace_bytes, tclip_em_dirichlet_score_workspace_bytes(p),
                                 "tclip_em_dirichlet_score_workspace_bytes"))
        return rc;
    const int T = p->n_task, R = p->rows_per_task, K = p->n_class;
    hipStream_t st = (hipStream_t)stream;
    float* rowc = (float*)workspace;
    dispatch_E<LaunchScoreRowConsts>(K, st, alpha, T * K, K, rowc);
    dispatch_E<LaunchScore>(K, st, src, alpha, (const float*)rowc, v, T, R, K, (float)p->lambd, (float)p->n_query, p->hard ? 1 : 0, u,
                            preds, logits);
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

}  // namespace tclip

extern "C" {

// O(T K) and independent of rows_per_task: the per-class row constants rowc (T,K) f32; the scored rows, their logarithms and
// their logits never leave the blocks' LDS, so there is no per-row scratch and no chunk.
size_t tclip_em_dirichlet_score_workspace_bytes(const tclip_score_problem* p) {
    if (check_score_problem(p) != TCLIP_OK) return 0;
    return align_up((size_t)p->n_task * p->n_class * 4);
}

int tclip_em_dirichlet_score(const tclip_score_problem* p, const float* x, const float* alpha, const float* v, float* u,
                             int32_t* preds, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_score_problem(p)) return rc;
    if (!x) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score: x is null");
    if (!alpha) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score: alpha is null");
    if (!preds) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score: preds is null");
    if (!workspace) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score: workspace is null");
    return score(p, dense_rows(x), alpha, v, u, preds, logits, workspace, workspace_bytes, stream);
}

int tclip_em_dirichlet_score_tasks(const tclip_score_problem* p, const float* table, const int64_t* idx, const int32_t* cols,
                                   const float* alpha, const float* v, float* u, int32_t* preds, float* logits, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (int rc = check_score_problem(p)) return rc;
    if (!table) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score_tasks: table is null");
    if (!idx) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score_tasks: idx is null");
    if (!alpha) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score_tasks: alpha is null");
    if (!preds) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score_tasks: preds is null");
    if (!workspace) return fail(TCLIP_ERR_ARG, "tclip_em_dirichlet_score_tasks: workspace is null");
    return score(p, RowSrc{table, idx, cols}, alpha, v, u, preds, logits, workspace, workspace_bytes, stream);
}

}  // extern "C"
