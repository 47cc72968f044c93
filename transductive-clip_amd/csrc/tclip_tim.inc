// ALPHA_TIM (SURVEY.md F4; reference: src/methods/few_shot/tim.py:192-322) and TIM_GD (tim.py:90-189), both on rows of any
// length (tclip_alpha_tim_run: probability features, D = K; tclip_alpha_tim_visual_run and tclip_tim_gd_run: any D in 1..1024):
// included at the end of tclip_kernels.hip, uses its helpers (fail, check_problem, align_up,
// k_support_stats, k_div_rows) and launch_vis_support_stats of tclip_visual_fs.inc.
//
// Per task the reference keeps one weight matrix W (K classes x D features) and runs `iter` Adam
// steps on  lw0 * CE(support) - (lw1 * H(marginal of the query predictions) - lw2 * H(query | prediction))
// with logits T (x.w_k - |w_k|^2/2 - |x|^2/2).  Autograd is replaced by the closed-form gradient:
//   dL/dlogit[i,k] = p_k (g_k - sum_j g_j p_j),  g = dL/dp  (softmax backward, row by row),
//   dL/dW[k,:]     = T (sum_i G[i,k] x_i - (sum_i G[i,k]) w_k).
// The reference's matmuls go through MKL and its backward through autograd's own operation order, so there is
// no bit-level target here (unlike EM-Dirichlet): parity is pinned to fixtures within a float tolerance.
// tclip_alpha_tim[_visual]_run_tasks and tclip_tim_gd_run_tasks are the same loops fed from the feature tables: every kernel that
// touches a task row goes through TimRows<kIdx>::row, and kIdx = true reads the table rows in place in every step.
// Per iteration: k_tim_gemm_mfma<false> (logits; 64x64 tiles on the matrix cores), k_tim_softmax, k_tim_marginal, k_tim_grad,
// k_tim_gemm_mfma<true> (dW, also the column sums of G), k_tim_adam (one wavefront per weight row), k_tim_criterion.
// tclip_alpha_tim_sweep_tasks runs the same loop over n_values x tasks solves for a list of alpha values (tim_loop_on with
// `values`); the helpers all four sweep entries share (check_sweep_*, k_sweep_values) are here too, this file being included first.
// So is what the host drivers of every method of tclip_tim.inc, tclip_lshot.inc and tclip_methods.inc share: the description of
// the rows an entry was given (Rows and its five adaptors), a method's MethodRule, and the shared checks in their one order
// (check_method_problem, check_pointers, check_values; DESIGN.md, "The method host drivers").  Here tim_ws lays the workspace
// out, alpha_tim_run and tim_gd_run are the one function behind each method's entries, tim_run picks the dense or the table rows.

namespace tclip {

// The support rows of a task followed by its query rows, D elements each.  kIdx = false: dense x_s [T,S,D] and x_q [T,Q,D].
// kIdx = true: the rows of two feature tables read in place (tclip_*_run_tasks): row i of task t is
// xs[s_idx[t S + i]] for i < S and xq[q_idx[t Q + (i - S)]] otherwise, its element d table column cols[t D + d] (cols == nullptr:
// d).  The dense form carries no member of the indexed one: its kernels take the arguments they always took.
template <bool kIdx>
struct TimRows;
template <>
struct TimRows<false> {
    const float* xs;
    const float* xq;
    int S, Q, D;
    __device__ int real(int t) const { return t; }
    __device__ const float* row(int t, int i) const {
        return i < S ? xs + ((size_t)t * S + i) * D : xq + ((size_t)t * Q + (i - S)) * D;
    }
};
template <>
struct TimRows<true> {
    const float* xs;         // table_s [rows_s, D]
    const float* xq;         // table_q [rows_q, D]
    const int64_t* s_idx;    // [T, S]
    const int64_t* q_idx;    // [T, Q]
    const int32_t* cols;     // [T, D] or nullptr
    int S, Q, D;
    int n_real;              // 0: every task has index rows of its own.  T > 0 (a value sweep): task t reads the rows of task t % T
    // the task whose rows task t reads: a kernel takes it once and passes IT to row() and task_cols()
    __device__ int real(int t) const { return n_real ? t % n_real : t; }
    __device__ const float* row(int t, int i) const {
        return i < S ? xs + (size_t)s_idx[(size_t)t * S + i] * D : xq + (size_t)q_idx[(size_t)t * Q + (i - S)] * D;
    }
    __device__ const int32_t* task_cols(int t) const { return cols ? cols + (size_t)t * D : nullptr; }
};

// one constant per message that more than one entry gives
static const char* const kNullArg = "null pointer argument";
static const char* const kZeroShotOnly = "%s is a zero-shot method: n_support must be 0";
static const char* const kFewShotOnly = "%s is a few-shot method: n_support must be positive";
static const char* const kDimRange = "dim must be in 1..1024";
static const char* const kItersForLogits = "%s needs iters >= 1 (the accuracy is read from the last iteration's logits)";

// ---- value sweeps (tclip_*_sweep_tasks): what the four entries share ---------------------------------------------------------
// dim of a sweep entry: 0 = probability features (rows of n_class elements), 1..1024 = visual features
static int check_sweep_dim(int32_t dim) {
    if (dim < 0 || dim > 1024) return fail(TCLIP_ERR_ARG, "dim must be 0 (probability features) or in 1..1024 (visual features)");
    return TCLIP_OK;
}

// A sweep solves the same T tasks for P values: P T solves, value-major.  Grids carry a solve in blockIdx.y / .z, hence the cap.
static int check_sweep_count(const tclip_problem* p, int32_t n_values) {
    if (n_values < 1) return fail(TCLIP_ERR_ARG, "n_values must be >= 1");
    const size_t VT = (size_t)n_values * p->n_batches * p->tasks_per_batch;
    if (VT > 65535) return fail(TCLIP_ERR_ARG, "n_values*n_batches*tasks_per_batch must be <= 65535 per call");
    if (VT * p->n_class > 0x7fffffffu || VT * ((size_t)p->n_support + p->n_query) > 0x7fffffffu)
        return fail(TCLIP_ERR_ARG, "n_values*tasks*n_class and n_values*tasks*(n_support + n_query) must fit in int32");
    return TCLIP_OK;
}

static int check_sweep_values(const tclip_problem* p, const double* values, int32_t n_values) {
    if (!values) return fail(TCLIP_ERR_ARG, kNullArg);
    if (int rc = check_sweep_count(p, n_values)) return rc;
    for (int i = 0; i < n_values; i++)
        if (!(values[i] - values[i] == 0.0)) return fail(TCLIP_ERR_ARG, "every value of a sweep must be finite");
    return TCLIP_OK;
}

// ---- what rows an entry was given, and the checks every method's entries share (DESIGN.md, "The method host drivers") ---------
// The five call forms of a method differ in three things: the row length, whether the rows are dense tensors or table rows
// behind a tclip_task_source, and whether a value list replaces the scalar.  One adaptor per form builds the description; a
// workspace query uses its entry's adaptor with null pointers.
enum : unsigned {                  // checks an entry leaves out that its siblings make (kept as they were; DESIGN.md lists them)
    kAnySupport = 1,               // does not look at n_support
    kAnyIters = 2,                 // does not look at iters
};
struct Rows {
    int32_t dim;                   // the entry's dim argument; 0 where it has none
    bool visual;                   // rows of dim elements; otherwise of n_class
    bool tables, sweep;
    const float *x_q, *x_s;        // dense forms (x_s: few-shot methods)
    const tclip_task_source* src;  // table forms
    const double* values;          // sweeps
    int32_t n_values;
    unsigned skip;
    int D(const tclip_problem& p) const { return visual ? dim : p.n_class; }
    int n_sweep() const { return sweep ? n_values : 0; }
    RowSrc q() const { return tables ? RowSrc{src->table_q, src->q_idx, src->cols} : dense_rows(x_q); }
    RowSrc s() const { return tables ? RowSrc{src->table_s, src->s_idx, src->cols} : dense_rows(x_s); }
};
static Rows rows_dense(const float* x_q, const float* x_s, unsigned skip = 0) {
    return Rows{0, false, false, false, x_q, x_s, nullptr, nullptr, 0, skip};
}
static Rows rows_visual(int32_t dim, const float* x_q, const float* x_s, unsigned skip = 0) {
    return Rows{dim, true, false, false, x_q, x_s, nullptr, nullptr, 0, skip};
}
static Rows rows_tables(const tclip_task_source* src, unsigned skip = 0) {
    return Rows{0, false, true, false, nullptr, nullptr, src, nullptr, 0, skip};
}
static Rows rows_visual_tables(int32_t dim, const tclip_task_source* src, unsigned skip = 0) {
    return Rows{dim, true, true, false, nullptr, nullptr, src, nullptr, 0, skip};
}
// the sweeps' rule, once: dim == 0 is the problem of the _run_tasks entry, dim > 0 that of the _visual_run_tasks entry
static Rows rows_sweep(int32_t dim, const tclip_task_source* src, const double* values, int32_t n_values, unsigned skip = 0) {
    return Rows{dim, dim > 0, true, true, nullptr, nullptr, src, values, n_values, skip};
}

// a tclip_task_source whose members other than cols are all there
static bool task_source_complete(const tclip_task_source* src) {
    return src && src->table_q && src->q_idx && src->table_s && src->s_idx;
}

// What a method asks of the problem, whichever form it is called in
enum class Limits { None, Rows, Rows16 };      // int32 limits of the kernels on rows of dim elements
struct MethodRule {
    const char* who;
    bool few_shot;
    const char* support_text;      // kFewShotOnly / kZeroShotOnly, or the method's own wording
    const char* iters_text;        // null: iters may be 0
    Limits limits;
};

// The checks a run entry and its workspace query share, in the one order of every method: the problem, dim, iters, n_support,
// the int32 limits; a sweep query adds check_sweep_count.
static int check_method_problem(const tclip_problem* p, const Rows& r, const MethodRule& m) {
    if (int rc = check_problem(p)) return rc;
    if (r.sweep) {
        if (int rc = check_sweep_dim(r.dim)) return rc;
    } else if (r.visual && (r.dim < 1 || r.dim > 1024)) {
        return fail(TCLIP_ERR_ARG, kDimRange);
    }
    if (m.iters_text && !(r.skip & kAnyIters) && p->iters < 1) return fail(TCLIP_ERR_ARG, m.iters_text, m.who);
    if (!(r.skip & kAnySupport) && (p->n_support > 0) != m.few_shot) return fail(TCLIP_ERR_ARG, m.support_text, m.who);
    const size_t T = (size_t)p->n_batches * p->tasks_per_batch, R = (size_t)p->n_support + p->n_query;
    if (r.visual && m.limits == Limits::Rows && T * R > 0x7fffffffu)
        return fail(TCLIP_ERR_ARG, "%s: tasks * (n_support + n_query) must fit in int32", m.who);
    if (r.visual && m.limits == Limits::Rows16 && (T * R * 16 > 0x7fffffffu || T * (size_t)r.dim > 0x7fffffffu))
        return fail(TCLIP_ERR_ARG, "%s: tasks * (n_support + n_query) * 16 and tasks * dim must fit in int32", m.who);
    return TCLIP_OK;
}
// a workspace query's checks: true when `p` may be laid out
static bool query_accepts(const tclip_problem* p, const Rows& r, const MethodRule& m) {
    return check_method_problem(p, r, m) == TCLIP_OK && (!r.sweep || check_sweep_count(p, r.n_values) == TCLIP_OK);
}

// The rows' own pointers and every other pointer of the entry (`others`), then "cols must be NULL on visual features"
static int check_pointers(const Rows& r, const MethodRule& m, bool others, bool cols_allowed = false) {
    const bool rows = r.tables ? task_source_complete(r.src) : r.x_q && (r.x_s || !m.few_shot);
    if (!rows || !others) return fail(TCLIP_ERR_ARG, kNullArg);
    if (r.tables && r.visual && r.src->cols && !cols_allowed)
        return fail(TCLIP_ERR_ARG, "%s on visual features permutes no columns: cols must be NULL", m.who);
    return TCLIP_OK;
}
// a sweep's value list (the workspace check follows)
static int check_values(const tclip_problem* p, const Rows& r) {
    return r.sweep ? check_sweep_values(p, r.values, r.n_values) : TCLIP_OK;
}

// The values on the device for the kernels that read one per solve: kSweepChunk of them per launch as a kernel argument.  (A
// copy from the caller's pageable host array would make the call wait for the stream.)
constexpr int kSweepChunk = 16;
struct SweepChunk { double v[kSweepChunk]; };
__global__ void k_sweep_values(SweepChunk c, int n, double* __restrict__ out_d, float* __restrict__ out_f) {
    const int i = threadIdx.x;
    if (i >= n) return;
    double v = c.v[0];
#pragma unroll
    for (int j = 1; j < kSweepChunk; j++) v = i == j ? c.v[j] : v;
    if (out_d) out_d[i] = v;
    if (out_f) out_f[i] = (float)v;
}

// out_d [n_values] f64 and / or out_f [n_values] f32 (the conversion the single-value entries apply to their scalar)
static void launch_sweep_values(hipStream_t st, const double* values, int n_values, double* out_d, float* out_f) {
    for (int i0 = 0; i0 < n_values; i0 += kSweepChunk) {
        SweepChunk c = {};
        const int n = n_values - i0 < kSweepChunk ? n_values - i0 : kSweepChunk;
        for (int j = 0; j < n; j++) c.v[j] = values[i0 + j];
        hipLaunchKernelGGL(k_sweep_values, dim3(1), dim3(64), 0, st, c, n, out_d ? out_d + i0 : nullptr, out_f ? out_f + i0 : nullptr);
    }
}

constexpr int kTimMarginalGd = 2;   // TimLoss::ent1 of TIM_GD: Shannon with the 1e-12 of tim.py:171-172 inside the logarithm
struct TimLoss {
    float lw0, lw1, lw2, alpha;
    int ent0, ent1, ent2;   // 0 = Shannon, 1 = Alpha; ent1 also kTimMarginalGd
};

static void launch_vis_support_stats(hipStream_t st, const float* xs, const int64_t* ys, int T, int S, int K, int D, float* sup,
                                     float* cnt);   // tclip_visual_fs.inc
static void launch_vis_support_stats(hipStream_t st, const RowSrc& xs, const int64_t* ys, int T, int S, int K, int D, float* sup,
                                     float* cnt);   // tclip_visual_fs.inc: dense rows, or a feature table read in place

constexpr int kTimTile = 64;

__device__ __forceinline__ float tim_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// |x_i|^2 of every support / query row, once per run.  kIdx: the rows of the tables in place; a lane owns the same elements
// d = lane, lane + 64, ... of the (column-permuted) row, so the sum is the dense one.
template <bool kIdx>
__global__ void k_tim_row_sqnorm(TimRows<kIdx> X, int n_rows_total, float* __restrict__ xn) {
    const int R = X.S + X.Q;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows_total) return;
    const int tx = X.real(row / R);
    const float* x = X.row(tx, row % R);
    float s = 0.0f;
    if constexpr (kIdx) {
        const int32_t* c = X.task_cols(tx);
        for (int d = lane; d < X.D; d += 64) {
            const float v = x[c ? c[d] : d];
            s = fmaf(v, v, s);
        }
    } else {
        for (int d = lane; d < X.D; d += 64) s = fmaf(x[d], x[d], s);
    }
    s = tim_wave_sum(s);
    if (lane == 0) xn[row] = s;
}

__global__ void k_tim_w_sqnorm(const float* __restrict__ W, int n_rows, int D, float* __restrict__ wn) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const float* w = W + (size_t)row * D;
    float s = 0.0f;
    for (int d = lane; d < D; d += 64) s = fmaf(w[d], w[d], s);
    s = tim_wave_sum(s);
    if (lane == 0) wn[row] = s;
}

// L[t][i][k] = T ((x_i . w_k - |w_k|^2 / 2) - |x_i|^2 / 2)   (tim.py:212-216)   and   dW[t][k][d] = sum_i G[i][k] x_i[d]:
// The two GEMMs of a step on the matrix cores.  v_mfma_f32_32x32x2_f32 takes ONE fp32 of A and ONE of B per lane (lane l:
// A[row l & 31][k = l >> 5], B[k = l >> 5][column l & 31]) and is exact fp32 multiply-add, accumulated over k in order within a
// block of kTimSumSlices slices.  Its peak is the vector FMA peak (157 TFLOP/s),
// so the gain is what the freed vector pipe is worth to the staging code: measured against round 2's 4 x 4-per-thread FMA tiles
// (64 x 64, 1000 Adam steps): K = 10 +6 %, K = 100 +9 %, K = 397 36.5 against 35.1 TFLOP/s, K = 1000 (S = 4000, 4 tasks) 59.0 against 49.2
// (52.7 before interior tiles took their slices with 128-bit loads).
// Depth-16 slices of both operands through LDS (k-major, the tile dimension contiguous: conflict-free 32-float reads for
// the operand fragments), the next slice's global loads in flight behind the MFMAs; the block's four wavefronts sit 2 x 2.
//   kTN = false (logits):  C[m][n] = sum_k X_m[k] W_n[k]          rows of X and W contiguous along k (stored transposed)
//   kTN = true  (dW):      C[m][n] = sum_i G[i][m] X_i[n]         both operands contiguous along the tile dimension
// K classes and rows of X.D elements (R = S + Q rows per task): the logits are R x K over a depth of D, dW is K x D over a
// depth of R; W and dW rows have D elements, G and the logits' rows K.
// Epilogue: the logits' scaling and norms, or (dW) the column sums of G by the blocks of the first column tile.
// TILE = 128 (2 x 2 MFMA tiles per wavefront) loses to partial tiles and to fewer blocks: K = 397 25.4, K = 1000 48.9 TFLOP/s.
// The contraction is summed in two levels: the MFMAs accumulate kTimSumSlices slices (64 products) from zero, then that block sum
// is added to the running total.  One accumulator over a depth of 1000 rounds every addition at the size of the whole sum: on
// probability features at K ~ 1000 (all products of one sign in the logits, R = S + Q > 1000 rows in dW) the gradient was 6 to
// 12 times, the logits up to 25 times as far from float64 as the reference's fp32 run (tests/test_gpu_tim_gradient.py); with
// block sums of 64 both are as close as the reference (DESIGN.md 8d).  The column sums of G are taken the same way.
// The throughput figures in this comment were measured with the single accumulator; the two-level sum costs 1.4 to 3.5 % of a
// run of 1000 Adam steps (K = 397, D = 1024, 20 tasks: 59.5 against 61.3 TFLOP/s; K = 1000, D = 1024, 4 tasks: 51.5 against 52.2).
constexpr int kTimSumSlices = 4;
constexpr int kTimMfmaDepth = 16;    // measured at 64 x 64 tiles: depth 16 52.7, 32 45.9, 64 25.2 TFLOP/s (K = 1000, S = 4000, 4 tasks)
typedef float tim_f16x __attribute__((ext_vector_type(16)));

// TILE = 64, the one instantiation launched: one 32 x 32 MFMA tile per wavefront (more, smaller blocks: few tasks, class counts just
// above a multiple of 64), 16 + 16 accumulator registers per lane for the two levels of the sum.  TILE = 128 (2 x 2 MFMA tiles per
// wavefront, 4 MFMAs per 4 LDS reads) would hold 64 + 64.
// kIdx: the rows of X are table rows read in place (TimRows<true>).  A thread stages the same (row, depth) / (depth, column)
// positions of a slice into the same LDS words, so the MFMAs accumulate the dense kernel's values in its order.  With cols the
// elements are fetched one by one inside the table row just addressed (at most 4 KB); without, interior tiles keep the 128-bit
// loads when the tables' base pointers are 16-byte aligned too (a table may be a view at an odd offset).
template <bool kTN, int TILE, bool kIdx>
__global__ __launch_bounds__(256) void k_tim_gemm_mfma(TimRows<kIdx> X, int K, const float* __restrict__ Bmat /* W (logits) or G (dW) */,
                                                       const float* __restrict__ wn, const float* __restrict__ xn, float temp,
                                                       float* __restrict__ C, float* __restrict__ cs) {
    constexpr int kPad = 1;                                          // odd row stride: the transposed stores of two depth groups hit different banks
    constexpr int MI = TILE / 64;                                    // MFMA tiles per wavefront and dimension
    constexpr int PER = TILE * kTimMfmaDepth / 256;                      // floats of each operand slice a thread stages (4 or 8)
    __shared__ float As[kTimMfmaDepth][TILE + kPad];
    __shared__ float Bs[kTimMfmaDepth][TILE + kPad];
    const int F = X.D, R = X.S + X.Q, t = blockIdx.z;               // F: elements of a feature row
    const int tx = X.real(t);                                        // the task whose rows this one reads: t itself outside a value sweep
    const int M = kTN ? K : R, N = kTN ? F : K, D = kTN ? R : F;     // C is M x N, the contraction runs over D
    const int m0 = blockIdx.y * TILE, n0 = blockIdx.x * TILE;
    const int id = threadIdx.x, wave = id >> 6, lane = id & 63, wm = wave >> 1, wnn = wave & 1, half = lane >> 5, li = lane & 31;
    tim_f16x acc[MI][MI], total[MI][MI];                             // the current block of kTimSumSlices slices; the blocks before it
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < MI; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = total[i][j][r] = 0.0f;
    const bool sums = kTN && blockIdx.x == 0 && id < TILE;
    float colsum = 0.0f, colsum_total = 0.0f;
    // this thread's part of a depth-16 slice of both operands, global memory -> registers.  The NEXT slice is requested
    // before the current one's MFMAs are issued, so its latency hides behind them.
    float a[PER], b[PER];
    // kTN: depth = id / (TILE / PER), PER consecutive tile positions; else: tile row = id / (16 / PER), PER consecutive depths
    constexpr int kThreadsPerDepth = TILE / PER, kThreadsPerRow = kTimMfmaDepth / PER;
    // interior tiles of a problem whose rows are 16-byte aligned (row lengths a multiple of 4: every base pointer is a 256-byte
    // aligned workspace offset or a torch allocation) take their PER floats as 128-bit loads: a quarter of the load instructions.
    // The logits read rows of F elements only, dW rows of G (K elements) and of X (F elements)
    bool rows_vec = true;                                            // block-uniform, like the rest of the predicate
    const int32_t* c = nullptr;                                      // this task's column permutation, if any
    const float* arow_in_place = nullptr;                            // !kTN: a thread stages the same row of X in every slice
    if constexpr (kIdx) {
        c = X.task_cols(tx);
        rows_vec = !c && ((reinterpret_cast<uintptr_t>(X.xs) | reinterpret_cast<uintptr_t>(X.xq)) & 15) == 0;
        if (!kTN && m0 + id / kThreadsPerRow < M) arow_in_place = X.row(tx, m0 + id / kThreadsPerRow);
    }
    auto col = [&](int d) {
        if constexpr (kIdx) return c ? c[d] : d;
        else return d;
    };
    const bool vec = (F & 3) == 0 && (!kTN || (K & 3) == 0) && m0 + TILE <= M && n0 + TILE <= N && rows_vec;      // block-uniform
    auto fetch = [&](int d0) {
        if (kTN) {
            const int pp = (id % kThreadsPerDepth) * PER, i = d0 + id / kThreadsPerDepth;
            const float* grow = i < R ? Bmat + ((size_t)t * R + i) * K : nullptr;      // G row i
            const float* xrow = i < R ? X.row(tx, i) : nullptr;
            if (vec && grow) {
#pragma unroll
                for (int j = 0; j < PER; j += 4) {
                    const float4 av = *reinterpret_cast<const float4*>(grow + m0 + pp + j);
                    const float4 bv = *reinterpret_cast<const float4*>(xrow + n0 + pp + j);
                    a[j] = av.x; a[j + 1] = av.y; a[j + 2] = av.z; a[j + 3] = av.w;
                    b[j] = bv.x; b[j + 1] = bv.y; b[j + 2] = bv.z; b[j + 3] = bv.w;
                }
                return;
            }
#pragma unroll
            for (int j = 0; j < PER; j++) {
                a[j] = (grow && m0 + pp + j < M) ? grow[m0 + pp + j] : 0.0f;
                b[j] = (xrow && n0 + pp + j < N) ? xrow[col(n0 + pp + j)] : 0.0f;
            }
        } else {
            const int row = id / kThreadsPerRow, kp = (id % kThreadsPerRow) * PER;
            const float* arow = kIdx ? arow_in_place : m0 + row < M ? X.row(tx, m0 + row) : nullptr;
            const float* brow = n0 + row < N ? Bmat + ((size_t)t * K + n0 + row) * F : nullptr;   // W row
            if (vec && d0 + kTimMfmaDepth <= D) {
#pragma unroll
                for (int j = 0; j < PER; j += 4) {
                    const float4 av = *reinterpret_cast<const float4*>(arow + d0 + kp + j);
                    const float4 bv = *reinterpret_cast<const float4*>(brow + d0 + kp + j);
                    a[j] = av.x; a[j + 1] = av.y; a[j + 2] = av.z; a[j + 3] = av.w;
                    b[j] = bv.x; b[j + 1] = bv.y; b[j + 2] = bv.z; b[j + 3] = bv.w;
                }
                return;
            }
#pragma unroll
            for (int j = 0; j < PER; j++) {
                const int d = d0 + kp + j;
                a[j] = (arow && d < D) ? arow[col(d)] : 0.0f;
                b[j] = (brow && d < D) ? brow[d] : 0.0f;
            }
        }
    };
    fetch(0);
    for (int d0 = 0; d0 < D; d0 += kTimMfmaDepth) {
        __syncthreads();                                             // the previous slice's fragments have been read
        if (kTN) {
            const int kd = id / kThreadsPerDepth, pp = (id % kThreadsPerDepth) * PER;
#pragma unroll
            for (int j = 0; j < PER; j++) {
                As[kd][pp + j] = a[j];
                Bs[kd][pp + j] = b[j];
            }
        } else {
            const int row = id / kThreadsPerRow, kp = (id % kThreadsPerRow) * PER;
#pragma unroll
            for (int j = 0; j < PER; j++) {
                As[kp + j][row] = a[j];
                Bs[kp + j][row] = b[j];
            }
        }
        __syncthreads();
        if (d0 + kTimMfmaDepth < D) fetch(d0 + kTimMfmaDepth);
        if (sums) {
#pragma unroll
            for (int kk = 0; kk < kTimMfmaDepth; kk++) colsum += As[kk][id];
        }
#pragma unroll
        for (int kk = 0; kk < kTimMfmaDepth; kk += 2) {
            float af[MI], bf[MI];
#pragma unroll
            for (int i = 0; i < MI; i++) {
                af[i] = As[kk + half][wm * (TILE / 2) + i * 32 + li];
                bf[i] = Bs[kk + half][wnn * (TILE / 2) + i * 32 + li];
            }
#pragma unroll
            for (int i = 0; i < MI; i++)
#pragma unroll
                for (int j = 0; j < MI; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if ((d0 / kTimMfmaDepth + 1) % kTimSumSlices == 0 || d0 + kTimMfmaDepth >= D) {      // block-uniform: a block sum is complete
#pragma unroll
            for (int i = 0; i < MI; i++)
#pragma unroll
                for (int j = 0; j < MI; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        total[i][j][r] += acc[i][j][r];
                        acc[i][j][r] = 0.0f;
                    }
            colsum_total += colsum;
            colsum = 0.0f;
        }
    }
    // C/D map of the 32 x 32 tile: register r of lane l holds row 8 (r >> 2) + 4 (l >> 5) + (r & 3), column l & 31
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < MI; j++) {
            const int n = n0 + wnn * (TILE / 2) + j * 32 + li;
            if (n >= N) continue;
            const float wnv = kTN ? 0.0f : wn[(size_t)t * K + n];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + wm * (TILE / 2) + i * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
                if (m >= M) continue;
                const float v = total[i][j][r];
                if (kTN) C[((size_t)t * K + m) * F + n] = v;
                else C[((size_t)t * R + m) * K + n] = temp * ((v - 0.5f * wnv) - 0.5f * xn[(size_t)t * R + m]);
            }
        }
    if (sums && m0 + id < M) cs[(size_t)t * K + m0 + id] = colsum_total;
}

// Row softmax in place (one wavefront per row); on request the raw query logits and their first-maximum index
// are kept - that is what compute_acc sees after the last iteration (tim.py:321).
__global__ void k_tim_softmax(float* __restrict__ P, int n_rows_total, int S, int Q, int K, float* __restrict__ logits_q,
                              int32_t* __restrict__ preds) {
    const int R = S + Q;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows_total) return;
    float* p = P + (size_t)row * K;
    float v[16];
    float mx = -INFINITY;
    int arg = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int k = e * 64 + lane;
        v[e] = k < K ? p[k] : -INFINITY;
        if (v[e] > mx) { mx = v[e]; arg = k; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o);
        const int oa = __shfl_xor(arg, o);
        if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
    }
    const int t = row / R, i = row % R;
    if (i >= S && logits_q) {
        float* out = logits_q + ((size_t)t * Q + (i - S)) * K;
#pragma unroll
        for (int e = 0; e < 16; e++)
            if (e * 64 + lane < K) out[e * 64 + lane] = v[e];
        if (lane == 0) preds[(size_t)t * Q + (i - S)] = arg < K ? arg : 0;        // 0 for a NaN row
    }
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        v[e] = e * 64 + lane < K ? expf(v[e] - mx) : 0.0f;
        s += v[e];
    }
    s = tim_wave_sum(s);
#pragma unroll
    for (int e = 0; e < 16; e++)
        if (e * 64 + lane < K) p[e * 64 + lane] = v[e] / s;
}

// marginal[t][k] = mean over the query rows of p[q][k]                                              (q_probs.mean(1))
// Summed in double: the Alpha marginal term is m^(alpha-1), six times m's relative error at alpha = 7, and a sequential fp32 sum
// over 128 rows put the gradient 3 to 8 times as far from float64 as the reference's fp32 run, whose mean is a cascade sum
// (tests/test_gpu_tim_gradient.py).  The mean is rounded to fp32 once.
__global__ void k_tim_marginal(const float* __restrict__ P, int S, int Q, int K, float* __restrict__ marg) {
    const int t = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const float* p = P + ((size_t)t * (S + Q) + S) * K + k;
    double s = 0.0;
    for (int q = 0; q < Q; q++) s += (double)p[(size_t)q * K];
    marg[(size_t)t * K + k] = (float)(s / (double)Q);
}

// P -> G = dLoss/dlogits, row by row (tim.py:276-305 differentiated by hand; 1e-12 where the reference adds it).
// alphas == nullptr: every task takes c.alpha and its own labels.  Otherwise (a value sweep over n_real tasks): task t takes
// alphas[t / n_real] and the labels of task t % n_real.
__global__ void k_tim_grad(float* __restrict__ P, const int64_t* __restrict__ ys, const float* __restrict__ marg,
                           int n_rows_total, int S, int Q, int K, TimLoss c, const float* __restrict__ alphas, int n_real) {
    const int R = S + Q;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows_total) return;
    const int t = row / R, i = row % R;
    const float alpha = alphas ? alphas[t / n_real] : c.alpha;
    float* p = P + (size_t)row * K;
    if (i < S) {                                                      // cross-entropy of a support row: only g_y is non-zero
        const int y = (int)ys[(size_t)(alphas ? t % n_real : t) * S + i];
        const float py = (y >= 0 && y < K) ? p[y] : 1.0f;
        const float gy = c.ent0 == 0 ? -c.lw0 / ((py + 1e-12f) * (float)S)
                                     : c.lw0 * powf(py + 1e-12f, -alpha) / (float)S;
        const float dot = gy * py;
        for (int k = lane; k < K; k += 64) p[k] = p[k] * ((k == y ? gy : 0.0f) - dot);
        return;
    }
    const float* m = marg + (size_t)t * K;
    const float invQ = 1.0f / (float)Q, a = alpha, am1 = alpha - 1.0f;
    float g[16], pv[16];
    float dot = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int k = e * 64 + lane;
        g[e] = 0.0f;
        pv[e] = 0.0f;
        if (k < K) {
            const float pk = p[k], mk = m[k];
            // -lw1 * d q_ent / d p   (through the mean over the Q rows)
            const float gm = c.ent1 == 0 ? (logf(mk) + 1.0f)
                           : c.ent1 == kTimMarginalGd ? (logf(mk + 1e-12f) + mk / (mk + 1e-12f)) : a * powf(mk, am1) / am1;
            // +lw2 * d q_cond_ent / d p
            const float pe = pk + 1e-12f;
            const float gc = c.ent2 == 0 ? -(logf(pe) + pk / pe) : -a * powf(pe, am1) / am1;
            g[e] = (c.lw1 * gm + c.lw2 * gc) * invQ;
            pv[e] = pk;
            dot = fmaf(g[e], pk, dot);
        }
    }
    dot = tim_wave_sum(dot);
#pragma unroll
    for (int e = 0; e < 16; e++)
        if (e * 64 + lane < K) p[e * 64 + lane] = pv[e] * (g[e] - dot);
}

// torch.optim.Adam, single-tensor CPU path (betas 0.9 / 0.999, eps 1e-8, no weight decay): one wavefront per weight
// row; also |w_k|^2 for the next logits and ||w_old_k - w_k|| for the logged criterion (tim.py:313-314).
__global__ void k_tim_adam(float* __restrict__ W, float* __restrict__ M, float* __restrict__ V, const float* __restrict__ dW,
                           const float* __restrict__ cs, int n_rows, int D, float temp, float neg_step, float bc2_sqrt,
                           float* __restrict__ wn, float* __restrict__ moved) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const size_t base = (size_t)row * D;
    const float c = cs[row];
    float n2 = 0.0f, d2 = 0.0f;
    for (int d = lane; d < D; d += 64) {
        const float w = W[base + d];
        const float g = temp * (dW[base + d] - c * w);
        const float m = M[base + d] + 0.1f * (g - M[base + d]);                 // exp_avg.lerp_(grad, 1 - beta1)
        const float v = fmaf(0.001f * g, g, 0.999f * V[base + d]);              // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
        const float denom = sqrtf(v) / bc2_sqrt + 1e-8f;
        const float wnew = w + neg_step * m / denom;                            // param.addcdiv_(exp_avg, denom, value=-step_size)
        M[base + d] = m;
        V[base + d] = v;
        W[base + d] = wnew;
        const float diff = w - wnew;
        d2 = fmaf(diff, diff, d2);
        n2 = fmaf(wnew, wnew, n2);
    }
    d2 = tim_wave_sum(d2);
    n2 = tim_wave_sum(n2);
    if (lane == 0) {
        wn[row] = n2;
        moved[row] = sqrtf(d2);
    }
}

// criterion of one batch (ALPHA_TIM: n = its tasks x classes) or of one task (TIM_GD: n = its classes): the mean of the
// block's n row displacements (fixed-order tree).  A displacement is the norm of a weight row of D elements (k_tim_adam);
// there are K of them per task whatever D is.
__global__ void k_tim_criterion(const float* __restrict__ moved, int n, float* __restrict__ out, int stride) {
    __shared__ float part[256];
    const float* m = moved + (size_t)blockIdx.x * n;
    float s = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) s += m[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * stride] = part[0] / (float)n;
}

// The workspace of both methods as typed pointers; a null `base` gives `bytes` alone.
// n_values > 0 (the sweep entry): the support class sums stay per task; every other region holds n_values * tasks solves, and
// the values follow as floats.  A region takes a whole number of 256-byte units PER VALUE (more than its contiguous contents
// need), so that the total is affine in n_values.
struct TimWs {
    float *sup, *cnt, *P, *xn, *wn, *marg, *cs, *dW, *M, *V, *moved, *alphas;
    size_t bytes;
};
static TimWs tim_ws(const tclip_problem& p, int dim, int n_values, char* base) {
    const size_t K = p.n_class, R = (size_t)p.n_support + p.n_query, D = dim, T = (size_t)p.n_batches * p.tasks_per_batch;
    const size_t P = n_values > 0 ? (size_t)n_values : 1;
    TimWs w;
    WsCursor c{base};
    auto take_per_value = [&](float*& ptr, size_t bytes, bool present = true) { c.take(ptr, P * align_up(bytes), present); };
    c.take(w.sup, T * K * D * 4);
    c.take(w.cnt, T * K * 4);
    take_per_value(w.P, T * R * K * 4);
    take_per_value(w.xn, T * R * 4);
    take_per_value(w.wn, T * K * 4);
    take_per_value(w.marg, T * K * 4);
    take_per_value(w.cs, T * K * 4);
    take_per_value(w.dW, T * K * D * 4);
    take_per_value(w.M, T * K * D * 4);
    take_per_value(w.V, T * K * D * 4);
    take_per_value(w.moved, T * K * 4);
    take_per_value(w.alphas, 4, n_values > 0);
    w.bytes = c.bytes;
    return w;
}

// The Adam loop of both methods on rows of D elements.  per_task = false (ALPHA_TIM): criterions [n_batches, iters], the mean over a
// batch's tasks and classes; per_task = true (TIM_GD, tim.py:181): criterions [iters, T], the mean over a task's classes.
// X: the task rows as the three kernels that touch them read them (k_tim_row_sqnorm and the two GEMMs of every step), x_s: the
// support rows as the class sums of init_weights read them - both dense, or both the feature tables in place (kIdx).
// values != nullptr (tclip_alpha_tim_sweep_tasks; X.n_real = the tasks): the loop runs over n_values * tasks solves in one set
// of launches per step, value-major.  Solve t reads the rows and labels of task t % tasks (X.real, k_tim_grad) and takes
// alpha = values[t / tasks]; the class means are computed once per task and written into every value's weights; a criterion is
// the mean over one batch's tasks within one value (criterions [n_values, n_batches, iters]).  No kernel mixes two solves, so
// each computes what the single-value loop computes for its task and its alpha.
template <bool kIdx>
static int tim_loop_on(const tclip_problem& p, const TimRows<kIdx>& X, const RowSrc& x_s, double lr, float temp, const TimLoss& loss,
                       bool per_task, const int64_t* y_s, float* weights, float* logits_q, int32_t* preds, float* criterions,
                       const TimWs& ws, hipStream_t st, const double* values = nullptr, int n_values = 0) {
    const int D = X.D;
    const int n_real = p.n_batches * p.tasks_per_batch, n_sweep = values ? n_values : 1;      // n_sweep * n_real <= 65535 (checked)
    const int Q = p.n_query, K = p.n_class, S = p.n_support, R = S + Q, B = p.n_batches * n_sweep, N = p.tasks_per_batch, T = B * N, TK = T * K;
    const int TR = T * R;
    float *const sup = ws.sup, *const cnt = ws.cnt, *const P = ws.P, *const xn = ws.xn, *const wn = ws.wn, *const marg = ws.marg;
    float *const cs = ws.cs, *const dW = ws.dW, *const M = ws.M, *const V = ws.V, *const moved = ws.moved, *const alphas = ws.alphas;
    if (values) launch_sweep_values(st, values, n_values, nullptr, alphas);
    const int tiles_k = (K + kTimTile - 1) / kTimTile, tiles_r = (R + kTimTile - 1) / kTimTile, tiles_d = (D + kTimTile - 1) / kTimTile;
    // init_weights (tim.py:115-134, :218-238): the class means of the support set (of the n_real tasks; one copy per value); Adam
    // state zero
    if (D == K)
        hipLaunchKernelGGL(k_support_stats, dim3(K, n_real), dim3(128), (size_t)S * sizeof(int), st, x_s, y_s, S, K, 0, sup, cnt);
    else
        launch_vis_support_stats(st, RowSrc{x_s.base, x_s.idx, nullptr}, y_s, n_real, S, K, D, sup, cnt);
    const size_t real_kd = (size_t)n_real * K * D;
    for (int v = 0; v < n_sweep; v++)
        hipLaunchKernelGGL(k_div_rows, dim3(ew_grid(real_kd)), dim3(256), 0, st, (const float*)sup, (const float*)cnt, real_kd, D,
                           weights + (size_t)v * real_kd);
    TCLIP_HIP(hipMemsetAsync(M, 0, (size_t)TK * D * 4, st));
    TCLIP_HIP(hipMemsetAsync(V, 0, (size_t)TK * D * 4, st));
    hipLaunchKernelGGL(k_tim_row_sqnorm<kIdx>, dim3((TR + 3) / 4), dim3(256), 0, st, X, TR, xn);
    hipLaunchKernelGGL(k_tim_w_sqnorm, dim3((TK + 3) / 4), dim3(256), 0, st, (const float*)weights, TK, D, wn);
    for (int it = 0; it < p.iters; it++) {
        const bool last = it + 1 == p.iters;
        hipLaunchKernelGGL((k_tim_gemm_mfma<false, kTimTile, kIdx>), dim3(tiles_k, tiles_r, T), dim3(256), 0, st, X, K, (const float*)weights,
                           (const float*)wn, (const float*)xn, temp, P, (float*)nullptr);
        hipLaunchKernelGGL(k_tim_softmax, dim3((TR + 3) / 4), dim3(256), 0, st, P, TR, S, Q, K, last ? logits_q : (float*)nullptr,
                           preds);
        hipLaunchKernelGGL(k_tim_marginal, dim3((K + 127) / 128, T), dim3(128), 0, st, (const float*)P, S, Q, K, marg);
        hipLaunchKernelGGL(k_tim_grad, dim3((TR + 3) / 4), dim3(256), 0, st, P, y_s, (const float*)marg, TR, S, Q, K, loss,
                           (const float*)alphas, n_real);
        hipLaunchKernelGGL((k_tim_gemm_mfma<true, kTimTile, kIdx>), dim3(tiles_d, tiles_k, T), dim3(256), 0, st, X, K, (const float*)P,
                           (const float*)nullptr, (const float*)nullptr, 0.0f, dW, cs);
        // Adam's step scalars, in double as torch computes them (torch/optim/adam.py, _single_tensor_adam)
        const double step = it + 1, bc1 = 1.0 - pow(0.9, step), bc2 = 1.0 - pow(0.999, step);
        hipLaunchKernelGGL(k_tim_adam, dim3((TK + 3) / 4), dim3(256), 0, st, weights, M, V, (const float*)dW, (const float*)cs, TK, D,
                           temp, (float)(-(lr / bc1)), (float)sqrt(bc2), wn, moved);
        if (per_task)
            hipLaunchKernelGGL(k_tim_criterion, dim3(T), dim3(256), 0, st, (const float*)moved, K, criterions + (size_t)it * T, 1);
        else
            hipLaunchKernelGGL(k_tim_criterion, dim3(B), dim3(256), 0, st, (const float*)moved, N * K, criterions + it, p.iters);
    }
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

// The rule of each method, and its one entry: the checks in the one order of DESIGN.md ("The method host drivers"), then the loop
// on the rows as given - dense, or the feature tables read in place in every step (TimRows<true>), with the dense workspace and
// the dense launches; a sweep (ALPHA_TIM) runs n_values * tasks solves of it.
static const MethodRule kAlphaTim{"ALPHA_TIM", true, kFewShotOnly, kItersForLogits, Limits::Rows};
static const MethodRule kTimGd{"TIM_GD", true, kFewShotOnly, kItersForLogits, Limits::Rows};

struct TimOutputs {
    float *weights, *logits_q;
    int32_t* preds;
    float* criterions;
    bool given() const { return weights && logits_q && preds && criterions; }
};

static int tim_run(const tclip_problem& p, const Rows& r, double lr, float temp, const TimLoss& loss, bool per_task, const int64_t* y_s,
                   const TimOutputs& out, void* workspace, void* stream) {
    const int D = r.D(p);
    const TimWs ws = tim_ws(p, D, r.n_sweep(), (char*)workspace);
    const RowSrc x_q = r.q(), x_s = r.s();
    if (r.tables)
        return tim_loop_on(p, TimRows<true>{x_s.base, x_q.base, x_s.idx, x_q.idx, x_s.cols, p.n_support, p.n_query, D,
                                            r.sweep ? p.n_batches * p.tasks_per_batch : 0},
                           x_s, lr, temp, loss, per_task, y_s, out.weights, out.logits_q, out.preds, out.criterions, ws,
                           (hipStream_t)stream, r.values, r.n_sweep());
    return tim_loop_on(p, TimRows<false>{x_s.base, x_q.base, p.n_support, p.n_query, D}, x_s, lr, temp, loss, per_task, y_s, out.weights,
                       out.logits_q, out.preds, out.criterions, ws, (hipStream_t)stream);
}

// ALPHA_TIM, all five forms (ws_query: the workspace query to name).  A sweep does not read prm->alpha_value.
static int alpha_tim_run(const tclip_problem* pp, const Rows& r, const tclip_tim_params* prm, const int64_t* y_s, const TimOutputs& out,
                         void* workspace, size_t workspace_bytes, void* stream, const char* ws_query) {
    if (int rc = check_method_problem(pp, r, kAlphaTim)) return rc;
    if (int rc = check_pointers(r, kAlphaTim, prm && y_s && out.given() && workspace)) return rc;
    for (int i = 0; i < 3; i++)
        if (prm->entropies[i] != TCLIP_TIM_SHANNON && prm->entropies[i] != TCLIP_TIM_ALPHA)
            return fail(TCLIP_ERR_ARG, "entropies must be TCLIP_TIM_SHANNON or TCLIP_TIM_ALPHA");
    if (int rc = check_values(pp, r)) return rc;
    const bool any_alpha = prm->entropies[0] || prm->entropies[1] || prm->entropies[2];
    for (int i = 0; i < (r.sweep ? r.n_values : 1); i++)
        if (any_alpha && !((r.sweep ? (float)r.values[i] : prm->alpha_value) != 1.0f))
            return fail(TCLIP_ERR_ARG, "alpha_value must differ from 1 for an Alpha entropy");
    if (int rc = check_workspace(workspace, workspace_bytes, tim_ws(*pp, r.D(*pp), r.n_sweep(), nullptr).bytes, ws_query)) return rc;
    const TimLoss loss{prm->loss_weights[0], prm->loss_weights[1], prm->loss_weights[2], r.sweep ? 0.0f : prm->alpha_value,
                       prm->entropies[0], prm->entropies[1], prm->entropies[2]};
    return tim_run(*pp, r, prm->lr, prm->temp, loss, false, y_s, out, workspace, stream);
}
static size_t alpha_tim_bytes(const tclip_problem* p, const Rows& r) {
    return query_accepts(p, r, kAlphaTim) ? tim_ws(*p, r.D(*p), r.n_sweep(), nullptr).bytes : 0;
}

// TIM_GD, both forms: dim is always given (dim == n_class: probability features, the only rows whose columns are permuted)
static int tim_gd_run(const tclip_problem* pp, const Rows& r, double lr, float temp, const float loss_weights[3], const int64_t* y_s,
                      const TimOutputs& out, void* workspace, size_t workspace_bytes, void* stream, const char* ws_query) {
    if (int rc = check_method_problem(pp, r, kTimGd)) return rc;
    if (int rc = check_pointers(r, kTimGd, loss_weights && y_s && out.given() && workspace, true)) return rc;
    if (r.tables && r.src->cols && r.dim != pp->n_class)
        return fail(TCLIP_ERR_ARG, "TIM_GD permutes columns on probability features only: cols must be NULL unless dim == n_class");
    if (int rc = check_workspace(workspace, workspace_bytes, tim_ws(*pp, r.dim, 0, nullptr).bytes, ws_query)) return rc;
    // tim.py:166-175: all three entropies Shannon, the marginal one with 1e-12 inside its logarithm
    const TimLoss loss{loss_weights[0], loss_weights[1], loss_weights[2], 0.0f, TCLIP_TIM_SHANNON, kTimMarginalGd, TCLIP_TIM_SHANNON};
    return tim_run(*pp, r, lr, temp, loss, true, y_s, out, workspace, stream);
}

}  // namespace tclip

extern "C" {

// ---- ALPHA_TIM.  Its queries look at neither iters nor n_support.  The _tasks forms read the task rows in place in
// k_tim_row_sqnorm, the two GEMMs of every Adam step and the class sums of init_weights; neither x_s nor x_q is built, workspace
// and checks are the dense entries'.
constexpr unsigned kAlphaTimQuery = kAnyIters | kAnySupport;
size_t tclip_alpha_tim_workspace_bytes(const tclip_problem* p) { return alpha_tim_bytes(p, rows_dense(nullptr, nullptr, kAlphaTimQuery)); }
size_t tclip_alpha_tim_tasks_workspace_bytes(const tclip_problem* p) { return alpha_tim_bytes(p, rows_tables(nullptr, kAlphaTimQuery)); }
size_t tclip_alpha_tim_visual_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return alpha_tim_bytes(p, rows_visual(dim, nullptr, nullptr, kAlphaTimQuery));
}
size_t tclip_alpha_tim_visual_tasks_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return alpha_tim_bytes(p, rows_visual_tables(dim, nullptr, kAlphaTimQuery));
}
size_t tclip_alpha_tim_sweep_tasks_workspace_bytes(const tclip_problem* p, int32_t dim, int32_t n_values) {
    return alpha_tim_bytes(p, rows_sweep(dim, nullptr, nullptr, n_values, kAlphaTimQuery));
}

int tclip_alpha_tim_run(const tclip_problem* pp, const tclip_tim_params* prm, const float* x_q, const float* x_s,
                        const int64_t* y_s, float* weights, float* logits_q, int32_t* preds, float* criterions,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return alpha_tim_run(pp, rows_dense(x_q, x_s), prm, y_s, {weights, logits_q, preds, criterions}, workspace, workspace_bytes, stream,
                         "tclip_alpha_tim_workspace_bytes");
}

int tclip_alpha_tim_visual_run(const tclip_problem* pp, int32_t dim, const tclip_tim_params* prm, const float* x_q, const float* x_s,
                               const int64_t* y_s, float* weights, float* logits_q, int32_t* preds, float* criterions,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return alpha_tim_run(pp, rows_visual(dim, x_q, x_s), prm, y_s, {weights, logits_q, preds, criterions}, workspace, workspace_bytes,
                         stream, "tclip_alpha_tim_visual_workspace_bytes");
}

int tclip_alpha_tim_run_tasks(const tclip_problem* pp, const tclip_tim_params* prm, const tclip_task_source* src, const int64_t* y_s,
                              float* weights, float* logits_q, int32_t* preds, float* criterions, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return alpha_tim_run(pp, rows_tables(src), prm, y_s, {weights, logits_q, preds, criterions}, workspace, workspace_bytes, stream,
                         "tclip_alpha_tim_tasks_workspace_bytes");
}

int tclip_alpha_tim_visual_run_tasks(const tclip_problem* pp, int32_t dim, const tclip_tim_params* prm, const tclip_task_source* src,
                                     const int64_t* y_s, float* weights, float* logits_q, int32_t* preds, float* criterions,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return alpha_tim_run(pp, rows_visual_tables(dim, src), prm, y_s, {weights, logits_q, preds, criterions}, workspace, workspace_bytes,
                         stream, "tclip_alpha_tim_visual_tasks_workspace_bytes");
}

// ALPHA_TIM for a list of alpha values on the same tasks (see tim_loop_on)
int tclip_alpha_tim_sweep_tasks(const tclip_problem* pp, int32_t dim, const tclip_tim_params* prm, const tclip_task_source* src,
                                const int64_t* y_s, const double* values, int32_t n_values, float* weights, float* logits_q,
                                int32_t* preds, float* criterions, void* workspace, size_t workspace_bytes, void* stream) {
    return alpha_tim_run(pp, rows_sweep(dim, src, values, n_values), prm, y_s, {weights, logits_q, preds, criterions}, workspace,
                         workspace_bytes, stream, "tclip_alpha_tim_sweep_tasks_workspace_bytes");
}

// ---- TIM_GD: the queries make every check of the problem that the entries make
size_t tclip_tim_gd_workspace_bytes(const tclip_problem* p, int32_t dim) {
    return query_accepts(p, rows_visual(dim, nullptr, nullptr), kTimGd) ? tim_ws(*p, dim, 0, nullptr).bytes : 0;
}
size_t tclip_tim_gd_tasks_workspace_bytes(const tclip_problem* p, int32_t dim) { return tclip_tim_gd_workspace_bytes(p, dim); }

int tclip_tim_gd_run(const tclip_problem* pp, int32_t dim, double lr, float temp, const float loss_weights[3], const float* x_q,
                     const float* x_s, const int64_t* y_s, float* weights, float* logits_q, int32_t* preds, float* criterions,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return tim_gd_run(pp, rows_visual(dim, x_q, x_s), lr, temp, loss_weights, y_s, {weights, logits_q, preds, criterions}, workspace,
                      workspace_bytes, stream, "tclip_tim_gd_workspace_bytes");
}

int tclip_tim_gd_run_tasks(const tclip_problem* pp, int32_t dim, double lr, float temp, const float loss_weights[3],
                           const tclip_task_source* src, const int64_t* y_s, float* weights, float* logits_q, int32_t* preds,
                           float* criterions, void* workspace, size_t workspace_bytes, void* stream) {
    return tim_gd_run(pp, rows_visual_tables(dim, src), lr, temp, loss_weights, y_s, {weights, logits_q, preds, criterions}, workspace,
                      workspace_bytes, stream, "tclip_tim_gd_tasks_workspace_bytes");
}

}  // extern "C"
