// The penalised clustering objective the EM-Dirichlet loop descends, as four float64 terms per task and outer iteration
// (reference: objective_function, src/methods/zero_shot/hard_em_dirichlet.py:179-198, few_shot/hard_em_dirichlet.py:149-168,
// which the reference defines and never calls).  Included by tclip_kernels.hip inside namespace tclip, after the E-step
// kernels; launched by em_estep behind k_softmax, only for the objective entries (tclip_em_dirichlet_run_objective).
//
//   terms[t, it, 0] = fit_q = sum_n sum_k u[n,k] * logit0[n,k]            logit0: the E-step's fp32 logits, get_logits(query)
//   terms[t, it, 1] = fit_s = sum_k cnt[k] * rowc[k] + sum_k sum_d (alpha[k,d] - 1) * sup[k,d]        (0 in zero-shot)
//   terms[t, it, 2] = ent   = sum_n sum_k u * log(u + 1e-15)
//   terms[t, it, 3] = part  = sum_k p_k * log(p_k + 1e-15),  p_k = (sum_n u[n,k]) / Q
// objective = -(fit_q + fit_s) / 2 + ent - lambd * part is composed by the caller.
//
// Everything is read as fp32 and summed in float64 in an order that depends on (Q, K) alone: no atomics, no dependence on the
// grid, the stream group or what shares the call, so a task's terms have the same bits whatever runs with it.
// `done` (optional, with the until-stable schedule): rows and tasks of a batch b with done[b] set are left alone; their terms
// stay as the entry zero-filled them.

constexpr double kObjEps = 1e-15;

// One 16-lane group per (task, query) row, the layout of k_softmax: lane l takes k = l, l + 16, ...; the two partial sums are
// folded by a 16-lane butterfly (addition commutes, so all lanes hold the same bits) and lane 0 writes rowterms[r] =
// {sum_k u * logit0, sum_k u * log(u + eps)}.  u == 0 contributes exactly 0 to the entropy and skips the logarithm (a one-hot
// row evaluates one).
__global__ __launch_bounds__(256) void k_objective_rows(const float* __restrict__ logit0, const float* __restrict__ u, int TQ, int K,
                                                        double* __restrict__ rowterms, const int32_t* __restrict__ done,
                                                        int rows_per_batch) {
    const int lane = threadIdx.x & 15;
    const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (r >= TQ) return;
    if (done && done[r / rows_per_batch]) return;       // the whole 16-lane group of a row leaves together
    const float* x = logit0 + (size_t)r * K;
    const float* ur = u + (size_t)r * K;
    double fit = 0.0, ent = 0.0;
    for (int k = lane; k < K; k += 16) {
        const double uk = (double)ur[k];
        fit += uk * (double)x[k];
        if (uk != 0.0) ent += uk * log(uk + kObjEps);
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        fit += __shfl_xor(fit, m, 16);
        ent += __shfl_xor(ent, m, 16);
    }
    if (lane == 0) {
        rowterms[2 * (size_t)r] = fit;
        rowterms[2 * (size_t)r + 1] = ent;
    }
}

// the sum of one value per thread over a block of 256 threads, a fixed tree through LDS; valid in thread 0
__device__ __forceinline__ double objective_block_sum(double v, double* sh) {
    __syncthreads();                                    // the previous use of sh has been read
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// One block of 256 threads per task: the Q row terms summed in index order; the column sums of u over the queries in index
// order, consecutive lanes on consecutive k; in few-shot (sup != null) the K x K reduction of fit_s, thread i on the elements
// i, i + 256, ... of the task's alpha and sup.  Per-thread partial sums meet in objective_block_sum.  Thread 0 writes the four
// doubles of (t, it); `stride` = iters, the terms' row length per task.
__global__ __launch_bounds__(256) void k_objective_task(const double* __restrict__ rowterms, const float* __restrict__ u,
                                                        const float* __restrict__ alpha, const float* __restrict__ sup,
                                                        const float* __restrict__ cnt, const float* __restrict__ rowc, int Q, int K,
                                                        int it, int stride, double* __restrict__ terms,
                                                        const int32_t* __restrict__ done, int tasks_per_batch) {
    __shared__ double sh[256];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (done && done[t / tasks_per_batch]) return;      // block-uniform
    double fit_q = 0.0, ent = 0.0;
    if (tid < 2) {                                      // thread 0: fit_q, thread 1: ent
        const double* rt = rowterms + 2 * (size_t)t * Q + tid;
        double s = 0.0;
        for (int n = 0; n < Q; n++) s += rt[2 * (size_t)n];
        fit_q = s;
    }
    ent = __shfl(fit_q, 1, 64);
    const float* ut = u + (size_t)t * Q * K;
    double part = 0.0;
    for (int k = tid; k < K; k += 256) {
        double s = 0.0;
        for (int n = 0; n < Q; n++) s += (double)ut[(size_t)n * K + k];
        const double p = s / (double)Q;
        part += p * log(p + kObjEps);
    }
    part = objective_block_sum(part, sh);
    double fit_s = 0.0;
    if (sup) {
        const size_t KK = (size_t)K * K, base = (size_t)t * KK;
        for (size_t i = tid; i < KK; i += 256) fit_s += ((double)alpha[base + i] - 1.0) * (double)sup[base + i];
        for (int k = tid; k < K; k += 256) fit_s += (double)cnt[(size_t)t * K + k] * (double)rowc[(size_t)t * K + k];
        fit_s = objective_block_sum(fit_s, sh);
    }
    if (tid == 0) {
        double* o = terms + ((size_t)t * stride + it) * 4;
        o[0] = fit_q;
        o[1] = fit_s;
        o[2] = ent;
        o[3] = part;
    }
}
