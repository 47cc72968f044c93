// Kernels and launchers of zero-shot SOFT_KMEANS, HARD_KMEANS and EM_GAUSSIAN on VISUAL features (the reference's
// use_softmax_feature == False; src/methods/zero_shot/{soft_kmeans,hard_kmeans,em_gaussian}.py): included at the end of
// tclip_kernels.hip, uses its helpers (fail, dsum_outer, dev_ceil_log2, k_probability_features).
//
// The loop is the one of the probability-feature path (kmeans_loop, tclip_methods.inc), but the clustering runs in the
// D-dimensional embedding space, D independent of the class count K: centroids w are [T, K, D], queries z are the raw
// embeddings [T, Q, D].  The two kernels
// whose work grows with D are new here; the softmax, the first-minimum one-hot, the criterion and the v term only see
// [T, Q, K] / [T, K] tensors and are the library's own.
//   * k_vis_dist: logit[t,q,k] = temperature * (pre * sum_d (w[t,k,d] - z[t,q,d])^2) in torch's last-dim order for every D
//     in 1..1024, including the cascade dumps after 16 and 32 eight-float steps per accumulator (D >= 512, D = 1024).
//   * k_vis_mstats: the centroid statistics sum_q u[t,q,k] z[t,q,d] in the order of torch's
//     (z.unsqueeze(2) * u.unsqueeze(3)).sum(1): an outer sum over K*D contiguous columns (k_mstats for D = K).
//   * EM_GAUSSIAN_COV (em_gaussian_cov.py; driver em_gaussian_cov_loop): k_vis_mstats<true> gives the inverse variances s in the
//     same outer-sum order, k_vis_dist<true> the Mahalanobis sums in the same last-dim order with s in a second LDS tile,
//     k_vis_logdet the half log-determinants once per class and iteration.
//   * k_vis_prototypes: the accuracy tail's cluster prototypes (one-hot statistics of the predictions) of D-dim rows.

namespace tclip {

// ---- squared distances ------------------------------------------------------------------------------------------------
// One lane per class as k_kmeans_logits_tile: a block stages up to 64 centroids in LDS (odd row stride), each wavefront takes
// one query at a time (wave-uniform: its values arrive through the scalar cache), lane k keeps torch's 32 partial sums
// (accumulator r = 0..3, vector lane j = 0..7: element d = 32 m + 8 r + j belongs to slot 8 r + j at step m) plus the
// cascade's second level in registers.  Rows of up to 512 elements are staged once; longer rows (at most 1024) in two
// chunks of 512 elements, which is where torch's 16-step cascade block ends: the chunks are restaged for every group of
// n_waves queries, so that each wavefront carries one query's 64 accumulators across the chunk boundary and no more.
// Rows of fewer than 8 elements take torch's 4-way scalar row sum instead (cascade_sum: no vector is complete).
//
// kCov, EM_GAUSSIAN_COV's E-step (em_gaussian_cov.py:106-129): every squared difference is multiplied by the cluster's inverse
// variance s[t,k,d] before it is added (square and product rounded one after the other, as diff.square_().mul_(s) does), and
// logit[t,q,k] = -1/2 sum + det[t,k], det the half log-determinant k_vis_logdet left.  The same sums in the same order; a second
// LDS tile holds s, so a chunk is 256 elements (8 of the cascade's 16 steps: the dumps fall on chunk ends all the same) and
// rows of more than 256 elements are restaged for every group of queries.
constexpr int kVisTile = 64, kVisChunk = 512, kVisCovChunk = 256, kVisThreads = 1024;
constexpr int kVisLds = kVisTile * (kVisChunk + 1) * (int)sizeof(float);
constexpr int kVisCovLds = 2 * kVisTile * (kVisCovChunk + 1) * (int)sizeof(float);

template <bool kCov>
__global__ __launch_bounds__(kVisThreads) void k_vis_dist(const float* __restrict__ w, const float* __restrict__ z,
                                                          const uint8_t* __restrict__ need, int Q, int K, int D, float pre,
                                                          float temperature, float* __restrict__ logit0,
                                                          const float* __restrict__ s, const float* __restrict__ det) {
    extern __shared__ float wt[];                                   // [kVisTile][stride]; kCov: s's tile behind it
    constexpr int kChunk = kCov ? kVisCovChunk : kVisChunk, kChunkSteps = kChunk / 32;
    const int t = blockIdx.y, k0 = blockIdx.x * kVisTile;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n_waves = blockDim.x >> 6;
    const int k = k0 + lane;
    const bool ok = k < K && need[(size_t)t * K + k];
    if (!__syncthreads_or(ok)) return;                              // no class of the tile moved
    const int rows = K - k0 < kVisTile ? K - k0 : kVisTile;
    const int n_chunks = (D + kChunk - 1) / kChunk;
    const int stride = (D < kChunk ? D : kChunk) | 1;
    const int s_off = kVisTile * stride;                            // kCov: s's element lies s_off words behind w's
    const float* wsrc = w + ((size_t)t * K + k0) * D;
    const float* ssrc = kCov ? s + ((size_t)t * K + k0) * D : nullptr;
    auto stage_one = [&](const float* src, float* dst, int c0, int clen) {     // rows x clen words, eight loads in flight per thread
        const int n = rows * clen, step = blockDim.x;
        for (int i0 = threadIdx.x; i0 < n; i0 += 8 * step) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int i = i0 + j * step;
                v[j] = i < n ? src[(size_t)(i / clen) * D + c0 + i % clen] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int i = i0 + j * step;
                if (i < n) dst[(i / clen) * stride + i % clen] = v[j];
            }
        }
    };
    auto stage = [&](int c0, int clen) {
        stage_one(wsrc, wt, c0, clen);
        if (kCov) stage_one(ssrc, wt + s_off, c0, clen);
    };
    // one term of the row sum: element d of the lane's row at p[d]
    auto term = [&](const float* p, int d, float zv) {
        const float df = p[d] - zv;
        return kCov ? (df * df) * p[s_off + d] : df * df;
    };
    const float* wl = wt + (lane < rows ? lane : rows - 1) * stride;    // lanes beyond the last class recompute it; nothing is stored
    const int vec_size = D >> 3, size_ilp = vec_size >> 2, nleft = vec_size - 4 * size_ilp, ntail = D - 8 * vec_size;
    if (n_chunks == 1) {
        stage(0, D);
        __syncthreads();
    }
    for (int qb = 0; qb < Q; qb += n_waves) {                       // the same trip count in every wavefront (block barriers inside)
        const int q = qb + wave;
        const float* zq = z + ((size_t)t * Q + (q < Q ? q : Q - 1)) * D;     // wave-uniform: scalar loads
        float a0[32], a1[32];
#pragma unroll
        for (int sl = 0; sl < 32; sl++) a0[sl] = a1[sl] = 0.0f;
        for (int c = 0; c < n_chunks; c++) {
            const int c0 = c * kChunk;
            if (n_chunks > 1) {
                __syncthreads();                                    // every wavefront is done with the previous chunk
                stage(c0, D - c0 < kChunk ? D - c0 : kChunk);
                __syncthreads();
            }
            const float* wc = wl - c0;                              // element d of the row at wc[d]
            const int m_end = size_ilp < (c + 1) * kChunkSteps ? size_ilp : (c + 1) * kChunkSteps;
            for (int m = c * kChunkSteps; m < m_end; m++) {
                float zc[32];
#pragma unroll
                for (int sl = 0; sl < 32; sl++) zc[sl] = zq[32 * m + sl];
#pragma unroll
                for (int sl = 0; sl < 32; sl++) a0[sl] += term(wc, 32 * m + sl, zc[sl]);
                if ((m & 15) == 15) {                               // end of a 16-step cascade block: level 0 into level 1
#pragma unroll
                    for (int sl = 0; sl < 32; sl++) { a1[sl] += a0[sl]; a0[sl] = 0.0f; }
                }
            }
        }
        if (q >= Q) continue;                                       // wave-uniform; after the last barrier of this query group
        const float* wc = wl - (n_chunks - 1) * kChunk;             // the leftovers and the tail lie in the last chunk
        float fin = 0.0f;
        if (vec_size == 0) {                                        // D < 8: row_sum of 4 interleaved scalar partials
            const int ilp = D >> 2;
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float x = 0.0f;
                if (r < 4 * ilp) x += term(wc, r, zq[r]);
                p[r] = x;
            }
            for (int i = 4 * ilp; i < D; i++) p[0] += term(wc, i, zq[i]);
            fin = p[0];
            fin += p[1];
            fin += p[2];
            fin += p[3];
        } else {
#pragma unroll
            for (int sl = 0; sl < 32; sl++) a0[sl] += a1[sl];       // multi_row_sum's finish (levels 2 and 3 hold +0)
            int d = 32 * size_ilp;
            for (int i = 0; i < nleft; i++, d += 8) {               // whole vectors beyond the 4-way part join accumulator 0
#pragma unroll
                for (int j = 0; j < 8; j++) a0[j] += term(wc, d + j, zq[d + j]);
            }
            for (int i = 0; i < ntail; i++) fin += term(wc, d + i, zq[d + i]);     // the D mod 8 tail first
#pragma unroll
            for (int j = 0; j < 8; j++) {
                float p0 = a0[j];
                p0 += a0[8 + j];
                p0 += a0[16 + j];
                p0 += a0[24 + j];
                fin += p0;
            }
        }
        if (ok) logit0[((size_t)t * Q + q) * K + k] = kCov ? -0.5f * fin + det[(size_t)t * K + k] : temperature * (pre * fin);
    }
}

template <bool kCov>
static bool vis_dist_lds_raised() {
    struct Seen { int device; bool ok; };
    static std::mutex mu;
    static std::vector<Seen> seen;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(mu);
    for (auto& e : seen)
        if (e.device == dev) return e.ok;
    const bool ok = hipFuncSetAttribute((const void*)k_vis_dist<kCov>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        kCov ? kVisCovLds : kVisLds) == hipSuccess;
    seen.push_back(Seen{dev, ok});
    return ok;
}

static int launch_vis_dist(int T, hipStream_t st, const float* w, const float* z, const uint8_t* need, int Q, int K, int D,
                           float pre, float temperature, float* logit0) {
    const int stride = (D < kVisChunk ? D : kVisChunk) | 1;
    const size_t lds = (size_t)kVisTile * stride * sizeof(float);
    if (lds > 65536 && !vis_dist_lds_raised<false>()) return fail(TCLIP_ERR_HIP, "k_vis_dist: cannot raise the LDS limit to %s bytes", "131328");
    hipLaunchKernelGGL(k_vis_dist<false>, dim3((K + kVisTile - 1) / kVisTile, T), dim3(kVisThreads), lds, st, w, z, need, Q, K, D, pre,
                       temperature, logit0, (const float*)nullptr, (const float*)nullptr);
    return TCLIP_OK;
}

// ---- EM_GAUSSIAN_COV's half log-determinants ------------------------------------------------------------------------------
// det[t,k] = 1/2 sum_d log(s[t,k,d] + eps) for the classes `need` marks, once per class and iteration: the sum in torch's
// last-dim order (dsum_inner_serial's, its eight vector lanes on eight threads), the logarithm MKL's vsLn as in k_cov_logits_rows.
// One wavefront per class row: the logarithms are taken 64 elements at a time and parked in LDS.
constexpr int kVisDetWaves = 4, kVisDetMaxD = 1024;

__global__ __launch_bounds__(64 * kVisDetWaves) void k_vis_logdet(const float* __restrict__ s, const uint8_t* __restrict__ need, int TK,
                                                                  int D, float* __restrict__ det) {
    __shared__ float lg[kVisDetWaves][kVisDetMaxD];
    __shared__ float part[kVisDetWaves][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * kVisDetWaves + wave;
    const bool on = row < TK && need[row < TK ? row : 0];
    float* l = lg[wave];
    if (on) {
        const float* sr = s + (size_t)row * D;
        for (int d = lane; d < D; d += 64) l[d] = log_f32(sr[d] + kEpsF);
    }
    __syncthreads();
    auto get = [&](int d) { return l[d]; };
    if (on && D >= 8 && lane < 8) part[wave][lane] = dsum_inner_lane(D, lane, get);
    __syncthreads();
    if (!on || lane != 0) return;
    float fin = 0.0f;
    if (D < 8) {
        fin = dsum_ilp4(D, get);
    } else {
        for (int d = (D >> 3) * 8; d < D; d++) fin += l[d];
        for (int jj = 0; jj < 8; jj++) fin += part[wave][jj];
    }
    det[row] = 0.5f * fin;
}

// logit[t,q,k] = -1/2 sum_d (w[t,k,d] - z[t,q,d])^2 s[t,k,d] + 1/2 sum_d log(s[t,k,d] + eps) for the classes `need` marks
static int launch_vis_cov_logits(int T, hipStream_t st, const float* w, const float* s, const float* z, const uint8_t* need, int Q,
                                 int K, int D, float* det, float* logit0) {
    const int TK = T * K;
    hipLaunchKernelGGL(k_vis_logdet, dim3((TK + kVisDetWaves - 1) / kVisDetWaves), dim3(64 * kVisDetWaves), 0, st, s, need, TK, D, det);
    const int stride = (D < kVisCovChunk ? D : kVisCovChunk) | 1;
    const size_t lds = (size_t)2 * kVisTile * stride * sizeof(float);
    if (lds > 65536 && !vis_dist_lds_raised<true>()) return fail(TCLIP_ERR_HIP, "k_vis_dist: cannot raise the LDS limit to %s bytes", "131584");
    hipLaunchKernelGGL(k_vis_dist<true>, dim3((K + kVisTile - 1) / kVisTile, T), dim3(kVisThreads), lds, st, w, z, need, Q, K, D, 0.0f,
                       0.0f, logit0, s, (const float*)det);
    return TCLIP_OK;
}

// ---- centroid statistics ---------------------------------------------------------------------------------------------
// y[t,k,d] = sum_q u[t,q,k] z[t,q,d] / max(cs[t,k], eps) with the sum in torch's outer-sum order over the K*D contiguous
// columns of a task (dsum_outer).  mode 0: only rows `live` marks are written (w_init passes all-ones, w_update of SOFT_KMEANS /
// EM_GAUSSIAN keeps the centroid of an empty cluster); mode 1: HARD_KMEANS, rows that are not live get the quotient times 0
// (num / den * nonzero_clusters, hard_kmeans.py:148-150), whose sign torch keeps.
// The few-shot modes write every row and ignore `live`: mode 2, PADDLE's w_update (few_shot/paddle.py:154-158), adds the support
// class sums to the query sum and the class counts to cs, one add_ each, then divides; mode 3, BD-CSPN's rectified prototypes
// (few_shot/bdcspn.py:139-141), is the plain quotient.  Q is then any row count (BD-CSPN: S + n_query augmented rows).
// The rows kernel: one thread per column d, kVisRows classes per thread (u wave-uniform, each z value read once per
// kVisRows classes), for the classes whose columns all take the cascade order; k_vis_mstats_one the last few.
// kCov: the inverse diagonal covariances of EM_GAUSSIAN_COV (em_gaussian_cov.py:172-193) for the rows `live` marks,
//   y[t,k,d] = cs[t,k] / max(sum_q (wc[t,k,d] - z[t,q,d])^2 * u[t,q,k], eps),
// the same outer sum over the same K*D columns with the square and the product by u rounded one after the other
// (k_mstats*<true> for D = K); `mode` is 0.
constexpr int kVisRows = 16;

__device__ __forceinline__ void vis_mstats_put(float* y, size_t idx, float s, float c, bool alive, int mode,
                                               const float* __restrict__ sup, const float* __restrict__ cnt, size_t row) {
    if (mode == 2) { y[idx] = (s + sup[idx]) / (c + cnt[row]); return; }
    if (mode == 3) { y[idx] = s / c; return; }
    const float r = s / (c < kEpsF ? kEpsF : c);
    if (alive) y[idx] = r;
    else if (mode == 1) y[idx] = r * 0.0f;
}

template <bool kCov>
__global__ __launch_bounds__(64) void k_vis_mstats(const float* __restrict__ u, const float* __restrict__ z,
                                                   const float* __restrict__ cs, const uint8_t* __restrict__ live, int Q, int K,
                                                   int D, int mode, float* __restrict__ y, const float* __restrict__ sup,
                                                   const float* __restrict__ cnt, const float* __restrict__ wc) {
    const int t = blockIdx.z, k0 = blockIdx.y * kVisRows;
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    if (mode == 0) {   // nothing is stored for rows that are not live: skip the group when none of its rows is (block-uniform)
        bool any = false;
#pragma unroll
        for (int j = 0; j < kVisRows; j++) any = any || (k0 + j < K && live[(size_t)t * K + k0 + j]);
        if (!any) return;
    }
    const float* ut = u + (size_t)t * Q * K + k0;
    const float* zt = z + (size_t)t * Q * D + d;
    const int nj = K - k0 < kVisRows ? K - k0 : kVisRows;
    float wcv[kVisRows];
#pragma unroll
    for (int j = 0; j < kVisRows; j++) wcv[j] = kCov && j < nj ? wc[((size_t)t * K + k0 + j) * D + d] : 0.0f;
    auto term = [&](int j, float uv, float fv) {
        if (kCov) {
            const float df = wcv[j] - fv;
            return (df * df) * uv;
        }
        return uv * fv;
    };
    const int cl = dev_ceil_log2(Q) / 4;
    const int level_power = cl > 4 ? cl : 4;
    const int step = 1 << level_power, mask = step - 1;
    float a0[kVisRows], a1[kVisRows], a2[kVisRows], a3[kVisRows];
#pragma unroll
    for (int j = 0; j < kVisRows; j++) a0[j] = a1[j] = a2[j] = a3[j] = 0.0f;
    int i = 0;
    for (; i + step <= Q;) {
        for (int jj = 0; jj < step; ++jj, ++i) {
            const float fv = zt[(size_t)i * D];
#pragma unroll
            for (int j = 0; j < kVisRows; j++) a0[j] += term(j, j < nj ? ut[(size_t)i * K + j] : 0.0f, fv);
        }
        const bool l2 = (i & (mask << level_power)) == 0, l3 = l2 && (i & (mask << (2 * level_power))) == 0;
#pragma unroll
        for (int j = 0; j < kVisRows; j++) {
            a1[j] += a0[j]; a0[j] = 0.0f;
            if (l2) { a2[j] += a1[j]; a1[j] = 0.0f; }
            if (l3) { a3[j] += a2[j]; a2[j] = 0.0f; }
        }
    }
    for (; i < Q; ++i) {
        const float fv = zt[(size_t)i * D];
#pragma unroll
        for (int j = 0; j < kVisRows; j++) a0[j] += term(j, j < nj ? ut[(size_t)i * K + j] : 0.0f, fv);
    }
#pragma unroll
    for (int j = 0; j < kVisRows; j++) {
        if (j >= nj) continue;
        const size_t row = (size_t)t * K + k0 + j;
        float s = a0[j];
        s += a1[j];
        s += a2[j];
        s += a3[j];
        if (kCov) {
            if (live[row]) y[row * D + d] = cs[row] / (s < kEpsF ? kEpsF : s);
            continue;
        }
        vis_mstats_put(y, row * D + d, s, cs[row], live[row] != 0, mode, sup, cnt, row);
    }
}

// One output per thread, any column (the rows of the 4-way row-sum columns: at most the last 31 of K*D).
template <bool kCov>
__global__ void k_vis_mstats_one(const float* __restrict__ u, const float* __restrict__ z, const float* __restrict__ cs,
                                 const uint8_t* __restrict__ live, int Q, int K, int D, int k_first, int mode, float* __restrict__ y,
                                 const float* __restrict__ sup, const float* __restrict__ cnt, const float* __restrict__ wc) {
    const int t = blockIdx.z, k = blockIdx.y + k_first;
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const size_t row = (size_t)t * K + k;
    if (mode == 0 && !live[row]) return;
    const float* ut = u + (size_t)t * Q * K + k;
    const float* zt = z + (size_t)t * Q * D + d;
    const float wcv = kCov ? wc[row * D + d] : 0.0f;
    const float s = dsum_outer(Q, (long)k * D + d, (long)K * D, [&](int q) {
        if (kCov) {
            const float df = wcv - zt[(size_t)q * D];
            return (df * df) * ut[(size_t)q * K];
        }
        return ut[(size_t)q * K] * zt[(size_t)q * D];
    });
    if (kCov) {
        y[row * D + d] = cs[row] / (s < kEpsF ? kEpsF : s);      // mode 0: the row is live
        return;
    }
    vis_mstats_put(y, row * D + d, s, cs[row], live[row] != 0, mode, sup, cnt, row);
}

template <bool kCov>
static void launch_vis_mstats_mode(hipStream_t st, const float* u, const float* z, const float* cs, const uint8_t* live, int T, int Q,
                                   int K, int D, int mode, float* y, const float* sup, const float* cnt, const float* wc) {
    const long ncols = (long)K * D;
    const int full_rows = ncols >= 8 ? (int)(((ncols / 32) * 32) / D) : 0;     // rows 0 .. full_rows-1 are all-cascade
    const int groups = full_rows / kVisRows;
    if (groups > 0)
        hipLaunchKernelGGL(k_vis_mstats<kCov>, dim3((D + 63) / 64, groups, T), dim3(64), 0, st, u, z, cs, live, Q, K, D, mode, y, sup,
                           cnt, wc);
    const int k_first = groups * kVisRows;
    if (k_first < K)
        hipLaunchKernelGGL(k_vis_mstats_one<kCov>, dim3((D + 63) / 64, K - k_first, T), dim3(64), 0, st, u, z, cs, live, Q, K, D, k_first,
                           mode, y, sup, cnt, wc);
}
static void launch_vis_mstats(hipStream_t st, const float* u, const float* z, const float* cs, const uint8_t* live, int T, int Q,
                              int K, int D, int mode, float* y, const float* sup = nullptr, const float* cnt = nullptr) {
    launch_vis_mstats_mode<false>(st, u, z, cs, live, T, Q, K, D, mode, y, sup, cnt, nullptr);
}
// EM_GAUSSIAN_COV: s = cs / max(sum_q (w - z_q)^2 u, eps) for the rows `live` marks
static void launch_vis_cov_stats(hipStream_t st, const float* u, const float* z, const float* cs, const uint8_t* live, const float* w,
                                 int T, int Q, int K, int D, float* s) {
    launch_vis_mstats_mode<true>(st, u, z, cs, live, T, Q, K, D, 0, s, nullptr, nullptr, w);
}

// ---- accuracy-tail prototypes -----------------------------------------------------------------------------------------
// Per task the clusters present in preds in first-appearance order and their mean raw feature, as compute_acc_clustering
// builds it (soft_kmeans.py:36-44): (one_hot(preds).unsqueeze(-1) * z.unsqueeze(2)).sum(1) / clamp(sizes, eps), the sum in
// the outer-sum order of K*D columns (the one-hot's zero products included: they decide nothing but are added all the same).
// One block per task; only the present clusters' rows are computed.
__global__ __launch_bounds__(256) void k_vis_prototypes(const int32_t* __restrict__ preds, const float* __restrict__ z, int Q, int K,
                                                        int D, int Cmax, int32_t* __restrict__ n_clusters,
                                                        int32_t* __restrict__ cluster_ids, float* __restrict__ protos) {
    const int t = blockIdx.x;
    __shared__ int ids[1024];
    __shared__ int cnt;
    __shared__ float sizes[1024];
    if (threadIdx.x == 0) {
        int c = 0;
        for (int q = 0; q < Q; q++) {
            int p = preds[(size_t)t * Q + q];
            p = p < 0 ? 0 : (p >= K ? K - 1 : p);          // never index outside the task (the host side rejects such labels)
            bool seen = false;
            for (int i = 0; i < c; i++) seen |= ids[i] == p;
            if (!seen) ids[c++] = p;
        }
        cnt = c;
        n_clusters[t] = c;
        for (int i = 0; i < Cmax; i++) cluster_ids[(size_t)t * Cmax + i] = i < c ? ids[i] : -1;
    }
    __syncthreads();
    const int c = cnt;
    const int32_t* pt = preds + (size_t)t * Q;
    for (int ci = threadIdx.x; ci < c; ci += blockDim.x) {
        const int k = ids[ci];
        sizes[ci] = dsum_outer(Q, k, K, [&](int q) { return pt[q] == k ? 1.0f : 0.0f; });
    }
    __syncthreads();
    const float* zt = z + (size_t)t * Q * D;
    for (int i = threadIdx.x; i < c * D; i += blockDim.x) {
        const int ci = i / D, d = i % D, k = ids[ci];
        const float s = dsum_outer(Q, (long)k * D + d, (long)K * D, [&](int q) { return (pt[q] == k ? 1.0f : 0.0f) * zt[(size_t)q * D + d]; });
        const float sz = sizes[ci];
        protos[((size_t)t * Cmax + ci) * D + d] = s / (sz < kEpsF ? kEpsF : sz);
    }
}

}  // namespace tclip

extern "C" {

int tclip_cluster_prototypes_visual(int32_t T, int32_t Q, int32_t K, int32_t dim, const float* x_q, const int32_t* preds,
                                    int32_t* n_clusters, int32_t* cluster_ids, float* prototypes, void* stream) {
    if (T < 1 || Q < 1 || K < 2 || K > 1024 || dim < 1 || !x_q || !preds || !n_clusters || !cluster_ids || !prototypes)
        return fail(TCLIP_ERR_ARG, "bad argument to tclip_cluster_prototypes_visual");
    if ((size_t)K * dim > 0x7fffffffu) return fail(TCLIP_ERR_ARG, "n_class * dim must fit in int32");
    const int Cmax = Q < K ? Q : K;
    hipLaunchKernelGGL(k_vis_prototypes, dim3(T), dim3(256), 0, (hipStream_t)stream, preds, x_q, Q, K, dim, Cmax, n_clusters,
                       cluster_ids, prototypes);
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

int tclip_visual_init(const float* visual, const float* text, int64_t n_rows, int32_t dim, int32_t n_class, float temperature,
                      float* out, void* stream) {
    if (!visual || !text || !out || n_rows < 0 || dim < 1 || n_class < 1) return fail(TCLIP_ERR_ARG, "bad argument to tclip_visual_init");
    if (n_rows == 0) return TCLIP_OK;
    const size_t lds = ((size_t)dim + (size_t)n_class) * sizeof(float);
    if (lds > 60000 || n_rows > 0x7fffffff) return fail(TCLIP_ERR_ARG, "dim + n_class must be <= 15000");
    hipLaunchKernelGGL(k_probability_features<true>, dim3((unsigned)n_rows), dim3(256), lds, (hipStream_t)stream, visual, text, dim,
                       n_class, temperature, front_end_vec(text, dim), out);
    TCLIP_HIP(hipGetLastError());
    return TCLIP_OK;
}

}  // extern "C"
