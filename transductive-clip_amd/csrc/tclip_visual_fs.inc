// The support class sums of few-shot PADDLE and BD-CSPN on VISUAL features (the reference's use_softmax_feature == False;
// src/methods/few_shot/paddle.py:94-219, bdcspn.py:42-200): included at the end of tclip_kernels.hip after tclip_visual.inc,
// uses the library's helpers (SparseCascade, outer_column_is_cascade).
//
// The op sequences are paddle_loop / bdcspn_pass of tclip_methods.inc for both feature kinds; here a feature row has D elements,
// D independent of the class count K: prototypes and centroids are [T, K, D], support rows [T, S, D], query rows [T, Q, D],
// the responsibilities stay [T, Q, K].  Only the support class sums need a kernel of their own; the centroid statistics are
// k_vis_mstats's few-shot modes (tclip_visual.inc).

namespace tclip {

// ---- support class sums ------------------------------------------------------------------------------------------------
// sup[t,k,d] = sum_s 1[y_s = k] x_s[t,s,d] in the order of torch's (support.unsqueeze(2) * y_s_one_hot.unsqueeze(3)).sum(1): an
// outer sum over S rows of K*D contiguous columns, so the cascade levels follow S and the last K*D mod 32 columns take the
// 4-way row sum.  cnt[t,k] = the number of members (y_s_one_hot.sum(1): a sum of zeros and ones, exact in any order).
// One block per (class, task): the members of the class are compacted in order into LDS and only they are visited; the dumps
// that fall between two members are replayed (SparseCascade), since the zero products of the other rows only matter through
// the positions of the dumps.  A label outside 0..K-1 matches no block and is never used as an index.
// The rows come from a RowSrc without a column permutation (the reference permutes no columns on visual features): row s of
// task t is xs.base[t, s, :] of a dense [T, S, D] tensor, or xs.base[xs.idx[t S + s], :] of a feature table read in place
// (tclip_paddle_visual_run_tasks); the order of the additions is the same.
__global__ __launch_bounds__(256) void k_vis_support_stats(RowSrc xs, const int64_t* __restrict__ ys, int S, int K,
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
    const float* xt = xs.base + (xs.idx ? 0 : (size_t)t * S * D);
    const int64_t* it = xs.idx ? xs.idx + (size_t)t * S : nullptr;
    auto row = [&](int s_) { return xt + (size_t)(it ? it[s_] : (int64_t)s_) * D; };
    const long ncols = (long)K * D;
    const int size_ilp = S >> 2;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const long col = (long)k * D + d;
        float r;
        if (outer_column_is_cascade(col, ncols)) {
            SparseCascade c(S);
            for (int i = 0; i < nm; i++) c.add(vis_members[i], row(vis_members[i])[d]);
            r = c.finish();
        } else {   // 4 interleaved cascades over s/4; the leftovers (s >= 4*(S/4)) join partial 0 after its cascade is complete
            SparseCascade c0(size_ilp), c1(size_ilp), c2(size_ilp), c3(size_ilp);
            bool has_extra = false;
            float p0 = 0.f;
            for (int i = 0; i < nm; i++) {
                const int s = vis_members[i];
                const float v = row(s)[d];
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

static void launch_vis_support_stats(hipStream_t st, const RowSrc& xs, const int64_t* ys, int T, int S, int K, int D, float* sup,
                                     float* cnt) {
    hipLaunchKernelGGL(k_vis_support_stats, dim3(K, T), dim3(256), (size_t)S * sizeof(int), st, xs, ys, S, K, D, sup, cnt);
}

// a dense [T, S, D] tensor (ALPHA_TIM, TIM_GD, LaplacianShot, BD-CSPN)
static void launch_vis_support_stats(hipStream_t st, const float* xs, const int64_t* ys, int T, int S, int K, int D, float* sup,
                                     float* cnt) {
    launch_vis_support_stats(st, dense_rows(xs), ys, T, S, K, D, sup, cnt);
}

}  // namespace tclip
