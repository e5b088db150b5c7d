// Probabilistic matrix factorisation (polara/lib/optimize.py:123-154 as simple_pmf_sgd drives it): one SGD sweep over the
// interactions per epoch, on a conflict-free blocked schedule (polara_amd/pmf.py: block_schedule).  The blocks of one
// stratum share no user and no item: one launch sweeps them side by side, each block sequentially by one lane group, and the
// launches of an epoch follow each other in stream order.  The arithmetic of a sample is spelled out in polara_hip.h.
// gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "pmf_common.h"               // after the pragma: the shared helpers are compiled without contraction too

// W lanes per block, 64 / W blocks per wave.  The loop runs to the longest block of the wave with every lane active (the
// butterfly reads its neighbours); a group past the end of its block computes on zeros and stores nothing.  Sample t + 1's
// rows are loaded while sample t is computed — unless they are sample t's own rows, whose new values then stay in registers.
template <int W, int ADJ>
__global__ __launch_bounds__(PMF_THREADS) void pmf_stratum_kernel(PmfArgs a, int stratum) {
    constexpr int G = 64 / W;
    const int lane = pk_lane();
    const int g = lane / W, c = lane % W;
    const int64_t b = (int64_t)blockIdx.x * G + g;
    const bool col = c < a.rank;
    int64_t t0 = 0, len = 0;
    if (b < a.B) {
        t0 = a.block_ptr[(int64_t)stratum * a.B + b];
        len = a.block_ptr[(int64_t)stratum * a.B + b + 1] - t0;
    }
    int64_t maxlen = len;
#pragma unroll
    for (int off = 32; off >= W; off >>= 1) {
        const int64_t o = __shfl_xor(maxlen, off, 64);
        maxlen = o > maxlen ? o : maxlen;
    }
    maxlen = ((int64_t)__builtin_amdgcn_readfirstlane((int)(maxlen >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(maxlen & 0xffffffffll));

    auto sample = [&](int64_t t, int &m, int &n, double &v) {
        if (t < len) {
            m = a.users[t0 + t];
            n = a.items[t0 + t];
            v = a.vals[t0 + t];
        } else {
            m = -1;
            n = -1;
            v = 0.0;
        }
    };
    auto row = [&](const double *X, int64_t ld, int r) { return (r >= 0 && col) ? X[(int64_t)r * ld + c] : 0.0; };
    auto count = [&](const double *cnt, int r) { return r >= 0 ? cnt[r] : 1.0; };

    int m0, n0, m1, n1, m2, n2;
    double v0, v1, v2;
    sample(0, m0, n0, v0);
    sample(1, m1, n1, v1);
    double p = row(a.P, a.ldp, m0), q = row(a.Q, a.ldq, n0);
    double sp = ADJ ? row(a.SP, a.ldsp, m0) : 0.0, sq = ADJ ? row(a.SQ, a.ldsq, n0) : 0.0;
    double rc0 = count(a.rnnz, m0), cc0 = count(a.cnnz, n0);
    double sse = 0.0;
    for (int64_t t = 0; t < maxlen; ++t) {
        sample(t + 2, m2, n2, v2);
        const bool new_m = m1 != m0, new_n = n1 != n0;
        const double p_next = new_m ? row(a.P, a.ldp, m1) : 0.0, q_next = new_n ? row(a.Q, a.ldq, n1) : 0.0;
        const double sp_next = (ADJ && new_m) ? row(a.SP, a.ldsp, m1) : 0.0, sq_next = (ADJ && new_n) ? row(a.SQ, a.ldsq, n1) : 0.0;
        const double rc1 = count(a.rnnz, m1), cc1 = count(a.cnnz, n1);

        const double dot = pmf_group_sum<W>(p * q);
        const double err = v0 - dot;
        const double row_lambda = a.lambd / rc0, col_lambda = a.lambd / cc0;
        const double gp = err * q - p * row_lambda;
        const double gq = err * p - q * col_lambda;
        const double ap = pmf_adjust<ADJ>(gp, sp, a);
        const double p_new = p + a.eta * ap;
        const double aq = pmf_adjust<ADJ>(gq, sq, a);
        const double q_new = q + a.eta * aq;
        if (m0 >= 0) {
            if (col) {
                a.P[(int64_t)m0 * a.ldp + c] = p_new;
                a.Q[(int64_t)n0 * a.ldq + c] = q_new;
                if constexpr (ADJ != PK_PMF_ADJUST_NONE) {
                    a.SP[(int64_t)m0 * a.ldsp + c] = sp;
                    a.SQ[(int64_t)n0 * a.ldsq + c] = sq;
                }
            }
            sse = sse + err * err;
        }
        p = new_m ? p_next : p_new;
        q = new_n ? q_next : q_new;
        if constexpr (ADJ != PK_PMF_ADJUST_NONE) {
            sp = new_m ? sp_next : sp;
            sq = new_n ? sq_next : sq;
        }
        m0 = m1, n0 = n1, v0 = v1, rc0 = rc1, cc0 = cc1;
        m1 = m2, n1 = n2, v1 = v2;
    }
    if (b < a.B && c == 0) a.block_sse[(int64_t)stratum * a.B + b] = sse;
}

// block sums -> stratum sums (block order) -> the epoch's sum (stratum order)
__global__ __launch_bounds__(256) void pmf_sse_kernel(int B, const double *__restrict__ block_sse, double *__restrict__ out) {
    __shared__ double stratum_sse[PK_PMF_MAX_BLOCKS];
    for (int s = threadIdx.x; s < B; s += 256) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc = acc + block_sse[(int64_t)s * B + b];
        stratum_sse[s] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int s = 0; s < B; ++s) total = total + stratum_sse[s];
        out[0] = total;
    }
}

void pmf_launch_sse(hipStream_t st, int blocks, const double *block_sse_dev, double *sse_dev) {
    hipLaunchKernelGGL(pmf_sse_kernel, dim3(1), dim3(256), 0, st, blocks, block_sse_dev, sse_dev);
}

extern "C" int32_t pk_pmf_max_rank(void) { return PMF_MAX_RANK; }
extern "C" int64_t pk_pmf_work_doubles(int32_t blocks) { return (int64_t)(blocks < 1 ? 1 : blocks) * (blocks < 1 ? 1 : blocks); }

template <int W>
static void pmf_launch(hipStream_t st, int adjust, unsigned grid, const PmfArgs &a, int stratum) {
    if (adjust == PK_PMF_ADJUST_NONE)
        hipLaunchKernelGGL((pmf_stratum_kernel<W, PK_PMF_ADJUST_NONE>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else if (adjust == PK_PMF_ADJUST_ADAGRAD)
        hipLaunchKernelGGL((pmf_stratum_kernel<W, PK_PMF_ADJUST_ADAGRAD>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else
        hipLaunchKernelGGL((pmf_stratum_kernel<W, PK_PMF_ADJUST_RMSPROP>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
}

extern "C" int pk_pmf_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, const int64_t *block_ptr_dev,
                                const int32_t *users_dev, const int32_t *items_dev, const double *vals_dev, double *P_dev, int64_t ldp,
                                double *Q_dev, int64_t ldq, const double *row_nnz_dev, const double *col_nnz_dev, double eta,
                                double lambd, int32_t adjust, double *SP_dev, int64_t ldsp, double *SQ_dev, int64_t ldsq, double gamma,
                                double smoothing, double *work_dev, double *sse_dev) {
    PK_REQUIRE(rank >= 1 && rank <= PMF_MAX_RANK, "pk_pmf_epoch_f64: rank %d outside 1..%d", (int)rank, PMF_MAX_RANK);
    PK_REQUIRE(blocks >= 1 && blocks <= PK_PMF_MAX_BLOCKS, "pk_pmf_epoch_f64: %d blocks outside 1..%d", (int)blocks, PK_PMF_MAX_BLOCKS);
    PK_REQUIRE(nnz >= 0 && block_ptr_dev && P_dev && Q_dev && row_nnz_dev && col_nnz_dev && work_dev && sse_dev && P_dev != Q_dev,
               "pk_pmf_epoch_f64: bad pointers");
    PK_REQUIRE(nnz == 0 || (users_dev && items_dev && vals_dev), "pk_pmf_epoch_f64: no interactions given");
    PK_REQUIRE(ldp >= rank && ldq >= rank, "pk_pmf_epoch_f64: bad leading dimension");
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || adjust == PK_PMF_ADJUST_ADAGRAD || adjust == PK_PMF_ADJUST_RMSPROP,
               "pk_pmf_epoch_f64: unknown gradient adjustment %d", (int)adjust);
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || (SP_dev && SQ_dev && SP_dev != SQ_dev && ldsp >= rank && ldsq >= rank),
               "pk_pmf_epoch_f64: the gradient adjustment needs its two state blocks");
    PmfArgs a;
    a.B = blocks, a.rank = rank;
    a.block_ptr = block_ptr_dev, a.users = users_dev, a.items = items_dev, a.vals = vals_dev;
    a.P = P_dev, a.Q = Q_dev, a.ldp = ldp, a.ldq = ldq;
    a.rnnz = row_nnz_dev, a.cnnz = col_nnz_dev;
    a.eta = eta, a.lambd = lambd;
    a.SP = SP_dev, a.SQ = SQ_dev, a.ldsp = ldsp, a.ldsq = ldsq;
    a.gamma = gamma, a.one_minus_gamma = 1.0 - gamma, a.smoothing = smoothing;
    a.block_sse = work_dev;
    const int w = rank <= 16 ? 16 : rank <= 32 ? 32 : 64;
    const unsigned grid = (unsigned)pk_ceil_div(blocks, 64 / w);
    hipStream_t st = pk_stream(stream);
    for (int s = 0; s < blocks; ++s) {
        if (w == 16)
            pmf_launch<16>(st, adjust, grid, a, s);
        else if (w == 32)
            pmf_launch<32>(st, adjust, grid, a, s);
        else
            pmf_launch<64>(st, adjust, grid, a, s);
        PK_CHECK_LAUNCH("pmf_stratum_kernel");
    }
    pmf_launch_sse(st, (int)blocks, work_dev, sse_dev);
    PK_CHECK_LAUNCH("pmf_sse_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_pmf() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&pmf_sse_kernel));
}
