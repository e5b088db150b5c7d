// Local Collective Embeddings (polara/lib/optimize.py:309-391): the multiplicative updates of the three factors and the
// reductions of the objective.  All blocks are tall row-major fp64 with a leading dimension; the H factors are kept
// transposed ([labels x k], [users x k]), so all three updates are one form:
//     X <- X o (a N) / max(X M + (lambda + c_i) X, 1e-10),      M = ma M1 + mb M2  (k x k, symmetric)
// gfx950 only (wave = 64).
#include "pk_common.h"

#define LCE_FUSED_MAX_RANK 128      // M (k x k fp64) in LDS: 128 KiB at rank 128, plus 16 KiB of row staging, of 160 KiB per CU
#define LCE_THREADS 256
#define LCE_WAVES (LCE_THREADS / PK_WAVE)
#define LCE_RPT 4                   // rows per lane: one LDS read of M feeds four FMAs
#define LCE_FLOOR 1e-10             // the reference's np.maximum(., 1e-10)

// ---- fused multiplicative update -----------------------------------------------------------------------------------------
// CW: columns a row occupies in a wave (power of two >= k).  CW <= 64: a wave holds G = 64 / CW row groups, lane = (g, c);
// CW = 128: one group, a lane owns columns c and c + 64.  Every lane carries LCE_RPT rows, so a wave step covers
// G * LCE_RPT rows and a block step LCE_WAVES times that.  The rows of X of a wave step are staged in LDS transposed
// ([l][row of the step]): the product's inner loop reads M[l][c] (conflict-free along c) and four consecutive X values
// (the same address for all lanes of a group: a broadcast).  Summation over l ascending: a fixed order.
template <int CW>
__global__ __launch_bounds__(LCE_THREADS) void lce_update_kernel(int64_t m, int k, double *__restrict__ X, int64_t ldx,
                                                                 const double *__restrict__ N, int64_t ldn,
                                                                 const double *__restrict__ M1, int64_t ldm1, double ma,
                                                                 const double *__restrict__ M2, int64_t ldm2, double mb,
                                                                 double a, double lamb, const double *__restrict__ crow,
                                                                 int64_t n_steps) {
    constexpr int NC = CW > 64 ? CW / 64 : 1;
    constexpr int G = CW >= 64 ? 1 : 64 / CW;
    constexpr int GR = G * LCE_RPT;            // rows of a wave step
    extern __shared__ __attribute__((aligned(16))) double lce_smem[];
    double *sM = lce_smem;                     // [k][k]
    double *sX = lce_smem + ((k * k + 1) & ~1) + (threadIdx.x / PK_WAVE) * (k * GR);      // [k][GR] of this wave
    for (int e = threadIdx.x; e < k * k; e += LCE_THREADS) {
        const int l = e / k, j = e - l * k;
        double v = ma * M1[(int64_t)l * ldm1 + j];
        if (M2) v += mb * M2[(int64_t)l * ldm2 + j];
        sM[e] = v;
    }
    const int lane = pk_lane(), wave = threadIdx.x / PK_WAVE;
    const int c = CW >= 64 ? lane : lane % CW, g = CW >= 64 ? 0 : lane / CW;
    for (int64_t step = blockIdx.x; step < n_steps; step += gridDim.x) {
        const int64_t row0 = (step * LCE_WAVES + wave) * GR + g * LCE_RPT;
        double x[LCE_RPT][NC], nn[LCE_RPT][NC], acc[LCE_RPT][NC];
#pragma unroll
        for (int r = 0; r < LCE_RPT; ++r)
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const int col = c + 64 * q;
                const bool on = col < k && row0 + r < m;
                x[r][q] = on ? X[(row0 + r) * ldx + col] : 0.0;
                nn[r][q] = on ? N[(row0 + r) * ldn + col] : 0.0;
                acc[r][q] = 0.0;
            }
        __syncthreads();                        // M is in place (first step); the previous step's reads of sX are done
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int col = c + 64 * q;
            if (col < k) {
#pragma unroll
                for (int r = 0; r < LCE_RPT; ++r) sX[col * GR + g * LCE_RPT + r] = x[r][q];
            }
        }
        __syncthreads();
        int cc[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) cc[q] = min(c + 64 * q, k - 1);       // idle lanes read a valid column
        for (int l = 0; l < k; ++l) {
            double xv[LCE_RPT];
#pragma unroll
            for (int r = 0; r < LCE_RPT; ++r) xv[r] = sX[l * GR + g * LCE_RPT + r];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const double mv = sM[l * k + cc[q]];
#pragma unroll
                for (int r = 0; r < LCE_RPT; ++r) acc[r][q] = fma(xv[r], mv, acc[r][q]);
            }
        }
#pragma unroll
        for (int r = 0; r < LCE_RPT; ++r) {
            if (row0 + r >= m) continue;
            const double shift = lamb + (crow ? crow[row0 + r] : 0.0);
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const int col = c + 64 * q;
                if (col < k) {
                    const double den = fmax(acc[r][q] + shift * x[r][q], LCE_FLOOR);
                    X[(row0 + r) * ldx + col] = x[r][q] * ((a * nn[r][q]) / den);
                }
            }
        }
    }
}

// the element-wise half of the composed form (ranks above LCE_FUSED_MAX_RANK): P = X M comes from pk_tsmm_f64
__global__ __launch_bounds__(256) void lce_update_ew_kernel(int64_t m, int k, double *__restrict__ X, int64_t ldx,
                                                            const double *__restrict__ N, int64_t ldn,
                                                            const double *__restrict__ P, int64_t ldp, double a, double lamb,
                                                            const double *__restrict__ crow) {
    const int64_t total = m * k;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / k;
        const int col = (int)(e - row * k);
        const double x = X[row * ldx + col];
        const double shift = lamb + (crow ? crow[row] : 0.0);
        const double den = fmax(P[row * ldp + col] + shift * x, LCE_FLOOR);
        X[row * ldx + col] = x * ((a * N[row * ldn + col]) / den);
    }
}

extern "C" int32_t pk_lce_fused_max_rank(void) { return LCE_FUSED_MAX_RANK; }

extern "C" int pk_lce_update_f64(void *stream, int64_t m, int32_t k, double *X_dev, int64_t ldx, const double *N_dev, int64_t ldn,
                                 const double *M1_dev, int64_t ldm1, double ma, const double *M2_dev, int64_t ldm2, double mb,
                                 double a, double lamb, const double *c_dev) {
    PK_REQUIRE(m >= 1 && k >= 1 && k <= LCE_FUSED_MAX_RANK, "pk_lce_update_f64: rank %d outside 1..%d (compose pk_tsmm_f64 and pk_lce_update_ew_f64)",
               (int)k, LCE_FUSED_MAX_RANK);
    PK_REQUIRE(X_dev && N_dev && M1_dev && X_dev != N_dev, "pk_lce_update_f64: bad pointers");
    PK_REQUIRE(ldx >= k && ldn >= k && ldm1 >= k && (!M2_dev || ldm2 >= k), "pk_lce_update_f64: bad leading dimension");
    using kern_t = void (*)(int64_t, int, double *, int64_t, const double *, int64_t, const double *, int64_t, double, const double *,
                            int64_t, double, double, double, const double *, int64_t);
    const int cw = k <= 16 ? 16 : k <= 32 ? 32 : k <= 64 ? 64 : 128;
    kern_t kern = cw == 16 ? lce_update_kernel<16> : cw == 32 ? lce_update_kernel<32> : cw == 64 ? lce_update_kernel<64> : lce_update_kernel<128>;
    const int gr = (cw >= 64 ? 1 : 64 / cw) * LCE_RPT;
    const size_t lds = ((size_t)((k * k + 1) & ~1) + (size_t)LCE_WAVES * k * gr) * sizeof(double);
    const int64_t n_steps = pk_ceil_div(m, (int64_t)LCE_WAVES * gr);
    {   // per call: the attribute is per device and setting it is cheap (eigh.hip does the same)
        hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (LCE_FUSED_MAX_RANK * LCE_FUSED_MAX_RANK + LCE_WAVES * LCE_FUSED_MAX_RANK * LCE_RPT) * 8);
        if (e1 != hipSuccess) {
            pk_set_error("pk_lce_update_f64: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e1));
            return PK_E_LAUNCH;
        }
    }
    // workgroups a CU holds at this LDS size (at most 4: 16 waves), 256 CUs; a block keeps its copy of M across its steps
    const int per_cu = (int)(lds > 0 ? (160u * 1024u) / lds : 4);
    const int64_t cap = 256 * (int64_t)(per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu);
    const unsigned grid = (unsigned)(n_steps < cap ? n_steps : cap);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(LCE_THREADS), lds, pk_stream(stream), m, (int)k, X_dev, ldx, N_dev, ldn, M1_dev, ldm1,
                       ma, M2_dev, ldm2, mb, a, lamb, c_dev, n_steps);
    PK_CHECK_LAUNCH("lce_update_kernel");
    return PK_OK;
}

extern "C" int pk_lce_update_ew_f64(void *stream, int64_t m, int32_t k, double *X_dev, int64_t ldx, const double *N_dev, int64_t ldn,
                                    const double *P_dev, int64_t ldp, double a, double lamb, const double *c_dev) {
    PK_REQUIRE(m >= 1 && k >= 1 && X_dev && N_dev && P_dev && X_dev != N_dev && X_dev != P_dev, "pk_lce_update_ew_f64: bad arguments");
    PK_REQUIRE(ldx >= k && ldn >= k && ldp >= k, "pk_lce_update_ew_f64: bad leading dimension");
    const int64_t blocks = pk_ceil_div(m * k, 256);
    hipLaunchKernelGGL(lce_update_ew_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, pk_stream(stream), m, (int)k,
                       X_dev, ldx, N_dev, ldn, P_dev, ldp, a, lamb, c_dev);
    PK_CHECK_LAUNCH("lce_update_ew_kernel");
    return PK_OK;
}

// ---- reductions of the objective -----------------------------------------------------------------------------------------
// dot_p = sum_ij w_i P[i, j] Q[i, j] for up to PK_LCE_MAX_PAIRS blocks in one launch (Q == NULL: Q = 1; w == NULL: w = 1;
// the trace of a k x k matrix is the pair (its diagonal as a [k x 1] block of leading dimension ld + 1, NULL)).
// Fixed order, no atomics: pair p is cut into nb_p = pk_lce_dot_blocks(m_p * k_p) contiguous element ranges, a block sums
// its range with a fixed thread stride and a fixed LDS tree, the second kernel adds the nb_p partial sums in ascending
// order and forms   out[0] = bias + sum_p coef_p dot_p,   out[1 + p] = dot_p.
#define LCE_DOT_ELEMS 16384
#define LCE_DOT_MAX_BLOCKS 1024

struct LcePairs {
    const double *P[PK_LCE_MAX_PAIRS], *Q[PK_LCE_MAX_PAIRS], *w[PK_LCE_MAX_PAIRS];
    int64_t m[PK_LCE_MAX_PAIRS], ldp[PK_LCE_MAX_PAIRS], ldq[PK_LCE_MAX_PAIRS];
    int k[PK_LCE_MAX_PAIRS], first_block[PK_LCE_MAX_PAIRS + 1];
    double coef[PK_LCE_MAX_PAIRS];
    int n;
};

extern "C" int32_t pk_lce_dot_blocks(int64_t n_elems) {
    const int64_t b = pk_ceil_div(n_elems < 1 ? 1 : n_elems, LCE_DOT_ELEMS);
    return (int32_t)(b < LCE_DOT_MAX_BLOCKS ? b : LCE_DOT_MAX_BLOCKS);
}
extern "C" int64_t pk_lce_dots_work_bytes(void) { return (int64_t)PK_LCE_MAX_PAIRS * LCE_DOT_MAX_BLOCKS * 8; }

__device__ __forceinline__ double lce_block_sum(double v, double *s) {
    v = pk_wave_sum(v);
    if (pk_lane() == 0) s[threadIdx.x / PK_WAVE] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x / PK_WAVE); ++i) t += s[i];
    return t;      // valid in thread 0
}

__global__ __launch_bounds__(256) void lce_dots_kernel(LcePairs d, double *__restrict__ partial) {
    __shared__ double s[4];
    int p = 0;
    while (p + 1 < d.n && (int)blockIdx.x >= d.first_block[p + 1]) ++p;
    const int nb = d.first_block[p + 1] - d.first_block[p], b = blockIdx.x - d.first_block[p];
    const int64_t total = d.m[p] * d.k[p];
    const int64_t per = (total + nb - 1) / nb, e0 = per * b, e1 = e0 + per < total ? e0 + per : total;
    const double *P = d.P[p], *Q = d.Q[p], *w = d.w[p];
    const int k = d.k[p];
    double acc = 0.0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const int64_t row = e / k;
        const int col = (int)(e - row * k);
        double v = P[row * d.ldp[p] + col];
        if (Q) v *= Q[row * d.ldq[p] + col];
        if (w) v *= w[row];
        acc += v;
    }
    const double t = lce_block_sum(acc, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(64) void lce_dots_final_kernel(LcePairs d, const double *__restrict__ partial, double bias,
                                                            double *__restrict__ out) {
    if (threadIdx.x != 0) return;
    double obj = bias;
    for (int p = 0; p < d.n; ++p) {
        double t = 0.0;
        for (int b = d.first_block[p]; b < d.first_block[p + 1]; ++b) t += partial[b];
        out[1 + p] = t;
        obj += d.coef[p] * t;
    }
    out[0] = obj;
}

extern "C" int pk_lce_dots_f64(void *stream, int32_t n_pairs, const double *const *P_dev, const double *const *Q_dev,
                               const double *const *w_dev, const int64_t *m, const int32_t *k, const int64_t *ldp, const int64_t *ldq,
                               const double *coef, double bias, double *out_dev, void *work_dev) {
    PK_REQUIRE(n_pairs >= 1 && n_pairs <= PK_LCE_MAX_PAIRS && P_dev && Q_dev && w_dev && m && k && ldp && ldq && coef && out_dev && work_dev,
               "pk_lce_dots_f64: bad arguments (1..%d pairs)", PK_LCE_MAX_PAIRS);
    LcePairs d;
    d.n = n_pairs;
    d.first_block[0] = 0;
    for (int p = 0; p < n_pairs; ++p) {
        PK_REQUIRE(P_dev[p] && m[p] >= 1 && k[p] >= 1 && ldp[p] >= 1 && (!Q_dev[p] || ldq[p] >= 1), "pk_lce_dots_f64: bad pair %d", p);
        d.P[p] = P_dev[p];
        d.Q[p] = Q_dev[p];
        d.w[p] = w_dev[p];
        d.m[p] = m[p];
        d.k[p] = k[p];
        d.ldp[p] = ldp[p];
        d.ldq[p] = Q_dev[p] ? ldq[p] : 0;
        d.coef[p] = coef[p];
        d.first_block[p + 1] = d.first_block[p] + pk_lce_dot_blocks(m[p] * k[p]);
    }
    hipLaunchKernelGGL(lce_dots_kernel, dim3((unsigned)d.first_block[n_pairs]), dim3(256), 0, pk_stream(stream), d, (double *)work_dev);
    PK_CHECK_LAUNCH("lce_dots_kernel");
    hipLaunchKernelGGL(lce_dots_final_kernel, dim3(1), dim3(64), 0, pk_stream(stream), d, (const double *)work_dev, bias, out_dev);
    PK_CHECK_LAUNCH("lce_dots_final_kernel");
    return PK_OK;
}

// ---- E <- max(E, lo): the clamp of the cold-start queries (coldstart/models.py:144) ----------------------------------------
__global__ __launch_bounds__(256) void lce_clamp_kernel(int64_t m, int k, double *__restrict__ E, int64_t lde, double lo) {
    const int64_t total = m * k;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / k;
        const int col = (int)(e - row * k);
        const double v = E[row * lde + col];
        if (v < lo) E[row * lde + col] = lo;
    }
}

extern "C" int pk_clamp_min_f64(void *stream, int64_t m, int32_t k, double *E_dev, int64_t lde, double lo) {
    PK_REQUIRE(m >= 0 && k >= 1 && lde >= k && E_dev, "pk_clamp_min_f64: bad arguments");
    if (m == 0) return PK_OK;
    const int64_t blocks = pk_ceil_div(m * k, 256);
    hipLaunchKernelGGL(lce_clamp_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, pk_stream(stream), m, (int)k, E_dev,
                       lde, lo);
    PK_CHECK_LAUNCH("lce_clamp_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_lce() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&lce_clamp_kernel));
}
