// Logistic matrix factorisation (Johnson 2014, in the shape the `implicit` package trains it: rank k plus a bias on either side,
// per-parameter AdaGrad): one half-step.  Y [n_cols x K] fixed (K = k + 2), C a CSR of confidences; every row u with n > 0 stored
// entries takes one full-batch AdaGrad step on its row of X against its n positives and m = min(n_cols, n * neg_prop) negatives
// drawn inside the kernel from a counter (no sample array exists).  The arithmetic of a row, the draw stream and the sigmoid are
// spelled out in include/polara_hip.h (and derived in DESIGN.md); this file follows that order literally.
// One workgroup of LMF_THREADS threads per row; rows are taken in the caller's order (longest first).  K is padded to KP = 16 NT
// (zeros) and the kernel is instantiated per NT = 1..8:
//   * the row's sample list — positives in storage order, then negatives in draw order — is staged through LDS in chunks of CH
//     gathered rows of Y: the next chunk is fetched into registers while the current one is reduced, and the column ids of the
//     chunk after next (stored ids or draws) are computed meanwhile by one thread per sample into a two-deep index ring;
//   * a chunk's logits: one lane per sample (a lane group of one: the sum over the columns is serial by specification, so a
//     wider group would only idle), the staging rows have an odd leading dimension so that the lanes fall into different banks;
//   * the gradient: one thread per (column, chain); chain j holds the samples q = j mod PK_LMF_CHAINS of the whole list, summed
//     left to right in registers across the chunks, then the chains of a column are added in chain order.  The order of summation
//     is a function of the row alone — not of the grid, the row order, the chunk length or the workgroup;
//   * the AdaGrad update of the row by one thread per column; the pinned column and its state are not touched.
// No atomics, no floating-point reduction across workgroups, nothing is written beside the rows.  gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "blocked_sweep.h"            // pair_stream_key: the key of a round's draw stream
#include "pk_sigmoid.h"

#define LMF_MAX_K 128
#ifndef LMF_THREADS
#define LMF_THREADS 256             // 64: one wave per row (the rejected mapping; built only for measurements)
#endif
#define LMF_DRAW_THREADS 256

template <int NT>
struct LmfShape {
    static constexpr int KP = 16 * NT;                                         // padded K
    // samples of a staging chunk: the largest of 64, 32, 16, 8 that keeps at most 16 doubles per thread in flight
    static constexpr int CH = 64 * KP <= 16 * LMF_THREADS ? 64 : 32 * KP <= 16 * LMF_THREADS ? 32 : 16 * KP <= 16 * LMF_THREADS ? 16 : 8;
    static constexpr int EPT = CH * KP / LMF_THREADS;                          // staged doubles per thread
    static constexpr int LD = KP + 1;                                          // odd: the logits' lanes read different banks
    static constexpr int PAIRS = KP * PK_LMF_CHAINS;                           // (column, chain) pairs
    static constexpr int PPT = (PAIRS + LMF_THREADS - 1) / LMF_THREADS;        // pairs per thread
    static_assert(CH * KP % LMF_THREADS == 0, "staging does not divide among the threads");
    static_assert(CH <= LMF_THREADS, "the logits need a lane per sample");
    static_assert(CH % PK_LMF_CHAINS == 0, "a chunk must hold whole turns of the chains");
    static_assert((CH * LD + 2 * CH + KP + PAIRS) * 8 + 2 * CH * 4 <= 64 * 1024, "static LDS budget");
};

// negative t of a row whose draws start at counter `base` = key + neg_ptr[row]: uniform over all columns
__device__ __forceinline__ int32_t lmf_draw(uint64_t base, int64_t t, int64_t n_cols) {
    return (int32_t)(((pk_mix64(base + (uint64_t)t) >> 32) * (uint64_t)n_cols) >> 32);
}

__device__ __forceinline__ int64_t lmf_negatives(int64_t n, int64_t neg_prop, int64_t n_cols) {
    const int64_t m = n * neg_prop;
    return m < n_cols ? m : n_cols;
}

template <int NT>
__global__ __launch_bounds__(LMF_THREADS) void lmf_half_step_kernel(int64_t n_rows, int64_t n_cols, int K,
                                                                    const int64_t *__restrict__ indptr,
                                                                    const int32_t *__restrict__ indices,
                                                                    const double *__restrict__ conf,
                                                                    const int32_t *__restrict__ row_order,
                                                                    const int64_t *__restrict__ neg_ptr, uint64_t key, int pinned,
                                                                    int64_t neg_prop, const double *__restrict__ Y, int64_t ldy,
                                                                    double lr, double reg, double *__restrict__ X, int64_t ldx,
                                                                    double *__restrict__ A, int64_t lda) {
    using S = LmfShape<NT>;
    constexpr int KP = S::KP, CH = S::CH, EPT = S::EPT, LD = S::LD, PAIRS = S::PAIRS, PPT = S::PPT;
    __shared__ double sY[CH * LD];              // the gathered rows of Y of one chunk
    __shared__ double sC[CH];                   // the confidences of the chunk's positives
    __shared__ double sG[CH];                   // the sample weights g
    __shared__ double sX[KP];                   // x_u as it was before the step
    __shared__ double sD[PAIRS];                // [PK_LMF_CHAINS][KP]: the chains' sums
    __shared__ int32_t sIdx[2][CH];             // column ids: of the chunk being fetched and of the one after it
    const int tid = threadIdx.x;
    const int64_t row = row_order ? (int64_t)row_order[blockIdx.x] : (int64_t)blockIdx.x;
    if (row < 0 || row >= n_rows) return;       // not a row: nothing is written (the caller's order is a permutation)
    const int64_t beg = indptr[row], n = indptr[row + 1] - beg;
    if (n <= 0) return;                         // an empty row is not touched at all
    const int64_t total = n + lmf_negatives(n, neg_prop, n_cols);
    const uint64_t base = key + (uint64_t)neg_ptr[row];
    double *xrow = X + row * ldx, *arow = A + row * lda;
    for (int c = tid; c < KP; c += LMF_THREADS) sX[c] = c < K ? xrow[c] : 0.0;

    // column of sample q of the list (positives in storage order, then negatives in draw order); -1 past its end
    auto column = [&](int64_t q) -> int32_t { return q < n ? indices[beg + q] : q < total ? lmf_draw(base, q - n, n_cols) : -1; };
    if (tid < CH) {
        sIdx[0][tid] = column(tid);
        sIdx[1][tid] = column(CH + tid);
    }
    __syncthreads();
    double ry[EPT], rc = 0.0;
    auto fetch = [&](int64_t q0, int buf) {
#pragma unroll
        for (int r = 0; r < EPT; ++r) {
            const int e = tid + LMF_THREADS * r, q = e / KP, j = e - q * KP;
            const int32_t idx = sIdx[buf][q];
            ry[r] = (j < K && idx >= 0 && idx < n_cols) ? Y[(int64_t)idx * ldy + j] : 0.0;
        }
        rc = (tid < CH && q0 + tid < n) ? conf[beg + q0 + tid] : 0.0;
    };
    double acc[PPT];
#pragma unroll
    for (int r = 0; r < PPT; ++r) acc[r] = 0.0;
    int buf = 0;
    fetch(0, 0);
    for (int64_t q0 = 0; q0 < total; q0 += CH, buf ^= 1) {
        __syncthreads();                        // the chains of the previous chunk have read sY and sG
#pragma unroll
        for (int r = 0; r < EPT; ++r) {
            const int e = tid + LMF_THREADS * r, q = e / KP;
            sY[q * LD + (e - q * KP)] = ry[r];
        }
        if (tid < CH) sC[tid] = rc;
        __syncthreads();
        if (q0 + CH < total) fetch(q0 + CH, buf ^ 1);          // in flight during the reduction below
        if (tid < CH) sIdx[buf][tid] = column(q0 + 2 * CH + tid);      // every fetch of the chunk that was there has landed in sY
        const int nq = (int)(total - q0 < CH ? total - q0 : CH);
        if (tid < nq) {                         // the logits, the columns left to right
            const double *yr = sY + tid * LD;
            double s = sX[0] * yr[0];
            for (int c = 1; c < K; ++c) s = s + sX[c] * yr[c];
            sG[tid] = q0 + tid < n ? sC[tid] * pk_sigmoid(s) : -pk_sigmoid(-s);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PPT; ++r) {         // the chains: (q0 is a multiple of PK_LMF_CHAINS)
            const int p = tid + LMF_THREADS * r;
            if (p < PAIRS) {
                const int j = p / KP, c = p - j * KP;
                for (int q = j; q < nq; q += PK_LMF_CHAINS) acc[r] = acc[r] + sG[q] * sY[q * LD + c];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int p = tid + LMF_THREADS * r;
        if (p < PAIRS) sD[p] = acc[r];
    }
    __syncthreads();
    for (int c = tid; c < K; c += LMF_THREADS) {
        if (c == pinned) continue;
        double D = sD[c];
#pragma unroll
        for (int j = 1; j < PK_LMF_CHAINS; ++j) D = D + sD[j * KP + c];
        const double x = sX[c];
        const double d = D - reg * x;
        const double a = arow[c] + d * d;
        arow[c] = a;
        xrow[c] = x + (lr / sqrt(1e-6 + a)) * d;
    }
}

// the draws of a half-step on their own, through lmf_draw: out[neg_ptr[row] + t]
__global__ __launch_bounds__(LMF_DRAW_THREADS) void lmf_draw_kernel(int64_t n_rows, int64_t n_cols, const int64_t *__restrict__ indptr,
                                                                    const int64_t *__restrict__ neg_ptr, int64_t neg_prop,
                                                                    uint64_t key, int32_t *__restrict__ out) {
    const int64_t row = blockIdx.x;
    if (row >= n_rows) return;
    const int64_t m = lmf_negatives(indptr[row + 1] - indptr[row], neg_prop, n_cols), at = neg_ptr[row];
    if (m != neg_ptr[row + 1] - at) return;     // not this plan's matrix: nothing is written
    const uint64_t base = key + (uint64_t)at;
    for (int64_t t = threadIdx.x; t < m; t += LMF_DRAW_THREADS) out[at + t] = lmf_draw(base, t, n_cols);
}

extern "C" int32_t pk_lmf_max_rank(void) { return LMF_MAX_K - 2; }
extern "C" int32_t pk_lmf_chains(void) { return PK_LMF_CHAINS; }

template <int NT>
static int lmf_launch(hipStream_t stream, int64_t n_rows, int64_t n_cols, int K, const int64_t *indptr, const int32_t *indices,
                      const double *conf, const int32_t *row_order, const int64_t *neg_ptr, uint64_t key, int pinned, int64_t neg_prop,
                      const double *Y, int64_t ldy, double lr, double reg, double *X, int64_t ldx, double *A, int64_t lda) {
    hipLaunchKernelGGL(lmf_half_step_kernel<NT>, dim3((unsigned)n_rows), dim3(LMF_THREADS), 0, stream, n_rows, n_cols, K, indptr, indices,
                       conf, row_order, neg_ptr, key, pinned, neg_prop, Y, ldy, lr, reg, X, ldx, A, lda);
    PK_CHECK_LAUNCH("lmf_half_step_kernel");
    return PK_OK;
}

static int lmf_check_sizes(const char *entry, int64_t n_rows, int64_t n_cols, int32_t neg_prop) {
    PK_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && n_cols >= 1 && n_cols < (1ll << 31), "%s: %lld rows, %lld columns (32-bit ids)",
               entry, (long long)n_rows, (long long)n_cols);
    PK_REQUIRE(neg_prop >= 1, "%s: neg_prop %d < 1", entry, (int)neg_prop);
    return PK_OK;
}

extern "C" int pk_lmf_half_step_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t K, const int64_t *indptr_dev,
                                    const int32_t *indices_dev, const double *conf_dev, const int32_t *row_order_dev,
                                    const int64_t *neg_ptr_dev, uint32_t seed, uint32_t round, int32_t pinned_col, int32_t neg_prop,
                                    const double *Y_dev, int64_t ldy, double learning_rate, double regularization, double *X_dev,
                                    int64_t ldx, double *A_dev, int64_t lda) {
    PK_REQUIRE(K >= 1 && K <= LMF_MAX_K, "pk_lmf_half_step_f64: %d columns outside 1..%d (rank + 2)", (int)K, LMF_MAX_K);
    const int rc = lmf_check_sizes("pk_lmf_half_step_f64", n_rows, n_cols, neg_prop);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(pinned_col >= -1 && pinned_col < K, "pk_lmf_half_step_f64: pinned column %d outside -1..%d", (int)pinned_col, (int)K - 1);
    PK_REQUIRE(indptr_dev && neg_ptr_dev && Y_dev && X_dev && A_dev && X_dev != Y_dev && A_dev != Y_dev && A_dev != X_dev,
               "pk_lmf_half_step_f64: bad pointers");
    PK_REQUIRE(ldy >= K && ldx >= K && lda >= K, "pk_lmf_half_step_f64: bad leading dimension");
    if (n_rows == 0) return PK_OK;
    PK_REQUIRE(indices_dev && conf_dev, "pk_lmf_half_step_f64: bad pointers");
    hipStream_t st = pk_stream(stream);
    const uint64_t key = pair_stream_key(seed, round);
    int out = PK_OK;
#define LMF_CASE(NT)                                                                                                                \
    case NT:                                                                                                                        \
        out = lmf_launch<NT>(st, n_rows, n_cols, K, indptr_dev, indices_dev, conf_dev, row_order_dev, neg_ptr_dev, key, pinned_col, \
                             neg_prop, Y_dev, ldy, learning_rate, regularization, X_dev, ldx, A_dev, lda);                          \
        break;
    switch ((K + 15) / 16) { LMF_CASE(1) LMF_CASE(2) LMF_CASE(3) LMF_CASE(4) LMF_CASE(5) LMF_CASE(6) LMF_CASE(7) LMF_CASE(8) }
#undef LMF_CASE
    return out;
}

extern "C" int pk_lmf_draw_negatives(void *stream, int64_t n_rows, int64_t n_cols, const int64_t *indptr_dev,
                                     const int64_t *neg_ptr_dev, int32_t neg_prop, uint32_t seed, uint32_t round, int32_t *out_dev) {
    const int rc = lmf_check_sizes("pk_lmf_draw_negatives", n_rows, n_cols, neg_prop);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(indptr_dev && neg_ptr_dev && out_dev, "pk_lmf_draw_negatives: bad pointers");
    if (n_rows == 0) return PK_OK;
    hipLaunchKernelGGL(lmf_draw_kernel, dim3((unsigned)n_rows), dim3(LMF_DRAW_THREADS), 0, pk_stream(stream), n_rows, n_cols, indptr_dev,
                       neg_ptr_dev, (int64_t)neg_prop, pair_stream_key(seed, round), out_dev);
    PK_CHECK_LAUNCH("lmf_draw_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_lmf() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&lmf_draw_kernel));
}
