// iALS++ (Rendle, Krichene, Zhang, Koren 2021): the block-subspace step of implicit ALS, and the cached predictions it works on.
//
// Block step.  Y [n_cols x k] fixed, C a CSR of confidences, G = Y^T Y, e_i = x_u . y_i cached for the stored entries of row u,
// pi = [p0, p0 + dw) a block of dw <= d = 16 NT coordinates (NT = 1, 2, 4); for every row u
//     g = G[pi,:] x_u + lambda_u x_pi + sum_i ((c_i - 1) e_i - c_i) y_{i,pi}
//     H = G[pi,pi] + lambda_u I + sum_i (c_i - 1) y_{i,pi} y_{i,pi}^T
//     delta = H^-1 g;   x_pi -= delta;   e_i -= y_{i,pi} . delta
// — the exact minimiser of the objective over x_pi.  G[pi,:] x_u comes in as R [n_rows x dw] (the host forms X G[:,pi] before
// the launch).  The structure is that of ials_half_step_kernel (ials.hip) with the block in place of the rank: one workgroup
// (4 waves) per row for every NT, rows in the caller's order (longest first), the block padded to KP = 16 NT with zeros:
//   * the row's entries are staged through LDS in chunks of CH = 32 gathered slices Y[i, p0 : p0 + dw] (128 NT contiguous
//     bytes each; the next chunk is in registers while the current one is multiplied);
//   * sum (c - 1) y_pi y_pi^T runs on v_mfma_f64_16x16x4_f64 over the lower-triangular 16 x 16 tiles only, four entries per
//     instruction in storage order, the accumulators started from G[pi,pi] + lambda_u I;
//   * g is summed by one thread per column, entry after entry in storage order, started from r_u + lambda_u x_pi;
//   * the tiles go to LDS ([KP + 1] x [KP + 1] doubles, odd leading dimension), g below them as row dw: the right-looking
//     Cholesky of the dw + 1 rows leaves L^-1 g there, a back substitution gives delta, and the thread of column j writes
//     x_pi[j] -= delta[j];
//   * a second pass over the row's entries writes e_i -= y_{i,pi} . delta: 16 lanes per entry (one 128-byte line per NT), a
//     lane's columns j = l, l + 16, .. added in ascending order, then a butterfly over the 16 lanes;
//   * a pivot that is not > 0 (NaN included) ends the row: x_pi and e are left untouched and flag[u] = 1.  A second, one-block
//     kernel counts the flags and finds the first.
// Every order of summation is a function of the row alone: no atomics, no floating-point reduction across workgroups.
// Lane mapping: one workgroup per row for every NT — at NT = 1 a single tile leaves three waves without matrix work, but they
// share the gather, the sum of g, the trailing update and the second pass; a one-wave-per-row instance was not built.
// LDS / VGPRs (no scratch, no spill in any instance): 52 240 bytes / 130 at NT = 4 (three workgroups per CU), 18 640 / 90 at
// NT = 2, 7 216 / 80 at NT = 1; the prediction kernel uses 26 / 40 / 88 VGPRs at 2 / 8 / 32 columns per lane and no LDS.
//
// Predictions.  e[p] = x_u . y_i for every stored entry p = (u, i), one wave per row and segment (every eighth entry of the row:
// the items' rows are long and few): a lane holds columns lane + 64 t of x_u, multiplies them in ascending t, and the wave adds
// the 64 partial sums by a butterfly (the same bits in every lane).  An entry is a sum of its own, so the segments change no bit.
// gfx950 only (wave = 64).
#include "pk_common.h"

#define IALSPP_MAX_RANK 2048
#define IALSPP_THREADS 256
#define IALSPP_REDUCE_THREADS 1024
#define IALSPP_PREDICT_SEGMENTS 8    // waves per row of the prediction kernel: entry p of a row belongs to segment p mod 8

typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int NT>
struct IalsppShape {
    static constexpr int KP = 16 * NT;                         // padded block width
    static constexpr int CH = 32;                              // entries of a staging chunk
    static constexpr int EPT = CH * KP / IALSPP_THREADS;       // staged doubles per thread: 2, 4, 8
    static constexpr int NTILES = NT * (NT + 1) / 2;           // lower-triangular tiles: 1, 3, 10
    static constexpr int TPW = (NTILES + 3) / 4;               // tiles per wave: 1, 1, 3
    static constexpr int LDA = KP + 1;                         // odd: a column of H falls into different banks
    static constexpr int TPR = NT == 1 ? 16 : NT == 2 ? 8 : 4; // threads per row in the trailing update
    static constexpr int A_ELEMS = (KP + 1) * LDA;
    static constexpr int LDS_DOUBLES = A_ELEMS + CH * KP + 2 * CH + (KP + 1) + 2 * KP;
    static_assert(NT == 1 || NT == 2 || NT == 4, "block widths 16, 32, 64");
    static_assert(CH * KP % IALSPP_THREADS == 0, "staging does not divide among the threads");
    static_assert(IALSPP_THREADS / TPR >= KP, "the trailing update needs a thread group per row 1 .. KP");
    static_assert(3 * LDS_DOUBLES * 8 <= 160 * 1024, "three workgroups per CU");
};

template <int NT>
__global__ __launch_bounds__(IALSPP_THREADS) void ialspp_block_step_kernel(
    int64_t n_rows, int64_t n_cols, int p0, int dw, const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    const double *__restrict__ conf, const int32_t *__restrict__ row_order, const double *__restrict__ Y, int64_t ldy,
    const double *__restrict__ G, int64_t ldg, double lambda, const double *__restrict__ lambda_rows, const double *__restrict__ R,
    int64_t ldr, double *__restrict__ X, int64_t ldx, double *__restrict__ E, int32_t *__restrict__ flags) {
    using S = IalsppShape<NT>;
    constexpr int KP = S::KP, CH = S::CH, EPT = S::EPT, TPW = S::TPW, LDA = S::LDA, TPR = S::TPR;
    extern __shared__ __attribute__((aligned(16))) double ialspp_smem[];
    double *sA = ialspp_smem;                   // [KP + 1][LDA]: the lower triangle of H, g in row dw
    double *sY = sA + S::A_ELEMS;               // [CH][KP]: the gathered slices of one chunk
    double *sW = sY + CH * KP;                  // [CH]: c - 1
    double *sC = sW + CH;                       // [CH]: (c - 1) e - c
    double *sCol = sC + CH;                     // [KP + 1]: the scaled column of the current Cholesky step
    double *sDiag = sCol + KP + 1;              // [KP]: the diagonal of L
    double *sDelta = sDiag + KP;                // [KP]: delta (zeros past dw)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row = row_order ? (int64_t)row_order[blockIdx.x] : (int64_t)blockIdx.x;
    if (row < 0 || row >= n_rows) return;       // not a row: nothing is written (the caller's order is a permutation)
    const int64_t beg = indptr[row], n = indptr[row + 1] - beg;
    double *xblk = X + row * ldx + p0;
    if (n <= 0) {                               // an empty row: x_pi = 0 exactly
        if (tid < dw) xblk[tid] = 0.0;
        if (tid == 0) flags[row] = 0;
        return;
    }
    const double lam = lambda_rows ? lambda_rows[row] : lambda;
    // ---- the tiles of this wave, their accumulators started from G[pi,pi] + lambda I --------------------------------------
    int ti[TPW], tj[TPW];
    bool on[TPW];
    f64x4 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int t = wave + 4 * j;
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= t) ++a;
        ti[j] = a;
        tj[j] = t - a * (a + 1) / 2;
        on[j] = t < S::NTILES;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = 16 * ti[j] + (lane >> 4) + 4 * r, gj = 16 * tj[j] + (lane & 15);
            double v = 0.0;
            if (on[j] && gi < dw && gj < dw) {
                v = G[(int64_t)(p0 + gi) * ldg + p0 + gj];
                if (gi == gj) v += lam;
            }
            acc[j][r] = v;
        }
    }
    // ---- the chunks -------------------------------------------------------------------------------------------------------
    double ry[EPT], rc = 0.0, re = 0.0;
    auto fetch = [&](int64_t q0) {
#pragma unroll
        for (int r = 0; r < EPT; ++r) {
            const int e = tid + IALSPP_THREADS * r, q = e / KP, j = e - q * KP;
            double v = 0.0;
            if (q0 + q < n && j < dw) {
                const int32_t idx = indices[beg + q0 + q];
                if (idx >= 0 && idx < n_cols) v = Y[(int64_t)idx * ldy + p0 + j];
            }
            ry[r] = v;
        }
        const bool in = tid < CH && q0 + tid < n;
        rc = in ? conf[beg + q0 + tid] : 0.0;
        re = in ? E[beg + q0 + tid] : 0.0;
    };
    double gacc = tid < dw ? fma(lam, xblk[tid], R[row * ldr + tid]) : 0.0;
    fetch(0);
    for (int64_t q0 = 0; q0 < n; q0 += CH) {
        __syncthreads();                        // the products of the previous chunk have read sY
#pragma unroll
        for (int r = 0; r < EPT; ++r) sY[tid + IALSPP_THREADS * r] = ry[r];
        if (tid < CH) {
            const bool in = q0 + tid < n;
            sW[tid] = in ? rc - 1.0 : 0.0;
            sC[tid] = in ? fma(rc - 1.0, re, -rc) : 0.0;
        }
        __syncthreads();
        if (q0 + CH < n) fetch(q0 + CH);        // in flight during the products below
        const int nq = (int)(n - q0 < CH ? n - q0 : CH);
        for (int qq = 0; qq < nq; qq += 4) {    // groups of four; the entries past nq are zeros
            const int q = qq + (lane >> 4);
            const double w = sW[q];
            const double *yr = sY + q * KP + (lane & 15);
#pragma unroll
            for (int j = 0; j < TPW; ++j)
                if (on[j]) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(w * yr[16 * ti[j]], yr[16 * tj[j]], acc[j], 0, 0, 0);
        }
        if (tid < KP)
            for (int q = 0; q < nq; ++q) gacc = fma(sC[q], sY[q * KP + tid], gacc);
    }
    // ---- H (lower tiles) and g to LDS -------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < TPW; ++j)
        if (on[j]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sA[(16 * ti[j] + (lane >> 4) + 4 * r) * LDA + 16 * tj[j] + (lane & 15)] = acc[j][r];
        }
    __syncthreads();
    if (tid < dw) sA[dw * LDA + tid] = gacc;
    // ---- right-looking Cholesky of rows 0 .. dw (row dw = g: it becomes z = L^-1 g) ----------------------------------------
    bool ok = true;
    for (int j = 0; j < dw; ++j) {
        __syncthreads();
        const double d = sA[j * LDA + j];
        if (!(d > 0.0)) {                       // the same value in every thread: the whole workgroup leaves
            ok = false;
            break;
        }
        const double s = sqrt(d);
        if (tid > j && tid <= dw) {
            const double l = sA[tid * LDA + j] / s;
            sA[tid * LDA + j] = l;
            sCol[tid] = l;
        }
        if (tid == j) sDiag[j] = s;
        __syncthreads();
        const int i = 1 + tid / TPR;
        if (i > j && i <= dw) {
            const double li = sCol[i];
            const int cmax = i < dw ? i : dw - 1;
            double *ar = sA + i * LDA;
            for (int c = j + 1 + tid % TPR; c <= cmax; c += TPR) ar[c] = fma(-li, sCol[c], ar[c]);
        }
    }
    if (!ok) {                                  // x_pi and e stay as they are
        if (tid == 0) flags[row] = 1;
        return;
    }
    // ---- back substitution L^T delta = z; x_pi -= delta --------------------------------------------------------------------
    double *z = sA + dw * LDA;
    if (tid < KP) sDelta[tid] = 0.0;
    for (int j = dw - 1; j >= 0; --j) {
        __syncthreads();
        const double dj = z[j] / sDiag[j];
        if (tid < j) z[tid] = fma(-sA[j * LDA + tid], dj, z[tid]);
        if (tid == j) {
            sDelta[j] = dj;
            xblk[j] -= dj;
        }
    }
    if (tid == 0) flags[row] = 0;
    __syncthreads();
    // ---- e_i -= y_{i,pi} . delta: 16 lanes per entry, 16 entries per pass ---------------------------------------------------
    const int grp = tid >> 4, l = tid & 15;
    for (int64_t q0 = 0; q0 < n; q0 += IALSPP_THREADS / 16) {
        const int64_t q = q0 + grp;
        double part = 0.0;
        if (q < n) {
            const int32_t idx = indices[beg + q];
            if (idx >= 0 && idx < n_cols) {
                const double *yr = Y + (int64_t)idx * ldy + p0;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int j = l + 16 * t;
                    if (j < dw) part = fma(yr[j], sDelta[j], part);
                }
            }
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        if (q < n && l == 0) E[beg + q] -= part;
    }
}

// info[0] = number of flagged rows, info[1] = the first of them (-1: none); the pattern of ials_info_kernel (ials.hip)
__global__ __launch_bounds__(IALSPP_REDUCE_THREADS) void ialspp_info_kernel(int64_t n_rows, const int32_t *__restrict__ flags,
                                                                           int32_t *__restrict__ info) {
    __shared__ int32_t s_cnt[IALSPP_REDUCE_THREADS];
    __shared__ int64_t s_first[IALSPP_REDUCE_THREADS];
    int32_t cnt = 0;
    int64_t first = n_rows;
    for (int64_t r = threadIdx.x; r < n_rows; r += IALSPP_REDUCE_THREADS)
        if (flags[r]) {
            ++cnt;
            if (r < first) first = r;
        }
    s_cnt[threadIdx.x] = cnt;
    s_first[threadIdx.x] = first;
    __syncthreads();
    for (int h = IALSPP_REDUCE_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
            if (s_first[threadIdx.x + h] < s_first[threadIdx.x]) s_first[threadIdx.x] = s_first[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        info[0] = s_cnt[0];
        info[1] = s_cnt[0] ? (int32_t)s_first[0] : -1;
    }
}

extern "C" int32_t pk_ialspp_max_rank(void) { return IALSPP_MAX_RANK; }

// the row flags of a block step (int32); the block width does not enter
extern "C" int64_t pk_ialspp_work_bytes(int64_t n_rows, int32_t block_size) {
    (void)block_size;
    return (n_rows < 1 ? 1 : n_rows) * 4 + 64;
}

extern "C" int pk_ialspp_block_step_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t rank, int32_t p0, int32_t block_size,
                                        const int64_t *indptr_dev, const int32_t *indices_dev, const double *conf_dev,
                                        const int32_t *row_order_dev, const double *Y_dev, int64_t ldy, const double *G_dev,
                                        int64_t ldg, double lambda, const double *lambda_rows_dev, const double *R_dev, int64_t ldr,
                                        double *X_dev, int64_t ldx, double *E_dev, int32_t *info_dev, void *work_dev) {
    PK_REQUIRE(rank >= 1 && rank <= IALSPP_MAX_RANK, "pk_ialspp_block_step_f64: rank %d outside 1..%d", (int)rank, IALSPP_MAX_RANK);
    PK_REQUIRE(block_size == 16 || block_size == 32 || block_size == 64, "pk_ialspp_block_step_f64: block size %d is not 16, 32 or 64",
               (int)block_size);
    PK_REQUIRE(p0 >= 0 && p0 < rank, "pk_ialspp_block_step_f64: block start %d outside the rank %d", (int)p0, (int)rank);
    PK_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && n_cols >= 0 && n_cols < (1ll << 31),
               "pk_ialspp_block_step_f64: %lld rows, %lld columns (32-bit ids)", (long long)n_rows, (long long)n_cols);
    PK_REQUIRE(indptr_dev && Y_dev && G_dev && R_dev && X_dev && E_dev && info_dev && work_dev && X_dev != Y_dev,
               "pk_ialspp_block_step_f64: bad pointers");
    const int dw = rank - p0 < block_size ? rank - p0 : block_size;
    PK_REQUIRE(ldy >= rank && ldg >= rank && ldx >= rank && ldr >= dw, "pk_ialspp_block_step_f64: bad leading dimension");
    hipStream_t st = pk_stream(stream);
    int32_t *flags = (int32_t *)work_dev;
    if (n_rows > 0) {
#define IALSPP_CASE(NT)                                                                                                            \
    case NT:                                                                                                                       \
        hipLaunchKernelGGL(ialspp_block_step_kernel<NT>, dim3((unsigned)n_rows), dim3(IALSPP_THREADS),                             \
                           (size_t)IalsppShape<NT>::LDS_DOUBLES * sizeof(double), st, n_rows, n_cols, (int)p0, dw, indptr_dev,     \
                           indices_dev, conf_dev, row_order_dev, Y_dev, ldy, G_dev, ldg, lambda, lambda_rows_dev, R_dev, ldr, X_dev, \
                           ldx, E_dev, flags);                                                                                     \
        break;
        switch (block_size / 16) {
            IALSPP_CASE(1) IALSPP_CASE(2) IALSPP_CASE(4)
        }
#undef IALSPP_CASE
        PK_CHECK_LAUNCH("ialspp_block_step_kernel");
    }
    hipLaunchKernelGGL(ialspp_info_kernel, dim3(1), dim3(IALSPP_REDUCE_THREADS), 0, st, n_rows, (const int32_t *)flags, info_dev);
    PK_CHECK_LAUNCH("ialspp_info_kernel");
    return PK_OK;
}

// ---- the cached predictions: e[p] = x_u . y_i for every stored entry, in storage order ------------------------------------------
// XR = columns per lane (the rank padded to 64 XR): 2 up to rank 128, 8 up to 512, 32 up to 2048
template <int XR>
__global__ __launch_bounds__(256) void ialspp_predict_kernel(int64_t n_rows, int64_t n_cols, int k, const int64_t *__restrict__ indptr,
                                                             const int32_t *__restrict__ indices, const double *__restrict__ X,
                                                             int64_t ldx, const double *__restrict__ Y, int64_t ldy,
                                                             double *__restrict__ E) {
    const int lane = pk_lane();
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int64_t end = indptr[row + 1];
    int64_t p = indptr[row] + blockIdx.y;       // an entry is a sum of its own: the segments of a row share nothing
    if (p >= end) return;
    double x[XR];
#pragma unroll
    for (int t = 0; t < XR; ++t) x[t] = lane + 64 * t < k ? X[row * ldx + lane + 64 * t] : 0.0;
    for (; p < end; p += gridDim.y) {
        const int32_t idx = indices[p];
        double acc = 0.0;
        if (idx >= 0 && idx < n_cols) {
            const double *yr = Y + (int64_t)idx * ldy + lane;
#pragma unroll
            for (int t = 0; t < XR; ++t)
                if (lane + 64 * t < k) acc = fma(x[t], yr[64 * t], acc);
        }
        const double s = pk_wave_sum(acc);
        if (lane == 0) E[p] = s;
    }
}

extern "C" int pk_ialspp_predict_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t rank, const int64_t *indptr_dev,
                                     const int32_t *indices_dev, const double *X_dev, int64_t ldx, const double *Y_dev, int64_t ldy,
                                     double *E_dev) {
    PK_REQUIRE(rank >= 1 && rank <= IALSPP_MAX_RANK, "pk_ialspp_predict_f64: rank %d outside 1..%d", (int)rank, IALSPP_MAX_RANK);
    PK_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && n_cols >= 0 && n_cols < (1ll << 31),
               "pk_ialspp_predict_f64: %lld rows, %lld columns (32-bit ids)", (long long)n_rows, (long long)n_cols);
    PK_REQUIRE(indptr_dev && X_dev && Y_dev && E_dev, "pk_ialspp_predict_f64: bad pointers");
    PK_REQUIRE(ldx >= rank && ldy >= rank, "pk_ialspp_predict_f64: bad leading dimension");
    if (n_rows == 0) return PK_OK;
    hipStream_t st = pk_stream(stream);
    const dim3 grid((unsigned)pk_ceil_div(n_rows, 4), IALSPP_PREDICT_SEGMENTS), block(256);
    if (rank <= 128)
        hipLaunchKernelGGL(ialspp_predict_kernel<2>, grid, block, 0, st, n_rows, n_cols, (int)rank, indptr_dev, indices_dev, X_dev, ldx,
                           Y_dev, ldy, E_dev);
    else if (rank <= 512)
        hipLaunchKernelGGL(ialspp_predict_kernel<8>, grid, block, 0, st, n_rows, n_cols, (int)rank, indptr_dev, indices_dev, X_dev, ldx,
                           Y_dev, ldy, E_dev);
    else
        hipLaunchKernelGGL(ialspp_predict_kernel<32>, grid, block, 0, st, n_rows, n_cols, (int)rank, indptr_dev, indices_dev, X_dev, ldx,
                           Y_dev, ldy, E_dev);
    PK_CHECK_LAUNCH("ialspp_predict_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_ialspp() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&ialspp_info_kernel));
}
