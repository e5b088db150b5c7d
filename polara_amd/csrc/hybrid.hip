// HybridSVD (hybrid/models.py:228-397) on the device: a dense Cholesky factor L of the item-similarity matrix
// K = S + beta I, and the three products the model needs of it.
//
//   * densify: K is scattered from a CSR of S (external item ids) into a dense fp64 image in the device's internal item
//     order — lower triangle only, + beta on the diagonal;
//   * pk_chol_f64: right-looking blocked Cholesky, 64-wide blocks.  Per step: the diagonal block is factored in one
//     workgroup (LDS), the panel below it is solved row by row (one lane per row, the row in registers), and the trailing
//     lower triangle gets the rank-64 update on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, one 64 x 64 tile per
//     workgroup).  The image is padded to whole tiles (pk_hybrid_ld): the padding is set to the identity first, so no
//     kernel needs a bounds check and the factor of the padded matrix is diag(L, I).  A pivot <= 0 or not finite writes
//     its column to a device int, and every later kernel of the call returns at once: nothing non-finite is written;
//   * pk_trmm_f64: Y = L X or L^T X for X of n x nc (nc <= 64): a task reads a strip of up to 32 tiles of the triangle
//     (each tile once, the next one fetched into registers while the current one runs on the matrix cores) and writes
//     a partial block; a second kernel adds the partials of a row in a fixed order;
//   * pk_trsm_f64: X = L^-T B, blocked back substitution: per block row (last to first) the diagonal block is solved
//     (one lane per column), then the blocks above it are updated on the matrix cores;
//   * EASE on the same image (the section at the end): the Gram diagonal, pk_trtri_f64 (L^-1 in place) and
//     pk_ease_weights_f64 (the scaled weights from L^-T L^-1, never stored).
//
// MFMA layout (MI355X guide, the same map as dense.hip's gram_kernel): D[16 x 16] += P[16 x 4] Q[4 x 16] with lane l
// holding P[l & 15][l >> 4], Q[l >> 4][l & 15] and D[(l >> 4) + 4 r][l & 15] in register r.
#include "pk_common.h"

#define PK_HYB_NB 64          // tile / block width
#define PK_HYB_MAX_NC 64      // columns of X one pk_trmm_f64 call takes
#define PK_HYB_CHUNK 32       // tiles of L one trmm task reads
#define PK_HYB_S 65           // LDS row stride (doubles) of a staged 64 x 64 tile

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- planning (host functions) --------------------------------------------------------------------------------------
extern "C" int64_t pk_hybrid_ld(int64_t n) { return pk_ceil_div(n, PK_HYB_NB) * PK_HYB_NB; }
extern "C" int32_t pk_hybrid_max_nc(void) { return PK_HYB_MAX_NC; }
static int64_t trmm_chunks(int64_t n) { return pk_ceil_div(pk_ceil_div(n, PK_HYB_NB), PK_HYB_CHUNK); }
extern "C" int64_t pk_trmm_work_bytes(int64_t n, int32_t nc) {
    const int64_t ch = trmm_chunks(n);
    return ch > 1 ? ch * pk_hybrid_ld(n) * (int64_t)nc * (int64_t)sizeof(double) : 0;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ int64_t hyb_min(int64_t a, int64_t b) { return a < b ? a : b; }

// ---- 64 x 64 tile staging: global (16-byte loads, 8 per thread) -> registers -> LDS ------------------------------------
struct TileRegs {
    double2 v[8];
};

__device__ __forceinline__ void tile_fetch(TileRegs &r, const double *__restrict__ A, int64_t ld, int64_t row0, int64_t col0) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int slot = tid + 256 * q;
        r.v[q] = *reinterpret_cast<const double2 *>(A + (row0 + (slot >> 5)) * ld + col0 + (slot & 31) * 2);
    }
}

// lower = true: entries above the tile's diagonal are stored as 0 (a diagonal tile of a triangle)
__device__ __forceinline__ void tile_store(double (*s)[PK_HYB_S], const TileRegs &r, bool lower) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int slot = tid + 256 * q;
        const int i = slot >> 5, c = (slot & 31) * 2;
        s[i][c] = (lower && c > i) ? 0.0 : r.v[q].x;
        s[i][c + 1] = (lower && c + 1 > i) ? 0.0 : r.v[q].y;
    }
}

// ---- padding and densify ------------------------------------------------------------------------------------------
// row i: the strict upper triangle is cleared; rows of the padding get the identity (columns [n, ld) of real rows lie in
// the upper triangle)
__global__ __launch_bounds__(256) void hyb_pad_kernel(int64_t n, int64_t npad, double *__restrict__ A, int64_t ld) {
    const int64_t i = blockIdx.x;
    double *row = A + i * ld;
    for (int64_t j = threadIdx.x; j < npad; j += 256) {
        if (j > i) row[j] = 0.0;
        else if (i >= n) row[j] = (j == i) ? 1.0 : 0.0;
    }
}

// one wave per row of S (external ids): entry (i, j) lands at (rank[i], rank[j]) when that lies in the lower triangle
__global__ __launch_bounds__(256) void hyb_densify_kernel(int64_t n, const int64_t *__restrict__ indptr,
                                                          const int64_t *__restrict__ indices, const double *__restrict__ data,
                                                          const int64_t *__restrict__ rank, double *__restrict__ K, int64_t ld) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t ri = rank[i];
    for (int64_t e = indptr[i] + (threadIdx.x & 63); e < indptr[i + 1]; e += 64) {
        const int64_t rj = rank[indices[e]];
        if (rj <= ri) K[ri * ld + rj] = data[e];
    }
}

__global__ __launch_bounds__(256) void hyb_diag_add_kernel(int64_t n, double *__restrict__ K, int64_t ld, double beta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) K[i * ld + i] += beta;
}

extern "C" int pk_hybrid_densify_f64(void *stream, int64_t n, const int64_t *indptr_dev, const int64_t *indices_dev,
                                     const double *data_dev, const int64_t *rank_dev, double beta, double *K_dev, int64_t ld) {
    PK_REQUIRE(n >= 1 && ld % PK_HYB_NB == 0 && ld >= pk_hybrid_ld(n), "pk_hybrid_densify_f64: bad sizes");
    PK_REQUIRE(K_dev != nullptr && indptr_dev != nullptr && rank_dev != nullptr, "pk_hybrid_densify_f64: null pointer");
    hipStream_t st = pk_stream(stream);
    if (hipMemsetAsync(K_dev, 0, (size_t)pk_hybrid_ld(n) * ld * sizeof(double), st) != hipSuccess) {
        pk_set_error("pk_hybrid_densify_f64: memset failed");
        return PK_E_LAUNCH;
    }
    hipLaunchKernelGGL(hyb_densify_kernel, dim3((unsigned)pk_ceil_div(n, 4)), dim3(256), 0, st, n, indptr_dev, indices_dev,
                       data_dev, rank_dev, K_dev, ld);
    PK_CHECK_LAUNCH("hyb_densify_kernel");
    hipLaunchKernelGGL(hyb_diag_add_kernel, dim3((unsigned)pk_ceil_div(n, 256)), dim3(256), 0, st, n, K_dev, ld, beta);
    PK_CHECK_LAUNCH("hyb_diag_add_kernel");
    return PK_OK;
}

// ---- Cholesky ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool hyb_bad_pivot(double d) { return !(d > 0.0) || !__builtin_isfinite(d); }

// the diagonal block at (k, k), unblocked right-looking in LDS
__global__ __launch_bounds__(256) void hyb_potrf_kernel(double *__restrict__ A, int64_t ld, int64_t k, int32_t *__restrict__ info) {
    __shared__ double s[PK_HYB_NB][PK_HYB_S];
    if (*info >= 0) return;
    const int tid = threadIdx.x;
    TileRegs r;
    tile_fetch(r, A, ld, k, k);
    tile_store(s, r, true);
    __syncthreads();
    for (int j = 0; j < PK_HYB_NB; ++j) {
        const double d = s[j][j];
        if (hyb_bad_pivot(d)) {                     // uniform: every thread read the same value
            if (tid == 0) *info = (int32_t)(k + j);
            return;                                 // nothing of this block is written back
        }
        const double sd = sqrt(d);
        __syncthreads();                            // everyone has read d
        if (tid > j && tid < PK_HYB_NB) s[tid][j] /= sd;
        if (tid == j) s[j][j] = sd;
        __syncthreads();
        for (int e = tid; e < PK_HYB_NB * PK_HYB_NB; e += 256) {
            const int i = e >> 6, c = e & 63;
            if (c > j && c <= i) s[i][c] -= s[i][j] * s[c][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < PK_HYB_NB * PK_HYB_NB; e += 256) {
        const int i = e >> 6, c = e & 63;
        if (c <= i) A[(k + i) * ld + k + c] = s[i][c];
    }
}

// rows [k + 64, npad) of block column k: x L_kk^T = b, one lane per row (the row lives in registers)
__global__ __launch_bounds__(256) void hyb_panel_kernel(double *__restrict__ A, int64_t ld, int64_t k, int64_t npad,
                                                        const int32_t *__restrict__ info) {
    __shared__ double s[PK_HYB_NB][PK_HYB_S];
    if (*info >= 0) return;
    TileRegs r;
    tile_fetch(r, A, ld, k, k);
    tile_store(s, r, true);
    __syncthreads();
    const int64_t row = k + PK_HYB_NB + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= npad) return;
    double *p = A + row * ld + k;
    double x[PK_HYB_NB];
#pragma unroll
    for (int c = 0; c < PK_HYB_NB; c += 2) {
        const double2 v = *reinterpret_cast<const double2 *>(p + c);
        x[c] = v.x;
        x[c + 1] = v.y;
    }
#pragma unroll
    for (int j = 0; j < PK_HYB_NB; ++j) {
        double v = x[j];
#pragma unroll
        for (int q = 0; q < j; ++q) v -= x[q] * s[j][q];
        x[j] = v / s[j][j];
    }
#pragma unroll
    for (int c = 0; c < PK_HYB_NB; c += 2) *reinterpret_cast<double2 *>(p + c) = make_double2(x[c], x[c + 1]);
}

// trailing update of the lower triangle: tile (I, J), I >= J, of the region [k + 64, npad)^2 gets  -= P_I P_J^T
__global__ __launch_bounds__(256) void hyb_syrk_kernel(double *__restrict__ A, int64_t ld, int64_t k,
                                                       const int32_t *__restrict__ info) {
    __shared__ double sP[PK_HYB_NB][PK_HYB_S];
    __shared__ double sQ[PK_HYB_NB][PK_HYB_S];
    if (*info >= 0) return;
    const int64_t x = blockIdx.x;
    int64_t I = (int64_t)((sqrt(8.0 * (double)x + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= x) ++I;
    while (I * (I + 1) / 2 > x) --I;
    const int64_t J = x - I * (I + 1) / 2;
    const int64_t r0 = k + PK_HYB_NB * (1 + I), c0 = k + PK_HYB_NB * (1 + J);
    TileRegs ra, rb;
    tile_fetch(ra, A, ld, r0, k);
    tile_fetch(rb, A, ld, c0, k);
    tile_store(sP, ra, false);
    tile_store(sQ, rb, false);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int p0 = 0; p0 < PK_HYB_NB; p0 += 4) {
        const double a = sP[16 * wave + (lane & 15)][p0 + (lane >> 4)];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sQ[16 * b + (lane & 15)][p0 + (lane >> 4)], acc[b], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int j = 16 * b + (lane & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 16 * wave + (lane >> 4) + 4 * q;
            if (I != J || j <= i) A[(r0 + i) * ld + c0 + j] -= acc[b][q];
        }
    }
}

extern "C" int pk_chol_f64(void *stream, int64_t n, double *A_dev, int64_t ld, int32_t *info_dev) {
    PK_REQUIRE(n >= 1 && ld % PK_HYB_NB == 0 && ld >= pk_hybrid_ld(n), "pk_chol_f64: bad sizes (n = %lld, ld = %lld)",
               (long long)n, (long long)ld);
    PK_REQUIRE(A_dev != nullptr && info_dev != nullptr && aligned16(A_dev), "pk_chol_f64: null or unaligned pointer");
    hipStream_t st = pk_stream(stream);
    const int64_t npad = pk_hybrid_ld(n), nb = npad / PK_HYB_NB;
    if (hipMemsetAsync(info_dev, 0xff, sizeof(int32_t), st) != hipSuccess) {      // -1: no failure
        pk_set_error("pk_chol_f64: memset failed");
        return PK_E_LAUNCH;
    }
    hipLaunchKernelGGL(hyb_pad_kernel, dim3((unsigned)npad), dim3(256), 0, st, n, npad, A_dev, ld);
    PK_CHECK_LAUNCH("hyb_pad_kernel");
    for (int64_t kb = 0; kb < nb; ++kb) {
        const int64_t k = kb * PK_HYB_NB;
        hipLaunchKernelGGL(hyb_potrf_kernel, dim3(1), dim3(256), 0, st, A_dev, ld, k, info_dev);
        PK_CHECK_LAUNCH("hyb_potrf_kernel");
        if (kb + 1 == nb) break;
        const int64_t rows = npad - k - PK_HYB_NB, T = nb - kb - 1;
        hipLaunchKernelGGL(hyb_panel_kernel, dim3((unsigned)pk_ceil_div(rows, 256)), dim3(256), 0, st, A_dev, ld, k, npad,
                           info_dev);
        PK_CHECK_LAUNCH("hyb_panel_kernel");
        hipLaunchKernelGGL(hyb_syrk_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, st, A_dev, ld, k, info_dev);
        PK_CHECK_LAUNCH("hyb_syrk_kernel");
    }
    return PK_OK;
}

// ---- triangular products -------------------------------------------------------------------------------------------
// rows [row0, row0 + 64) x columns [col0, col0 + 64) of X (n rows, nc columns) into sX, zeros outside
__device__ __forceinline__ void x_block_store(double (*sX)[PK_HYB_NB], const double *__restrict__ X, int64_t ldx, int64_t n,
                                              int nc, int64_t row0, int64_t col0) {
    for (int e = threadIdx.x; e < PK_HYB_NB * PK_HYB_NB; e += 256) {
        const int i = e >> 6, c = e & 63;
        const int64_t row = row0 + i, col = col0 + c;
        sX[i][c] = (row < n && col < nc) ? X[row * ldx + col] : 0.0;
    }
}

// strip s, chunk c: trans = 0 (Y = L X): tiles (s, t), t in [c CH, min((c + 1) CH, s + 1)), partial of Y rows of block s;
// trans = 1 (Y = L^T X): tiles (t, s), t in [s + c CH, min(s + (c + 1) CH, nb)), partial of Y rows of block s
__global__ __launch_bounds__(256) void hyb_trmm_kernel(int trans, int64_t n, int64_t nb, int nc, const double *__restrict__ L,
                                                       int64_t ld, const double *__restrict__ X, int64_t ldx,
                                                       double *__restrict__ Y, int64_t ldy, double *__restrict__ work, int nch) {
    __shared__ double sL[PK_HYB_NB][PK_HYB_S];
    __shared__ __attribute__((aligned(16))) double sX[PK_HYB_NB][PK_HYB_NB];
    const int64_t s = blockIdx.x, c = blockIdx.y;
    int64_t t0, t1;
    if (!trans) {
        t0 = c * PK_HYB_CHUNK;
        t1 = hyb_min(t0 + PK_HYB_CHUNK, s + 1);
    } else {
        t0 = s + c * PK_HYB_CHUNK;
        t1 = hyb_min(t0 + PK_HYB_CHUNK, nb);
    }
    if (t0 >= t1) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncb = (nc + 15) >> 4;
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    TileRegs r;
    auto tile_of = [&](int64_t t, int64_t &ti, int64_t &tj) {
        ti = trans ? t : s;
        tj = trans ? s : t;
    };
    int64_t ti, tj;
    tile_of(t0, ti, tj);
    tile_fetch(r, L, ld, ti * PK_HYB_NB, tj * PK_HYB_NB);
    for (int64_t t = t0; t < t1; ++t) {
        tile_of(t, ti, tj);
        tile_store(sL, r, ti == tj);
        x_block_store(sX, X, ldx, n, nc, (trans ? ti : tj) * PK_HYB_NB, 0);
        __syncthreads();
        if (t + 1 < t1) {
            int64_t ni, nj;
            tile_of(t + 1, ni, nj);
            tile_fetch(r, L, ld, ni * PK_HYB_NB, nj * PK_HYB_NB);
        }
#pragma unroll
        for (int k0 = 0; k0 < PK_HYB_NB; k0 += 4) {
            const double a = trans ? sL[k0 + (lane >> 4)][16 * wave + (lane & 15)] : sL[16 * wave + (lane & 15)][k0 + (lane >> 4)];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < ncb)
                    acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sX[k0 + (lane >> 4)][16 * b + (lane & 15)], acc[b], 0, 0, 0);
        }
        __syncthreads();
    }
    const int64_t npad = nb * PK_HYB_NB;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int j = 16 * b + (lane & 15);
        if (j >= nc) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = s * PK_HYB_NB + 16 * wave + (lane >> 4) + 4 * q;
            if (nch == 1) {
                if (i < n) Y[i * ldy + j] = acc[b][q];
            } else {
                work[(c * npad + i) * nc + j] = acc[b][q];
            }
        }
    }
}

// Y[i][j] = sum of the partials of row i in chunk order
__global__ __launch_bounds__(256) void hyb_trmm_reduce_kernel(int trans, int64_t n, int64_t nb, int nc,
                                                              const double *__restrict__ work, double *__restrict__ Y, int64_t ldy) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * nc) return;
    const int64_t i = e / nc, j = e % nc, s = i / PK_HYB_NB;
    const int64_t cnt = ((trans ? nb - s : s + 1) + PK_HYB_CHUNK - 1) / PK_HYB_CHUNK;
    const int64_t npad = nb * PK_HYB_NB;
    double v = 0.0;
    for (int64_t c = 0; c < cnt; ++c) v += work[(c * npad + i) * nc + j];
    Y[i * ldy + j] = v;
}

extern "C" int pk_trmm_f64(void *stream, int32_t trans, int64_t n, int32_t nc, const double *L_dev, int64_t ld,
                           const double *X_dev, int64_t ldx, double *Y_dev, int64_t ldy, void *work_dev) {
    PK_REQUIRE(n >= 1 && nc >= 1 && nc <= PK_HYB_MAX_NC, "pk_trmm_f64: bad sizes (n = %lld, nc = %d)", (long long)n, (int)nc);
    PK_REQUIRE(ld % PK_HYB_NB == 0 && ld >= pk_hybrid_ld(n) && ldx >= nc && ldy >= nc, "pk_trmm_f64: bad leading dimension");
    PK_REQUIRE(L_dev != nullptr && X_dev != nullptr && Y_dev != nullptr && aligned16(L_dev), "pk_trmm_f64: null or unaligned pointer");
    const int64_t nb = pk_hybrid_ld(n) / PK_HYB_NB, nch = trmm_chunks(n);
    PK_REQUIRE(nch == 1 || work_dev != nullptr, "pk_trmm_f64: work buffer required (pk_trmm_work_bytes)");
    hipStream_t st = pk_stream(stream);
    hipLaunchKernelGGL(hyb_trmm_kernel, dim3((unsigned)nb, (unsigned)nch), dim3(256), 0, st, (int)(trans != 0), n, nb, (int)nc,
                       L_dev, ld, X_dev, ldx, Y_dev, ldy, static_cast<double *>(work_dev), (int)nch);
    PK_CHECK_LAUNCH("hyb_trmm_kernel");
    if (nch > 1) {
        hipLaunchKernelGGL(hyb_trmm_reduce_kernel, dim3((unsigned)pk_ceil_div(n * nc, 256)), dim3(256), 0, st, (int)(trans != 0),
                           n, nb, (int)nc, static_cast<const double *>(work_dev), Y_dev, ldy);
        PK_CHECK_LAUNCH("hyb_trmm_reduce_kernel");
    }
    return PK_OK;
}

// ---- triangular solve X = L^-T B (in place on B) ---------------------------------------------------------------------
// block row J: L_JJ^T x = b per column (one lane per column, the column in registers)
__global__ __launch_bounds__(64) void hyb_trsm_diag_kernel(int r, const double *__restrict__ L, int64_t ld, int64_t J,
                                                           double *__restrict__ B, int64_t ldb) {
    __shared__ double s[PK_HYB_NB][PK_HYB_S];
    const int tid = threadIdx.x;
    const int64_t row0 = J * PK_HYB_NB;
    for (int e = tid; e < PK_HYB_NB * PK_HYB_NB; e += 64) {
        const int i = e >> 6, c = e & 63;
        s[i][c] = c <= i ? L[(row0 + i) * ld + row0 + c] : 0.0;
    }
    __syncthreads();
    const int64_t col = (int64_t)blockIdx.x * 64 + tid;
    if (col >= r) return;
    double x[PK_HYB_NB];
#pragma unroll
    for (int i = 0; i < PK_HYB_NB; ++i) x[i] = B[(row0 + i) * ldb + col];
#pragma unroll
    for (int j = PK_HYB_NB - 1; j >= 0; --j) {
        double v = x[j];
#pragma unroll
        for (int i = j + 1; i < PK_HYB_NB; ++i) v -= s[i][j] * x[i];
        x[j] = v / s[j][j];
    }
#pragma unroll
    for (int i = 0; i < PK_HYB_NB; ++i) B[(row0 + i) * ldb + col] = x[i];
}

// blocks I < J of B (columns [64 y, 64 y + 64)):  B_I -= L_JI^T X_J
__global__ __launch_bounds__(256) void hyb_trsm_update_kernel(int r, const double *__restrict__ L, int64_t ld, int64_t J,
                                                              double *__restrict__ B, int64_t ldb) {
    __shared__ double sL[PK_HYB_NB][PK_HYB_S];
    __shared__ __attribute__((aligned(16))) double sX[PK_HYB_NB][PK_HYB_NB];
    const int64_t I = blockIdx.x, col0 = (int64_t)blockIdx.y * PK_HYB_NB;
    TileRegs t;
    tile_fetch(t, L, ld, J * PK_HYB_NB, I * PK_HYB_NB);
    tile_store(sL, t, false);
    const int nc = (int)hyb_min(PK_HYB_NB, (int64_t)r - col0);
    for (int e = threadIdx.x; e < PK_HYB_NB * PK_HYB_NB; e += 256) {
        const int i = e >> 6, c = e & 63;
        sX[i][c] = c < nc ? B[(J * PK_HYB_NB + i) * ldb + col0 + c] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncb = (nc + 15) >> 4;
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k0 = 0; k0 < PK_HYB_NB; k0 += 4) {
        const double a = sL[k0 + (lane >> 4)][16 * wave + (lane & 15)];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b < ncb)
                acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sX[k0 + (lane >> 4)][16 * b + (lane & 15)], acc[b], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int j = 16 * b + (lane & 15);
        if (j >= nc) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = I * PK_HYB_NB + 16 * wave + (lane >> 4) + 4 * q;
            B[i * ldb + col0 + j] -= acc[b][q];
        }
    }
}

extern "C" int pk_trsm_f64(void *stream, int64_t n, int32_t r, const double *L_dev, int64_t ld, double *B_dev, int64_t ldb) {
    PK_REQUIRE(n >= 1 && r >= 1 && ld % PK_HYB_NB == 0 && ld >= pk_hybrid_ld(n) && ldb >= r, "pk_trsm_f64: bad sizes");
    PK_REQUIRE(L_dev != nullptr && B_dev != nullptr && aligned16(L_dev), "pk_trsm_f64: null or unaligned pointer");
    hipStream_t st = pk_stream(stream);
    const int64_t npad = pk_hybrid_ld(n), nb = npad / PK_HYB_NB;
    if (npad > n && hipMemset2DAsync(B_dev + n * ldb, (size_t)ldb * sizeof(double), 0, (size_t)r * sizeof(double),
                                     (size_t)(npad - n), st) != hipSuccess) {
        pk_set_error("pk_trsm_f64: memset failed");
        return PK_E_LAUNCH;
    }
    const unsigned cchunks = (unsigned)pk_ceil_div(r, PK_HYB_NB);
    for (int64_t J = nb - 1; J >= 0; --J) {
        hipLaunchKernelGGL(hyb_trsm_diag_kernel, dim3(cchunks), dim3(64), 0, st, (int)r, L_dev, ld, J, B_dev, ldb);
        PK_CHECK_LAUNCH("hyb_trsm_diag_kernel");
        if (J == 0) break;
        hipLaunchKernelGGL(hyb_trsm_update_kernel, dim3((unsigned)J, cchunks), dim3(256), 0, st, (int)r, L_dev, ld, J, B_dev, ldb);
        PK_CHECK_LAUNCH("hyb_trsm_update_kernel");
    }
    return PK_OK;
}

// ---- EASE: Gram diagonal, triangular inverse, weights ------------------------------------------------------------------
// B = I - P diag(1 / diag P), P = (X^T X + lambda I)^-1 = W^T W with W = L^-1.
//   * pk_ease_diag_f64: the diagonal pk_i2i_build_f64 leaves at 0, from the CSC image of X;
//   * pk_trtri_f64: W in place, block columns last to first (LAPACK's dtrtri('L') order).  All diagonal blocks are
//     inverted first (they depend on nothing else: one workgroup each, one lane per column of the inverse).  At block
//     column J the triangle below and to the right holds W already and the panel L[J + 1 :, J] is still L's:
//         W[J + 1 :, J] = -(W[J + 1 :, J + 1 :] L[J + 1 :, J]) W_JJ
//     the first product runs as tasks of up to 32 tiles of a tile row, each writing a partial block into the work buffer
//     (the panel is read by every task and must not change under them); the second kernel adds the partials of a tile
//     in chunk order, multiplies by the inverted diagonal block and writes the panel;
//   * pk_ease_weights_f64: d_j = sum_k W_kj^2, then one workgroup per tile pair (I, J), I >= J, sums W_KI^T W_KJ over
//     K >= I and writes both mirrored tiles of B, scaled, through LDS (both with unit-stride rows).
#define PK_EASE_GROUP 16      // lanes per item of the Gram diagonal

__device__ __forceinline__ double hyb_val(const void *v, int kind, int64_t p) {
    return kind == PK_VAL_F32 ? (double)static_cast<const float *>(v)[p] : static_cast<const double *>(v)[p];
}

__global__ __launch_bounds__(256) void ease_diag_kernel(int64_t n, const int64_t *__restrict__ t_indptr,
                                                        const void *__restrict__ t_values, int kind, double lam,
                                                        double *__restrict__ K, int64_t ld) {
    const int64_t j = (int64_t)blockIdx.x * (256 / PK_EASE_GROUP) + threadIdx.x / PK_EASE_GROUP;
    const int l = threadIdx.x % PK_EASE_GROUP;
    double s = 0.0;
    if (j < n)
        for (int64_t p = t_indptr[j] + l; p < t_indptr[j + 1]; p += PK_EASE_GROUP) {
            const double x = hyb_val(t_values, kind, p);
            s += x * x;
        }
#pragma unroll
    for (int o = PK_EASE_GROUP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, PK_EASE_GROUP);      // a + b == b + a: every lane agrees
    if (j < n && l == 0) K[j * ld + j] = s + lam;
}

extern "C" int pk_ease_diag_f64(void *stream, int64_t n_items, const int64_t *t_indptr_dev, const void *t_values_dev,
                                int val_kind, double lam, double *K_dev, int64_t ld) {
    PK_REQUIRE(n_items >= 1 && ld >= n_items, "pk_ease_diag_f64: bad sizes (n_items = %lld, ld = %lld)", (long long)n_items,
               (long long)ld);
    PK_REQUIRE(t_indptr_dev != nullptr && K_dev != nullptr && (val_kind == PK_VAL_F32 || val_kind == PK_VAL_F64),
               "pk_ease_diag_f64: null pointer or bad val_kind");
    hipLaunchKernelGGL(ease_diag_kernel, dim3((unsigned)pk_ceil_div(n_items, 256 / PK_EASE_GROUP)), dim3(256), 0,
                       pk_stream(stream), n_items, t_indptr_dev, t_values_dev, val_kind, lam, K_dev, ld);
    PK_CHECK_LAUNCH("ease_diag_kernel");
    return PK_OK;
}

// diagonal block b: L_bb x = e_j per column j of the inverse (one lane per column, forward substitution in LDS)
__global__ __launch_bounds__(256) void hyb_trtri_diag_kernel(double *__restrict__ A, int64_t ld) {
    __shared__ double s[PK_HYB_NB][PK_HYB_S];
    __shared__ double x[PK_HYB_NB][PK_HYB_S];
    const int64_t k = (int64_t)blockIdx.x * PK_HYB_NB;
    TileRegs r;
    tile_fetch(r, A, ld, k, k);
    tile_store(s, r, true);
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= PK_HYB_NB) return;
    // x_i = (e_j[i] - sum over j <= q < i of L_iq x_q) / L_ii, q ascending; the column lives in LDS (x[q][j]: its own bank)
    x[j][j] = 1.0 / s[j][j];
    for (int i = j + 1; i < PK_HYB_NB; ++i) {
        double v = 0.0;
        for (int q = j; q < i; ++q) v -= s[i][q] * x[q][j];
        x[i][j] = v / s[i][i];
    }
    for (int i = j; i < PK_HYB_NB; ++i) A[(k + i) * ld + k + j] = x[i][j];
}

// tile row s, chunk c of the panel product below diagonal block J: the partial sum over t in [32 c, min(32 c + 32, s + 1)) of
// W[off + 64 s, off + 64 t] L[off + 64 t, 64 J], off = 64 (J + 1), both tiles of the next step fetched into registers while
// the current pair is on the matrix cores
__global__ __launch_bounds__(256) void hyb_trtri_prod_kernel(const double *__restrict__ A, int64_t ld, int64_t J, int64_t nbt,
                                                             double *__restrict__ work) {
    __shared__ double sW[PK_HYB_NB][PK_HYB_S];
    __shared__ double sX[PK_HYB_NB][PK_HYB_S];
    const int64_t s = blockIdx.x, c = blockIdx.y;
    const int64_t t0 = c * PK_HYB_CHUNK, t1 = hyb_min(t0 + PK_HYB_CHUNK, s + 1);
    if (t0 >= t1) return;
    const int64_t col0 = J * PK_HYB_NB, off = col0 + PK_HYB_NB, row0 = off + s * PK_HYB_NB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    TileRegs rw, rx;
    tile_fetch(rw, A, ld, row0, off + t0 * PK_HYB_NB);
    tile_fetch(rx, A, ld, off + t0 * PK_HYB_NB, col0);
    for (int64_t t = t0; t < t1; ++t) {
        tile_store(sW, rw, t == s);
        tile_store(sX, rx, false);
        __syncthreads();
        if (t + 1 < t1) {
            tile_fetch(rw, A, ld, row0, off + (t + 1) * PK_HYB_NB);
            tile_fetch(rx, A, ld, off + (t + 1) * PK_HYB_NB, col0);
        }
#pragma unroll
        for (int k0 = 0; k0 < PK_HYB_NB; k0 += 4) {
            const double a = sW[16 * wave + (lane & 15)][k0 + (lane >> 4)];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sX[k0 + (lane >> 4)][16 * b + (lane & 15)], acc[b], 0, 0, 0);
        }
        __syncthreads();
    }
    double *w = work + (c * nbt + s) * PK_HYB_NB * PK_HYB_NB;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) w[(16 * wave + (lane >> 4) + 4 * q) * PK_HYB_NB + 16 * b + (lane & 15)] = acc[b][q];
}

// tile s of the panel below diagonal block J (row0 = 64 (J + 1 + s), col0 = 64 J): -(sum of its partials) W_JJ
__global__ __launch_bounds__(256) void hyb_trtri_panel_kernel(double *__restrict__ A, int64_t ld, int64_t J, int64_t nbt,
                                                              const double *__restrict__ work) {
    __shared__ double sY[PK_HYB_NB][PK_HYB_S];
    __shared__ double sD[PK_HYB_NB][PK_HYB_S];
    const int64_t s = blockIdx.x, col0 = J * PK_HYB_NB, row0 = col0 + PK_HYB_NB * (1 + s);
    TileRegs r;
    tile_fetch(r, A, ld, col0, col0);
    tile_store(sD, r, true);
    const int64_t cnt = (s + PK_HYB_CHUNK) / PK_HYB_CHUNK, cstride = nbt * PK_HYB_NB * PK_HYB_NB;
    const double *w = work + s * PK_HYB_NB * PK_HYB_NB;
    for (int e = threadIdx.x; e < PK_HYB_NB * PK_HYB_NB; e += 256) {
        double v = w[e];
        for (int64_t c = 1; c < cnt; ++c) v += w[c * cstride + e];
        sY[e >> 6][e & 63] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k0 = 0; k0 < PK_HYB_NB; k0 += 4) {
        const double a = sY[16 * wave + (lane & 15)][k0 + (lane >> 4)];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sD[k0 + (lane >> 4)][16 * b + (lane & 15)], acc[b], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int j = 16 * b + (lane & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 16 * wave + (lane >> 4) + 4 * q;
            A[(row0 + i) * ld + col0 + j] = -acc[b][q];
        }
    }
}

static int64_t trtri_chunks(int64_t n) {
    const int64_t below = pk_ceil_div(n, PK_HYB_NB) - 1;            // tile rows of the longest panel
    return below > 0 ? pk_ceil_div(below, PK_HYB_CHUNK) : 0;
}
extern "C" int64_t pk_trtri_work_bytes(int64_t n) {
    if (n < 1) return 0;
    return trtri_chunks(n) * (pk_hybrid_ld(n) - PK_HYB_NB) * PK_HYB_NB * (int64_t)sizeof(double);
}

extern "C" int pk_trtri_f64(void *stream, int64_t n, double *L_dev, int64_t ld, void *work_dev) {
    PK_REQUIRE(n >= 1 && ld % PK_HYB_NB == 0 && ld >= pk_hybrid_ld(n), "pk_trtri_f64: bad sizes (n = %lld, ld = %lld)",
               (long long)n, (long long)ld);
    PK_REQUIRE(L_dev != nullptr && aligned16(L_dev), "pk_trtri_f64: null or unaligned pointer");
    const int64_t nb = pk_hybrid_ld(n) / PK_HYB_NB;
    PK_REQUIRE(nb == 1 || work_dev != nullptr, "pk_trtri_f64: work buffer required (pk_trtri_work_bytes)");
    hipStream_t st = pk_stream(stream);
    double *work = static_cast<double *>(work_dev);
    hipLaunchKernelGGL(hyb_trtri_diag_kernel, dim3((unsigned)nb), dim3(256), 0, st, L_dev, ld);
    PK_CHECK_LAUNCH("hyb_trtri_diag_kernel");
    for (int64_t J = nb - 2; J >= 0; --J) {
        const int64_t nbt = nb - J - 1, nch = pk_ceil_div(nbt, PK_HYB_CHUNK);
        // Y = W[off :, off :] L[off :, J]: chunk c of tile row s at work[(c nbt + s) 64 + i][j]
        hipLaunchKernelGGL(hyb_trtri_prod_kernel, dim3((unsigned)nbt, (unsigned)nch), dim3(256), 0, st, L_dev, ld, J, nbt, work);
        PK_CHECK_LAUNCH("hyb_trtri_prod_kernel");
        hipLaunchKernelGGL(hyb_trtri_panel_kernel, dim3((unsigned)nbt), dim3(256), 0, st, L_dev, ld, J, nbt, work);
        PK_CHECK_LAUNCH("hyb_trtri_panel_kernel");
    }
    return PK_OK;
}

// d[j] = sum_k W[k][j]^2 over the rows of tile row b and below: four row phases per column, added in a fixed order
__global__ __launch_bounds__(256) void ease_colsq_kernel(int64_t n, int64_t npad, const double *__restrict__ W, int64_t ld,
                                                         double *__restrict__ d) {
    __shared__ double part[4][PK_HYB_NB];
    const int c = threadIdx.x & 63, p = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * PK_HYB_NB + c;
    double s = 0.0;
#pragma unroll 4
    for (int64_t k = (int64_t)blockIdx.x * PK_HYB_NB + p; k < npad; k += 4) {
        const double w = W[k * ld + j];
        s = fma(w, w, s);
    }
    part[p][c] = s;
    __syncthreads();
    if (p == 0 && j < n) d[j] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

// tile pair x = (I, J), I >= J (I ascending with x: the long sums start first): P_IJ = sum over K >= I of W_KI^T W_KJ,
// then B[I tile][J tile] = -P / d_J (columns) and B[J tile][I tile] = -P^T / d_I
__global__ __launch_bounds__(256) void ease_weights_kernel(int64_t n, int64_t nb, const double *__restrict__ W, int64_t ld,
                                                           const double *__restrict__ d, double *__restrict__ B, int64_t ldb) {
    __shared__ double sA[PK_HYB_NB][PK_HYB_S];
    __shared__ double sB[PK_HYB_NB][PK_HYB_S];
    __shared__ double sdi[PK_HYB_NB], sdj[PK_HYB_NB];
    const int64_t x = blockIdx.x;
    int64_t I = (int64_t)((sqrt(8.0 * (double)x + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= x) ++I;
    while (I * (I + 1) / 2 > x) --I;
    const int64_t J = x - I * (I + 1) / 2;
    const int64_t i0 = I * PK_HYB_NB, j0 = J * PK_HYB_NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    TileRegs ra, rb;
    tile_fetch(ra, W, ld, i0, i0);
    tile_fetch(rb, W, ld, i0, j0);
    for (int64_t K = I; K < nb; ++K) {
        tile_store(sA, ra, K == I);
        tile_store(sB, rb, K == J);
        __syncthreads();
        if (K + 1 < nb) {
            tile_fetch(ra, W, ld, (K + 1) * PK_HYB_NB, i0);
            tile_fetch(rb, W, ld, (K + 1) * PK_HYB_NB, j0);
        }
#pragma unroll
        for (int k0 = 0; k0 < PK_HYB_NB; k0 += 4) {
            const double a = sA[k0 + (lane >> 4)][16 * wave + (lane & 15)];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[k0 + (lane >> 4)][16 * b + (lane & 15)], acc[b], 0, 0, 0);
        }
        __syncthreads();
    }
    // P tile into sA (every wave is past its last read of it), the diagonal entries of both tiles next to it
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) sA[16 * wave + (lane >> 4) + 4 * q][16 * b + (lane & 15)] = acc[b][q];
    if (tid < PK_HYB_NB) {
        sdi[tid] = i0 + tid < n ? d[i0 + tid] : 1.0;
        sdj[tid] = j0 + tid < n ? d[j0 + tid] : 1.0;
    }
    __syncthreads();
    for (int e = tid; e < PK_HYB_NB * PK_HYB_NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        const int64_t gi = i0 + r, gj = j0 + c;                   // B[I tile][J tile]: row r, column c = P[r][c]
        if (gi < n && gj < n && (I != J || c <= r)) B[gi * ldb + gj] = (gi == gj) ? 0.0 : -sA[r][c] / sdj[c];
        const int64_t hi = j0 + r, hj = i0 + c;                   // B[J tile][I tile]: row r, column c = P[c][r]
        if (hi < n && hj < n && (I != J || c > r)) B[hi * ldb + hj] = -sA[c][r] / sdi[c];
    }
}

extern "C" int pk_ease_weights_f64(void *stream, int64_t n, const double *W_dev, int64_t ld, double *d_out_dev, double *B_dev,
                                   int64_t ldb) {
    PK_REQUIRE(n >= 1 && ld % PK_HYB_NB == 0 && ld >= pk_hybrid_ld(n) && ldb >= n,
               "pk_ease_weights_f64: bad sizes (n = %lld, ld = %lld, ldb = %lld)", (long long)n, (long long)ld, (long long)ldb);
    PK_REQUIRE(W_dev != nullptr && d_out_dev != nullptr && B_dev != nullptr && aligned16(W_dev),
               "pk_ease_weights_f64: null or unaligned pointer");
    const int64_t npad = pk_hybrid_ld(n), nb = npad / PK_HYB_NB, pairs = nb * (nb + 1) / 2;
    PK_REQUIRE(pairs <= 0x7fffffff, "pk_ease_weights_f64: catalogue too large for the grid");
    hipStream_t st = pk_stream(stream);
    if (ldb > n && hipMemset2DAsync(B_dev + n, (size_t)ldb * sizeof(double), 0, (size_t)(ldb - n) * sizeof(double), (size_t)n,
                                    st) != hipSuccess) {
        pk_set_error("pk_ease_weights_f64: memset failed");
        return PK_E_LAUNCH;
    }
    hipLaunchKernelGGL(ease_colsq_kernel, dim3((unsigned)nb), dim3(256), 0, st, n, npad, W_dev, ld, d_out_dev);
    PK_CHECK_LAUNCH("ease_colsq_kernel");
    hipLaunchKernelGGL(ease_weights_kernel, dim3((unsigned)pairs), dim3(256), 0, st, n, nb, W_dev, ld, d_out_dev, B_dev, ldb);
    PK_CHECK_LAUNCH("ease_weights_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_hybrid() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&hyb_syrk_kernel));
}
