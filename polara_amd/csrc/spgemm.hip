// Row-wise sparse x sparse product written back as a canonical CSR, with the similarity epilogues of the reference's
// lib/similarity.py fused in: the item similarity matrices S = f(F F^T) of the side-information models, built on the device.
//
//   C[r, :] = sum_p op(L.values[p], B[L.indices[p], :])        L: CSR [n_rows x n_inner], B: canonical CSR [n_inner x n_cols], fp64
//
// The sums are those of simagg.hip (spsp_accum.h: the same windows, the same order, bit-equal to SciPy's csr_matmat for
// op = MUL); op = MIN adds min(v, b) instead of v * b, the numerator of the weighted Jaccard index.  An entry is stored when
// its sum is != 0 (SciPy's numeric pass drops exact zeros, -0 included); with diag = 1 (square products) entry (r, r) is
// always stored, as 1.0 — set_diagonal_values(S, 1) fused in.
//
// Two passes over the (row, window) grid, both recomputing the window in LDS — no scratch proportional to the product:
//   1. spgemm_count_kernel: the stored entries of every (row, window) as int32; a window no wave touched leaves after the
//      accumulation without looking at its 2048 accumulators;
//   2. pk_exclusive_scan_i32 over the counts: the offset of every (row, window); those of window 0 are C.indptr;
//   3. spgemm_fill_kernel: the window again, its stored entries compacted in ascending column order: eight rounds of 256
//      consecutive columns, a ballot per wave, the four wave counts through LDS.
// No atomics on global memory, no order that depends on scheduling: the output is a function of the inputs alone.
// LDS: 16 KiB of accumulators + 272 B per workgroup of 256 threads, so the 160 KiB of a CU hold the 8 workgroups its
// 32 wave slots allow: occupancy is bound by waves, not by LDS.
#include "spsp_accum.h"

#define PK_SPGEMM_ROUNDS (PK_I2I_WIN / PK_I2I_THREADS)

struct SpgemmRows {        // the feature rows of one side of a weighted Jaccard pair (sorted columns)
    const int64_t *indptr;
    const int32_t *indices;
    const void *values;
    int kind;
};

struct SpgemmEpilogue {
    int kind;                     // PK_SPGEMM_EPI_*
    int wj_rect;                  // WJACCARD: 0 = symmetric (i = min(r, c), j = max(r, c), both rows from `cols`),
                                  //           1 = rectangular (j = the row, from `rows`; i = the column, from `cols`)
    const double *nf_rows, *nf_cols;
    SpgemmRows rows, cols;
};

// max_sum of _jaccard_similarity_weighted_tri for the pair (i, j): over row j in ascending order a matched feature adds
// max(dat_i, dat_j), an unmatched one dat_j; then the unmatched features of row i in ascending order.
__device__ double spgemm_wj_max_sum(const SpgemmRows &I, int64_t i, const SpgemmRows &J, int64_t j) {
    const int64_t i0 = I.indptr[i], i1 = I.indptr[i + 1], j0 = J.indptr[j], j1 = J.indptr[j + 1];
    double mx = 0.0;
    int64_t s = i0;
    for (int64_t k = j0; k < j1; ++k) {
        const int32_t cj = J.indices[k];
        while (s < i1 && I.indices[s] < cj) ++s;
        const double dj = i2i_val(J.values, J.kind, k);
        if (s < i1 && I.indices[s] == cj) {
            const double di = i2i_val(I.values, I.kind, s);
            mx += di > dj ? di : dj;
        } else {
            mx += dj;
        }
    }
    int64_t k = j0;
    for (s = i0; s < i1; ++s) {
        const int32_t ci = I.indices[s];
        while (k < j1 && J.indices[k] < ci) ++k;
        if (!(k < j1 && J.indices[k] == ci)) mx += i2i_val(I.values, I.kind, s);
    }
    return mx;
}

__device__ __forceinline__ double spgemm_epilogue(const SpgemmEpilogue &e, int64_t r, int64_t c, double s) {
    if (e.kind == PK_SPGEMM_EPI_JACCARD) return s / ((e.nf_cols[c] + e.nf_rows[r]) - s);
    if (e.kind == PK_SPGEMM_EPI_WJACCARD) {
        if (e.wj_rect) return s / spgemm_wj_max_sum(e.cols, c, e.rows, r);
        const int64_t i = r < c ? r : c, j = r < c ? c : r;
        return s / spgemm_wj_max_sum(e.cols, i, e.cols, j);
    }
    return s;
}

__device__ __forceinline__ bool spgemm_stored(const uint64_t *acc, int slot, int64_t w0, int64_t n_cols, int64_t r, int diag,
                                              double *a) {
    const int64_t col = w0 + slot;
    *a = __longlong_as_double((long long)acc[slot]);
    return col < n_cols && (*a != 0.0 || (diag && col == r));
}

template <int OP>
__global__ __launch_bounds__(PK_I2I_THREADS) void spgemm_count_kernel(
    int64_t n_inner, int64_t n_cols, const int64_t *__restrict__ l_indptr, const int32_t *__restrict__ l_indices,
    const void *__restrict__ l_values, int l_kind, const int64_t *__restrict__ b_indptr, const int32_t *__restrict__ b_indices,
    const double *__restrict__ b_values, int diag, int32_t *__restrict__ counts) {
    __shared__ uint64_t acc[PK_I2I_WIN];
    __shared__ uint32_t seen[PK_I2I_WIN / 32];
    const int64_t r = blockIdx.x, w0 = (int64_t)blockIdx.y * PK_I2I_WIN;
    const bool touched = spsp_accumulate<OP>(r, w0, n_inner, l_indptr, l_indices, l_values, l_kind, b_indptr, b_indices, b_values,
                                             0, acc, seen);
    const int any = __syncthreads_or(touched);
    const int64_t cell = r * gridDim.y + blockIdx.y;
    if (!any) {                              // nothing of this row falls into the window: at most its diagonal entry
        if (threadIdx.x == 0) counts[cell] = (diag && r >= w0 && r < w0 + PK_I2I_WIN && r < n_cols) ? 1 : 0;
        return;
    }
    int n = 0;
    for (int round = 0; round < PK_SPGEMM_ROUNDS; ++round) {
        double a;
        n += __syncthreads_count(spgemm_stored(acc, round * PK_I2I_THREADS + threadIdx.x, w0, n_cols, r, diag, &a));
    }
    if (threadIdx.x == 0) counts[cell] = n;
}

template <int OP>
__global__ __launch_bounds__(PK_I2I_THREADS) void spgemm_fill_kernel(
    int64_t n_inner, int64_t n_cols, const int64_t *__restrict__ l_indptr, const int32_t *__restrict__ l_indices,
    const void *__restrict__ l_values, int l_kind, const int64_t *__restrict__ b_indptr, const int32_t *__restrict__ b_indices,
    const double *__restrict__ b_values, int diag, SpgemmEpilogue epi, const int64_t *__restrict__ offsets, int64_t capacity,
    int32_t *__restrict__ out_indices, double *__restrict__ out_values) {
    __shared__ uint64_t acc[PK_I2I_WIN];
    __shared__ uint32_t seen[PK_I2I_WIN / 32];
    __shared__ int wcnt[PK_I2I_THREADS / 64];
    const int64_t r = blockIdx.x, w0 = (int64_t)blockIdx.y * PK_I2I_WIN;
    const bool touched = spsp_accumulate<OP>(r, w0, n_inner, l_indptr, l_indices, l_values, l_kind, b_indptr, b_indices, b_values,
                                             0, acc, seen);
    const int any = __syncthreads_or(touched);
    const int64_t cell = r * gridDim.y + blockIdx.y;
    int64_t base = offsets[cell];
    int64_t end = offsets[cell + 1];         // the count pass saw the same window: a guard, not a rule
    if (end > capacity) end = capacity;
    if (!any) {
        if (threadIdx.x == 0 && diag && r >= w0 && r < w0 + PK_I2I_WIN && r < n_cols && base < end) {
            out_indices[base] = (int32_t)r;
            out_values[base] = 1.0;
        }
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int round = 0; round < PK_SPGEMM_ROUNDS; ++round) {
        const int slot = round * PK_I2I_THREADS + threadIdx.x;
        double a;
        const bool st = spgemm_stored(acc, slot, w0, n_cols, r, diag, &a);
        const uint64_t mask = __ballot(st);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < PK_I2I_THREADS / 64; ++w) {
            const int c = wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (st) {
            const int64_t pos = base + before + __popcll(mask & ((1ull << lane) - 1));
            const int64_t col = w0 + slot;
            if (pos < end) {
                out_indices[pos] = (int32_t)col;
                out_values[pos] = (diag && col == r) ? 1.0 : spgemm_epilogue(epi, r, col, a);
            }
        }
        base += total;
        __syncthreads();
    }
}

static int64_t spgemm_align(int64_t b) { return (b + 255) / 256 * 256; }

extern "C" int64_t pk_spgemm_work_bytes(int64_t n_rows, int64_t n_cols) {
    if (n_rows < 0 || n_cols < 1) return -1;
    const int64_t cells = n_rows * pk_ceil_div(n_cols, PK_I2I_WIN);
    return spgemm_align(cells * 4) + spgemm_align((cells + 1) * 8) + spgemm_align(pk_scan_work_bytes(cells)) + 256;
}

static int spgemm_check(const char *who, int64_t n_rows, int64_t n_inner, int64_t n_cols, const void *l_indptr, const void *b_indptr,
                        int l_val_kind, int op, int diag, const void *work) {
    PK_REQUIRE(n_rows >= 0 && n_inner >= 1 && n_cols >= 1 && n_cols <= (int64_t)PK_I2I_ITEM_MASK,
               "%s: bad shape (n_rows %lld, n_inner %lld, n_cols %lld: n_inner >= 1, 1 <= n_cols < 2^30)", who, (long long)n_rows,
               (long long)n_inner, (long long)n_cols);
    PK_REQUIRE(l_val_kind == PK_VAL_F32 || l_val_kind == PK_VAL_F64, "%s: bad value kind", who);
    PK_REQUIRE(op == PK_SPGEMM_OP_MUL || op == PK_SPGEMM_OP_MIN, "%s: unknown op %d", who, op);
    PK_REQUIRE(diag == 0 || (diag == 1 && n_rows == n_cols), "%s: diag = 1 needs a square product (got %lld x %lld)", who,
               (long long)n_rows, (long long)n_cols);
    PK_REQUIRE(l_indptr && b_indptr && work, "%s: null pointer", who);
    PK_REQUIRE(pk_ceil_div(n_cols, PK_I2I_WIN) <= 65535 && n_rows <= 0x7fffffff, "%s: too many rows or columns for the grid", who);
    return PK_OK;
}

__global__ void spgemm_indptr_kernel(int64_t n_rows, int64_t n_win, const int64_t *__restrict__ offsets,
                                     int64_t *__restrict__ indptr) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= n_rows) indptr[r] = offsets[r * n_win];
}

extern "C" int pk_spgemm_count(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                               const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                               const int32_t *b_indices_dev, const double *b_values_dev, int32_t op, int32_t diag,
                               int64_t *indptr_out_dev, void *work_dev) {
    const int rc = spgemm_check("pk_spgemm_count", n_rows, n_inner, n_cols, l_indptr_dev, b_indptr_dev, l_val_kind, op, diag, work_dev);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(indptr_out_dev, "pk_spgemm_count: null pointer");
    hipStream_t s = pk_stream(stream);
    const int64_t n_win = pk_ceil_div(n_cols, PK_I2I_WIN), cells = n_rows * n_win;
    int32_t *counts = static_cast<int32_t *>(work_dev);
    int64_t *offsets = reinterpret_cast<int64_t *>(static_cast<char *>(work_dev) + spgemm_align(cells * 4));
    void *swork = reinterpret_cast<char *>(offsets) + spgemm_align((cells + 1) * 8);
    if (n_rows > 0) {
        const dim3 grid((unsigned)n_rows, (unsigned)n_win), block(PK_I2I_THREADS);
        if (op == PK_SPGEMM_OP_MIN)
            hipLaunchKernelGGL(spgemm_count_kernel<PK_SPGEMM_OP_MIN>, grid, block, 0, s, n_inner, n_cols, l_indptr_dev, l_indices_dev,
                               l_values_dev, l_val_kind, b_indptr_dev, b_indices_dev, b_values_dev, (int)diag, counts);
        else
            hipLaunchKernelGGL(spgemm_count_kernel<PK_SPGEMM_OP_MUL>, grid, block, 0, s, n_inner, n_cols, l_indptr_dev, l_indices_dev,
                               l_values_dev, l_val_kind, b_indptr_dev, b_indices_dev, b_values_dev, (int)diag, counts);
        PK_CHECK_LAUNCH("spgemm_count_kernel");
    }
    const int src = pk_exclusive_scan_i32(stream, cells, counts, offsets, swork);
    if (src != PK_OK) return src;
    hipLaunchKernelGGL(spgemm_indptr_kernel, dim3((unsigned)pk_ceil_div(n_rows + 1, 256)), dim3(256), 0, s, n_rows, n_win, offsets,
                       indptr_out_dev);
    PK_CHECK_LAUNCH("spgemm_indptr_kernel");
    return PK_OK;
}

extern "C" int pk_spgemm_fill(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                              const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                              const int32_t *b_indices_dev, const double *b_values_dev, int32_t op, int32_t diag, int32_t epilogue,
                              int32_t wj_rect, const double *nf_rows_dev, const double *nf_cols_dev, const int64_t *f_indptr_dev,
                              const int32_t *f_indices_dev, const double *f_values_dev, const void *work_dev, int64_t nnz,
                              int32_t *out_indices_dev, double *out_values_dev) {
    const int rc = spgemm_check("pk_spgemm_fill", n_rows, n_inner, n_cols, l_indptr_dev, b_indptr_dev, l_val_kind, op, diag, work_dev);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(epilogue == PK_SPGEMM_EPI_NONE || epilogue == PK_SPGEMM_EPI_JACCARD || epilogue == PK_SPGEMM_EPI_WJACCARD,
               "pk_spgemm_fill: unknown epilogue %d", (int)epilogue);
    PK_REQUIRE(epilogue != PK_SPGEMM_EPI_JACCARD || (nf_rows_dev && nf_cols_dev),
               "pk_spgemm_fill: the Jaccard epilogue needs the entry counts of both sides");
    PK_REQUIRE(epilogue != PK_SPGEMM_EPI_WJACCARD || (op == PK_SPGEMM_OP_MIN && f_indptr_dev && f_indices_dev && f_values_dev),
               "pk_spgemm_fill: the weighted Jaccard epilogue needs op = MIN and the column side's features by item");
    PK_REQUIRE(epilogue != PK_SPGEMM_EPI_WJACCARD || wj_rect == 1 || (wj_rect == 0 && n_rows == n_cols),
               "pk_spgemm_fill: the symmetric weighted Jaccard epilogue needs a square product");
    PK_REQUIRE(nnz >= 0 && (nnz == 0 || (out_indices_dev && out_values_dev)), "pk_spgemm_fill: bad output arrays (nnz %lld)",
               (long long)nnz);
    if (n_rows == 0 || nnz == 0) return PK_OK;
    const int64_t n_win = pk_ceil_div(n_cols, PK_I2I_WIN), cells = n_rows * n_win;
    const int64_t *offsets = reinterpret_cast<const int64_t *>(static_cast<const char *>(work_dev) + spgemm_align(cells * 4));
    SpgemmEpilogue epi;
    epi.kind = epilogue;
    epi.wj_rect = wj_rect;
    epi.nf_rows = nf_rows_dev;
    epi.nf_cols = nf_cols_dev;
    epi.rows = SpgemmRows{l_indptr_dev, l_indices_dev, l_values_dev, l_val_kind};
    epi.cols = SpgemmRows{f_indptr_dev, f_indices_dev, f_values_dev, PK_VAL_F64};
    const dim3 grid((unsigned)n_rows, (unsigned)n_win), block(PK_I2I_THREADS);
    hipStream_t s = pk_stream(stream);
    if (op == PK_SPGEMM_OP_MIN)
        hipLaunchKernelGGL(spgemm_fill_kernel<PK_SPGEMM_OP_MIN>, grid, block, 0, s, n_inner, n_cols, l_indptr_dev, l_indices_dev,
                           l_values_dev, l_val_kind, b_indptr_dev, b_indices_dev, b_values_dev, (int)diag, epi, offsets, nnz,
                           out_indices_dev, out_values_dev);
    else
        hipLaunchKernelGGL(spgemm_fill_kernel<PK_SPGEMM_OP_MUL>, grid, block, 0, s, n_inner, n_cols, l_indptr_dev, l_indices_dev,
                           l_values_dev, l_val_kind, b_indptr_dev, b_indices_dev, b_values_dev, (int)diag, epi, offsets, nnz,
                           out_indices_dev, out_values_dev);
    PK_CHECK_LAUNCH("spgemm_fill_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_spgemm() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&spgemm_fill_kernel<PK_SPGEMM_OP_MUL>));
}
