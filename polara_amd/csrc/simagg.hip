// Row-wise sparse x sparse product with the per-row top-k fused in: the hot path of SimilarityAggregation (hybrid/models.py:25-44,
// s_u = sum_i t_ui S[., i]) and of SimilarityAggregationItemColdStart (coldstart/models.py:101-119, s_c = sum_i sim[c, i] A[., i]).
//
//   scores[r, :] = sum_p L.values[p] * B[L.indices[p], :]      L: CSR [n_rows x n_inner], B: canonical CSR [n_inner x n_cols], fp64
//
// Numerical contract: for every (r, column) the products are added in ascending order of p, starting from +0.0, each one a
// separately rounded fp64 multiply and add (spsp_mul_add) — no contraction, no atomics, no order that depends on scheduling —
// and a -0 result is stored as +0.  That is the order of SciPy's csr_matmat, so the scores are bit-equal to SciPy's product
// and the lists are a function of the inputs alone.
//
//   * workgroup (r, w) of 256 threads covers the PK_I2I_WIN = 2048 columns of window w with 2048 fp64 accumulators in LDS
//     (16 KiB, the array that later holds the keys).  Each of the four waves owns a fixed 512-column quarter: two waves
//     never touch the same accumulator, so the accumulation needs no barrier;
//   * a wave takes the left row 64 entries at a time: lane l loads entry p + l as (i, v) and binary-searches B's row i for
//     the part [lo, hi) inside its quarter; a ballot gives the non-empty entries, the wave walks only those in ascending p
//     (lo, hi and v broadcast with readlane) and its lanes stride the segment doing the LDS read-modify-write — the columns
//     of one B row are distinct, so no two lanes collide, and a wave's LDS operations execute in program order;
//   * every LDS write is guarded by (unsigned)(col - c0) < 512: non-canonical input may give wrong sums, never a write
//     outside the array; an inner index outside [0, n_inner) is skipped;
//   * one __syncthreads, then the epilogue: the keys of i2i.hip formed in place, its LDS bitonic sort, the best pow2(topk)
//     of the window to the candidate buffer and i2i_merge_kernel for the lists (pk_spsp_topk), or the window written to a
//     dense fp64 block (pk_spsp_rows_f64).
#include "spsp_accum.h"                      // spsp_mul_add, spsp_accumulate: shared with spgemm.hip

extern "C" int64_t pk_spsp_topk_work_bytes(int64_t n_rows, int64_t n_cols, int32_t topk) {
    return pk_i2i_topk_work_bytes(n_rows, n_cols, topk);
}

// SEEN: the seen set of row r is row r of the pattern CSR (s_indptr, s_indices) over the columns (pk_spsp_topk_seen) instead
// of the left row's own inner indices (pk_spsp_topk, where n_inner == n_cols)
template <bool SEEN>
__global__ __launch_bounds__(PK_I2I_THREADS) void spsp_window_kernel(
    int64_t r0, int64_t n_inner, int64_t n_cols, const int64_t *__restrict__ l_indptr, const int32_t *__restrict__ l_indices,
    const void *__restrict__ l_values, int l_kind, const int64_t *__restrict__ b_indptr, const int32_t *__restrict__ b_indices,
    const double *__restrict__ b_values, const int64_t *__restrict__ s_indptr, const int32_t *__restrict__ s_indices, int P,
    int filter_seen, int sparse, uint64_t *__restrict__ cand_s, uint32_t *__restrict__ cand_m) {
    __shared__ uint64_t ks[PK_I2I_WIN];
    __shared__ uint32_t km[PK_I2I_WIN];
    __shared__ uint32_t seen[PK_I2I_WIN / 32];
    const int64_t w0 = (int64_t)blockIdx.y * PK_I2I_WIN;
    const bool touched = spsp_accumulate(r0 + blockIdx.x, w0, n_inner, l_indptr, l_indices, l_values, l_kind, b_indptr, b_indices,
                                         b_values, SEEN ? 0 : filter_seen, ks, seen);
    const int any = __syncthreads_or(touched);
    const int64_t base = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * P;
    if (sparse && !any) {                    // no candidate in this window: pad keys, no sort
        for (int k = threadIdx.x; k < P; k += PK_I2I_THREADS) {
            cand_s[base + k] = 0;
            cand_m[base + k] = PK_I2I_ITEM_MASK;
        }
        return;
    }
    if (SEEN && filter_seen) {               // the bitmap is zero (spsp_accumulate): the row's seen columns of this window
        const int64_t r = r0 + blockIdx.x, p1 = s_indptr[r + 1];
        const int64_t lo = i2i_lower_bound(s_indices, s_indptr[r], p1, w0);
        const int64_t hi = i2i_lower_bound(s_indices, lo, p1, w0 + PK_I2I_WIN);
        for (int64_t k = lo + threadIdx.x; k < hi; k += PK_I2I_THREADS) {
            const uint32_t d = (uint32_t)((int64_t)s_indices[k] - w0);
            if (d < PK_I2I_WIN) atomicOr(&seen[d >> 5], 1u << (d & 31));
        }
        __syncthreads();
    }
    for (int slot = threadIdx.x; slot < PK_I2I_WIN; slot += PK_I2I_THREADS) {
        const int64_t col = w0 + slot;
        const double a = __longlong_as_double((long long)ks[slot]);
        const double s = a == 0.0 ? 0.0 : a;                    // -0 -> +0
        const bool sn = filter_seen && ((seen[slot >> 5] >> (slot & 31)) & 1u);
        uint32_t cls;
        if (col >= n_cols)
            cls = 0;
        else if (sparse)
            cls = (s != 0.0 && !sn) ? 2 : 0;
        else
            cls = sn ? 1 : 2;
        ks[slot] = cls ? i2i_key(s) : 0;
        km[slot] = cls ? ((cls << 30) | (uint32_t)col) : PK_I2I_ITEM_MASK;
    }
    __syncthreads();
    i2i_sort<PK_I2I_THREADS>(ks, km, PK_I2I_WIN);
    for (int k = threadIdx.x; k < P; k += PK_I2I_THREADS) {
        cand_s[base + k] = ks[k];
        cand_m[base + k] = km[k];
    }
}

__global__ __launch_bounds__(PK_I2I_THREADS) void spsp_rows_kernel(
    int64_t r0, int64_t n_inner, int64_t n_cols, const int64_t *__restrict__ l_indptr, const int32_t *__restrict__ l_indices,
    const void *__restrict__ l_values, int l_kind, const int64_t *__restrict__ b_indptr, const int32_t *__restrict__ b_indices,
    const double *__restrict__ b_values, double *__restrict__ out, int64_t ld) {
    __shared__ uint64_t acc[PK_I2I_WIN];
    __shared__ uint32_t seen[PK_I2I_WIN / 32];
    const int64_t w0 = (int64_t)blockIdx.y * PK_I2I_WIN;
    spsp_accumulate(r0 + blockIdx.x, w0, n_inner, l_indptr, l_indices, l_values, l_kind, b_indptr, b_indices, b_values, 0, acc,
                    seen);
    __syncthreads();
    double *row = out + (int64_t)blockIdx.x * ld;
    for (int slot = threadIdx.x; slot < PK_I2I_WIN; slot += PK_I2I_THREADS) {
        const int64_t col = w0 + slot;
        const double a = __longlong_as_double((long long)acc[slot]);
        if (col < n_cols) row[col] = a == 0.0 ? 0.0 : a;
    }
}

static int spsp_check(const char *who, int64_t n_rows, int64_t n_inner, int64_t n_cols, const void *l_indptr, const void *b_indptr,
                      int l_val_kind) {
    PK_REQUIRE(n_rows >= 0 && n_inner >= 1 && n_cols >= 1 && n_cols <= (int64_t)PK_I2I_ITEM_MASK,
               "%s: bad shape (n_rows %lld, n_inner %lld, n_cols %lld: n_inner >= 1, 1 <= n_cols < 2^30)", who, (long long)n_rows,
               (long long)n_inner, (long long)n_cols);
    PK_REQUIRE(l_val_kind == PK_VAL_F32 || l_val_kind == PK_VAL_F64, "%s: bad value kind", who);
    PK_REQUIRE(l_indptr && b_indptr, "%s: null pointer", who);
    PK_REQUIRE(pk_ceil_div(n_cols, PK_I2I_WIN) <= 65535, "%s: too many columns for the grid", who);
    return PK_OK;
}

static int spsp_topk_launch(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols,
                            const int64_t *l_indptr_dev, const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind,
                            const int64_t *b_indptr_dev, const int32_t *b_indices_dev, const double *b_values_dev,
                            const int64_t *s_indptr_dev, const int32_t *s_indices_dev, int32_t topk, int32_t filter_seen,
                            int32_t sparse, int64_t *out_idx_dev, double *out_scores_dev, void *work_dev) {
    const int64_t n_win = pk_ceil_div(n_cols, PK_I2I_WIN);
    const int P = i2i_pow2(topk);
    const int64_t chunk = pk_i2i_chunk_users(n_rows, n_cols, topk);
    uint64_t *cand_s = static_cast<uint64_t *>(work_dev);
    uint32_t *cand_m = reinterpret_cast<uint32_t *>(cand_s + chunk * n_win * P);
    hipStream_t s = pk_stream(stream);
    auto kernel = s_indptr_dev ? spsp_window_kernel<true> : spsp_window_kernel<false>;
    for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
        const int64_t nr = n_rows - r0 < chunk ? n_rows - r0 : chunk;
        hipLaunchKernelGGL(kernel, dim3((unsigned)nr, (unsigned)n_win), dim3(PK_I2I_THREADS), 0, s, r0, n_inner, n_cols,
                           l_indptr_dev, l_indices_dev, l_values_dev, l_val_kind, b_indptr_dev, b_indices_dev, b_values_dev,
                           s_indptr_dev, s_indices_dev, P, (int)filter_seen, (int)sparse, cand_s, cand_m);
        PK_CHECK_LAUNCH("spsp_window_kernel");
        i2i_launch_merge(s, nr, r0, (int)n_win, P, (int)topk, cand_s, cand_m, out_idx_dev, out_scores_dev);
        PK_CHECK_LAUNCH("i2i_merge_kernel");
    }
    return PK_OK;
}

extern "C" int pk_spsp_topk(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                            const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                            const int32_t *b_indices_dev, const double *b_values_dev, int32_t topk, int32_t filter_seen,
                            int32_t sparse, int64_t *out_idx_dev, double *out_scores_dev, void *work_dev) {
    PK_REQUIRE(topk >= 1 && topk <= PK_I2I_MAX_TOPK, "pk_spsp_topk: topk %d outside 1..%d", (int)topk, PK_I2I_MAX_TOPK);
    PK_REQUIRE(!filter_seen || n_inner == n_cols,
               "pk_spsp_topk: filter_seen marks the left row's own columns, which needs n_inner == n_cols (got %lld and %lld)",
               (long long)n_inner, (long long)n_cols);
    const int rc = spsp_check("pk_spsp_topk", n_rows, n_inner, n_cols, l_indptr_dev, b_indptr_dev, l_val_kind);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(out_idx_dev && work_dev, "pk_spsp_topk: null pointer");
    if (n_rows == 0) return PK_OK;
    return spsp_topk_launch(stream, n_rows, n_inner, n_cols, l_indptr_dev, l_indices_dev, l_values_dev, l_val_kind,
                            b_indptr_dev, b_indices_dev, b_values_dev, nullptr, nullptr, topk, filter_seen, sparse, out_idx_dev,
                            out_scores_dev, work_dev);
}

extern "C" int pk_spsp_topk_seen(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                                 const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind,
                                 const int64_t *b_indptr_dev, const int32_t *b_indices_dev, const double *b_values_dev,
                                 const int64_t *seen_indptr_dev, const int32_t *seen_indices_dev, int32_t topk,
                                 int32_t filter_seen, int32_t sparse, int64_t *out_idx_dev, double *out_scores_dev,
                                 void *work_dev) {
    PK_REQUIRE(topk >= 1 && topk <= PK_I2I_MAX_TOPK, "pk_spsp_topk_seen: topk %d outside 1..%d", (int)topk, PK_I2I_MAX_TOPK);
    const int rc = spsp_check("pk_spsp_topk_seen", n_rows, n_inner, n_cols, l_indptr_dev, b_indptr_dev, l_val_kind);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(out_idx_dev && work_dev && seen_indptr_dev, "pk_spsp_topk_seen: null pointer");
    if (n_rows == 0) return PK_OK;
    return spsp_topk_launch(stream, n_rows, n_inner, n_cols, l_indptr_dev, l_indices_dev, l_values_dev,
                            l_val_kind, b_indptr_dev, b_indices_dev, b_values_dev, seen_indptr_dev, seen_indices_dev, topk,
                            filter_seen, sparse, out_idx_dev, out_scores_dev, work_dev);
}

extern "C" int pk_spsp_rows_f64(void *stream, int64_t row0, int64_t n_rows, int64_t n_inner, int64_t n_cols,
                                const int64_t *l_indptr_dev, const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind,
                                const int64_t *b_indptr_dev, const int32_t *b_indices_dev, const double *b_values_dev,
                                double *out_dev, int64_t ld) {
    const int rc = spsp_check("pk_spsp_rows_f64", n_rows, n_inner, n_cols, l_indptr_dev, b_indptr_dev, l_val_kind);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(row0 >= 0 && out_dev && ld >= n_cols, "pk_spsp_rows_f64: bad arguments (row0 %lld, ld %lld < n_cols %lld?)",
               (long long)row0, (long long)ld, (long long)n_cols);
    if (n_rows == 0) return PK_OK;
    PK_REQUIRE(n_rows <= 0x7fffffff, "pk_spsp_rows_f64: too many rows for the grid");
    hipLaunchKernelGGL(spsp_rows_kernel, dim3((unsigned)n_rows, (unsigned)pk_ceil_div(n_cols, PK_I2I_WIN)), dim3(PK_I2I_THREADS), 0,
                       pk_stream(stream), row0, n_inner, n_cols, l_indptr_dev, l_indices_dev, l_values_dev, l_val_kind, b_indptr_dev,
                       b_indices_dev, b_values_dev, out_dev, ld);
    PK_CHECK_LAUNCH("spsp_rows_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_simagg() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&spsp_window_kernel<false>));
}
