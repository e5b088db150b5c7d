// Neighbour pass without a Gram image (UserKNN; ItemKNN / RP3beta with gram = 'sparse'): a row of L B is formed from the
// sparse operands, normalised, and its K best are written as n_rows x K slots (include/polara_hip.h has the contract;
// DESIGN.md 8u).  It joins three pinned pieces:
//
//   * workgroup (r, w) accumulates window w (PK_I2I_WIN = 2048 columns) of row r in LDS with spsp_accumulate (spsp_accum.h:
//     the sums of pk_spsp_topk, SciPy's order);
//   * its epilogue forms w = knn_weight(g, row[r], col[c], shrink) and the key (class 2 = candidate, 0 = not) of every
//     column in place, sorts the window's keys (i2i_sort) and writes the best P = pow2(K) to the candidate buffer; a window
//     the accumulation did not touch holds no g != 0, so it writes pad keys and sorts nothing;
//   * i2i_merge_kernel merges a row's windows into its K best, best first (i2i.hip);
//   * uknn_finish_kernel, one workgroup per row, orders the winners by column (the same sort, key = column), sums their
//     absolute values with ONE thread in ascending column when `normalize` asks for it, and writes count, idx, val and pads.
//
// Rows are chunked under PK_I2I_CAND_BUDGET like pk_spsp_topk.  The (row, window) grid was chosen over one streaming
// workgroup per row (knn.hip) because a sparse row of the product touches few windows: the untouched ones leave after
// one block-wide vote, and at n_cols of 10^5 a streaming workgroup would walk 70 windows in sequence where the grid runs
// them side by side.  No atomics on results, no cross-workgroup ordering: equal inputs give equal bits.
#include "spsp_accum.h"
#include "knn_weight.h"
#include <float.h>

static inline int64_t uknn_align8(int64_t x) { return (x + 7) & ~(int64_t)7; }

// candidate keys of a chunk (u64 scores, then u32 class|column), then the chunk's merged lists: int64 idx, fp64 w
extern "C" int64_t pk_spsp_knn_work_bytes(int64_t n_rows, int64_t n_cols, int32_t K) {
    const int64_t chunk = pk_i2i_chunk_users(n_rows, n_cols, K);
    if (chunk <= 0) return 0;
    return uknn_align8(pk_i2i_topk_work_bytes(n_rows, n_cols, K)) + chunk * (int64_t)K * 16;
}

__global__ __launch_bounds__(PK_I2I_THREADS) void uknn_window_kernel(
    int64_t r0, int64_t n_inner, int64_t n_cols, const int64_t *__restrict__ l_indptr, const int32_t *__restrict__ l_indices,
    const void *__restrict__ l_values, int l_kind, const int64_t *__restrict__ b_indptr, const int32_t *__restrict__ b_indices,
    const double *__restrict__ b_values, int kind, const double *__restrict__ row, const double *__restrict__ colv, double shrink,
    const int32_t *__restrict__ exclude, int P, uint64_t *__restrict__ cand_s, uint32_t *__restrict__ cand_m) {
    __shared__ uint64_t ks[PK_I2I_WIN];
    __shared__ uint32_t km[PK_I2I_WIN];
    __shared__ uint32_t seen[PK_I2I_WIN / 32];
    const int64_t r = r0 + blockIdx.x;
    const int64_t w0 = (int64_t)blockIdx.y * PK_I2I_WIN;
    const bool touched =
        spsp_accumulate(r, w0, n_inner, l_indptr, l_indices, l_values, l_kind, b_indptr, b_indices, b_values, 0, ks, seen);
    const int any = __syncthreads_or(touched);
    const int64_t base = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * P;
    if (!any) {                              // every g of this window is +0: no candidate, pad keys, no sort
        for (int k = threadIdx.x; k < P; k += PK_I2I_THREADS) {
            cand_s[base + k] = 0;
            cand_m[base + k] = PK_I2I_ITEM_MASK;
        }
        return;
    }
    const double ri = row[r];
    const int64_t ex = exclude ? (int64_t)exclude[r] : -1;      // a negative entry excludes nothing
    for (int slot = threadIdx.x; slot < PK_I2I_WIN; slot += PK_I2I_THREADS) {
        const int64_t c = w0 + slot;
        const double a = __longlong_as_double((long long)ks[slot]);
        const double g = a == 0.0 ? 0.0 : a;                    // -0 -> +0
        bool cand = false;
        double w = 0.0;
        if (c < n_cols) {
            w = knn_weight(kind, g, ri, colv[c], shrink);
            cand = c != ex && g != 0.0 && fabs(w) <= DBL_MAX && w != 0.0;
        }
        ks[slot] = cand ? i2i_key(w) : 0;
        km[slot] = cand ? ((2u << 30) | (uint32_t)c) : PK_I2I_ITEM_MASK;
    }
    __syncthreads();
    i2i_sort<PK_I2I_THREADS>(ks, km, PK_I2I_WIN);
    for (int k = threadIdx.x; k < P; k += PK_I2I_THREADS) {
        cand_s[base + k] = ks[k];
        cand_m[base + k] = km[k];
    }
}

// one workgroup per row: the row's merged list (best first, pads idx -1 behind the candidates) in ascending column order
__global__ __launch_bounds__(PK_I2I_THREADS) void uknn_finish_kernel(int64_t r0, int K, int P, int normalize,
                                                                     const int64_t *__restrict__ top_idx,
                                                                     const double *__restrict__ top_w,
                                                                     int32_t *__restrict__ count, int32_t *__restrict__ idx,
                                                                     double *__restrict__ val) {
    __shared__ uint64_t ks[PK_I2I_MAX_TOPK];
    __shared__ uint32_t km[PK_I2I_MAX_TOPK];
    __shared__ double sw[PK_I2I_MAX_TOPK];
    __shared__ double s_sum;
    const int tid = threadIdx.x;
    const int64_t *ti = top_idx + (int64_t)blockIdx.x * K;
    const double *tw = top_w + (int64_t)blockIdx.x * K;
    const int64_t r = r0 + blockIdx.x;
    int c = 0;
    for (int t0 = 0; t0 < P; t0 += PK_I2I_THREADS) {
        const int t = t0 + tid;
        const bool kept = t < K && ti[t] >= 0;
        if (t < P) {
            ks[t] = kept ? (uint64_t)(PK_I2I_ITEM_MASK - (uint32_t)ti[t]) : 0;
            km[t] = kept ? ((2u << 30) | (uint32_t)t) : PK_I2I_ITEM_MASK;
        }
        c += __syncthreads_count(kept);
    }
    i2i_sort<PK_I2I_THREADS>(ks, km, P);
    for (int t = tid; t < c; t += PK_I2I_THREADS) sw[t] = tw[km[t] & PK_I2I_ITEM_MASK];
    __syncthreads();
    double s = 0.0;
    if (normalize) {
        if (tid == 0) {
            double a = 0.0;
            for (int t = 0; t < c; ++t) a = a + fabs(sw[t]);
            s_sum = a;
        }
        __syncthreads();
        s = s_sum;
    }
    const bool scale = normalize && fabs(s) <= DBL_MAX && s != 0.0;
    for (int t = tid; t < K; t += PK_I2I_THREADS) {
        const bool kept = t < c;
        idx[r * K + t] = kept ? (int32_t)(PK_I2I_ITEM_MASK - (uint32_t)ks[t]) : -1;
        val[r * K + t] = kept ? (scale ? sw[t] / s : sw[t]) : 0.0;
    }
    if (tid == 0) count[r] = c;
}

extern "C" int pk_spsp_knn_f64(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                               const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind,
                               const int64_t *b_indptr_dev, const int32_t *b_indices_dev, const double *b_values_dev, int32_t kind,
                               const double *row_dev, const double *col_dev, double shrink, const int32_t *exclude_dev, int32_t K,
                               int32_t normalize, int32_t *count_dev, int32_t *idx_dev, double *val_dev, void *work_dev) {
    PK_REQUIRE(n_rows >= 0 && n_inner >= 1 && n_cols >= 1 && n_cols <= (int64_t)PK_I2I_ITEM_MASK,
               "pk_spsp_knn_f64: bad shape (n_rows %lld, n_inner %lld, n_cols %lld: n_inner >= 1, 1 <= n_cols < 2^30)",
               (long long)n_rows, (long long)n_inner, (long long)n_cols);
    PK_REQUIRE(l_val_kind == PK_VAL_F32 || l_val_kind == PK_VAL_F64, "pk_spsp_knn_f64: bad value kind %d", (int)l_val_kind);
    PK_REQUIRE(kind == PK_KNN_SCALE || kind == PK_KNN_COSINE || kind == PK_KNN_TANIMOTO, "pk_spsp_knn_f64: unknown kind %d",
               (int)kind);
    PK_REQUIRE(K >= 1 && K <= PK_I2I_MAX_TOPK, "pk_spsp_knn_f64: K = %d outside 1..%d (pk_knn_max_neighbours)", (int)K,
               PK_I2I_MAX_TOPK);
    PK_REQUIRE(shrink >= 0.0 && shrink <= DBL_MAX, "pk_spsp_knn_f64: shrink must be finite and >= 0, got %g", shrink);
    PK_REQUIRE(pk_ceil_div(n_cols, PK_I2I_WIN) <= 65535, "pk_spsp_knn_f64: too many columns for the grid");
    PK_REQUIRE(l_indptr_dev && b_indptr_dev && row_dev && col_dev && count_dev && idx_dev && val_dev && work_dev,
               "pk_spsp_knn_f64: null pointer");
    if (n_rows == 0) return PK_OK;
    const int64_t n_win = pk_ceil_div(n_cols, PK_I2I_WIN);
    const int P = i2i_pow2(K);
    const int64_t chunk = pk_i2i_chunk_users(n_rows, n_cols, K);
    uint64_t *cand_s = static_cast<uint64_t *>(work_dev);
    uint32_t *cand_m = reinterpret_cast<uint32_t *>(cand_s + chunk * n_win * P);
    int64_t *top_idx = reinterpret_cast<int64_t *>(static_cast<char *>(work_dev) +
                                                   uknn_align8(pk_i2i_topk_work_bytes(n_rows, n_cols, K)));
    double *top_w = reinterpret_cast<double *>(top_idx + chunk * K);
    hipStream_t s = pk_stream(stream);
    for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
        const int64_t nr = n_rows - r0 < chunk ? n_rows - r0 : chunk;
        hipLaunchKernelGGL(uknn_window_kernel, dim3((unsigned)nr, (unsigned)n_win), dim3(PK_I2I_THREADS), 0, s, r0, n_inner, n_cols,
                           l_indptr_dev, l_indices_dev, l_values_dev, l_val_kind, b_indptr_dev, b_indices_dev, b_values_dev,
                           (int)kind, row_dev, col_dev, shrink, exclude_dev, P, cand_s, cand_m);
        PK_CHECK_LAUNCH("uknn_window_kernel");
        i2i_launch_merge(s, nr, 0, (int)n_win, P, (int)K, cand_s, cand_m, top_idx, top_w);      // chunk-local lists
        PK_CHECK_LAUNCH("i2i_merge_kernel");
        hipLaunchKernelGGL(uknn_finish_kernel, dim3((unsigned)nr), dim3(PK_I2I_THREADS), 0, s, r0, (int)K, P, (int)normalize,
                           top_idx, top_w, count_dev, idx_dev, val_dev);
        PK_CHECK_LAUNCH("uknn_finish_kernel");
    }
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_uknn() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&uknn_window_kernel));
}
