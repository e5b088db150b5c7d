// Neighbourhood and random-walk item models (ItemKNN, P3alpha / RP3beta): the pass between the dense Gram image and the
// sparse weights — normalise every entry of a row, keep its K best, write them in ascending column order
// (include/polara_hip.h has the contract).
//
//   * One workgroup of 256 threads per row of the image.  The row is streamed in windows of PK_I2I_WIN = 2048 columns, 8
//     consecutive columns per lane (four 16-byte loads of G, four of the column vector): the image is read once, in whole
//     lines.  A lane forms w and the key (class, w, column) of its 8 columns, the window's keys are bitonic-sorted in LDS
//     and its best P = pow2(K) are merged into the row's running list by one bitonic merge of 2 P keys — the keys, the
//     sort and the compare-exchange of the scoring pass (i2i_keys.h).
//   * A window in which no candidate beats the last entry of the running list leaves the list as it is: it costs one
//     block-wide vote and no sort.  The empty stretches of a sparse Gram row go this way, and later windows once the list
//     holds better entries (on dense rows nearly every window still enters: DESIGN.md 8s has the measurement).
//   * The kept prefix of the list is re-sorted by column (the same sort, key = column), gathered into registers, summed by
//     ONE thread in ascending column order when `normalize` asks for it, and written with its pads.
//   * No atomics, no cross-workgroup traffic, one launch: the result is a function of the inputs alone.
//   * No contraction: every product, sum, difference and quotient is rounded on its own; fp64 division is the correctly
//     rounded one (no fast-math flag in the build).
#include "i2i_keys.h"
#include "knn_weight.h"                    // knn_weight: shared with uknn.hip
#include <float.h>

#pragma clang fp contract(off)

#define KNN_SLOTS (PK_I2I_MAX_TOPK / PK_I2I_THREADS)      // output slots of a thread

extern "C" int32_t pk_knn_max_neighbours(void) { return PK_I2I_MAX_TOPK; }

__device__ __forceinline__ void knn_load8(const double *__restrict__ p, double *c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double2 a = reinterpret_cast<const double2 *>(p)[k];
        c[2 * k] = a.x, c[2 * k + 1] = a.y;
    }
}

// VEC: ldg % 8 == 0 and G, col 16-byte aligned — a lane whose 8 columns are all below n loads them as double2
template <bool VEC>
__global__ __launch_bounds__(PK_I2I_THREADS) void knn_prune_kernel(int64_t n, const double *__restrict__ G, int64_t ldg, int kind,
                                                                   const double *__restrict__ row, const double *__restrict__ col,
                                                                   double shrink, int K, int P, int normalize,
                                                                   int32_t *__restrict__ count, int32_t *__restrict__ idx,
                                                                   double *__restrict__ val) {
    __shared__ uint64_t ks[PK_I2I_WIN];
    __shared__ uint32_t km[PK_I2I_WIN];
    __shared__ uint64_t bs[2 * PK_I2I_MAX_TOPK];
    __shared__ uint32_t bm[2 * PK_I2I_MAX_TOPK];
    __shared__ double s_sum;
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const double *g_row = G + i * ldg;
    const double ri = row[i];
    for (int k = tid; k < 2 * P; k += PK_I2I_THREADS) {
        bs[k] = 0;
        bm[k] = PK_I2I_ITEM_MASK;             // class 0: a pad
    }
    __syncthreads();

    for (int64_t w0 = 0; w0 < n; w0 += PK_I2I_WIN) {
        const int64_t col0 = w0 + (int64_t)tid * PK_I2I_COLS;
        double g[PK_I2I_COLS], c[PK_I2I_COLS];
        if (VEC && col0 + PK_I2I_COLS <= n) {
            knn_load8(g_row + col0, g);
            knn_load8(col + col0, c);
        } else {
#pragma unroll
            for (int j = 0; j < PK_I2I_COLS; ++j) {
                const bool in = col0 + j < n;
                g[j] = in ? g_row[col0 + j] : 0.0;
                c[j] = in ? col[col0 + j] : 0.0;
            }
        }
        const uint64_t last_s = bs[P - 1];    // the running list's last entry: what a candidate must beat to enter
        const uint32_t last_m = bm[P - 1];
        int any = 0;
#pragma unroll
        for (int j = 0; j < PK_I2I_COLS; ++j) {
            const int64_t cj = col0 + j;
            const double w = knn_weight(kind, g[j], ri, c[j], shrink);
            const bool cand = cj < n && cj != i && g[j] != 0.0 && fabs(w) <= DBL_MAX && w != 0.0;
            const uint64_t s = i2i_key(w);
            const uint32_t m = (2u << 30) | (uint32_t)cj;
            const bool enters = cand && i2i_better(s, m, last_s, last_m);
            const int slot = tid * PK_I2I_COLS + j;
            ks[slot] = enters ? s : 0;
            km[slot] = enters ? m : PK_I2I_ITEM_MASK;
            any |= enters;
        }
        if (!__syncthreads_or(any)) continue;           // uniform: nothing of this window enters the list
        i2i_sort<PK_I2I_THREADS>(ks, km, PK_I2I_WIN);
        // the window's best P reversed behind the running best P: a bitonic sequence of 2 P keys
        for (int k = tid; k < P; k += PK_I2I_THREADS) {
            bs[2 * P - 1 - k] = ks[k];
            bm[2 * P - 1 - k] = km[k];
        }
        __syncthreads();
        for (int j = P; j > 0; j >>= 1) {
            for (int t = tid; t < P; t += PK_I2I_THREADS) {
                const int a = i2i_pair(t, j);
                i2i_cmpx(bs, bm, a, a + j);
            }
            __syncthreads();
        }
    }

    // the kept entries: the candidates among the first K of the list (candidates come before pads: a prefix)
    int c = 0;
    for (int base = 0; base < K; base += PK_I2I_THREADS) {
        const int t = base + tid;
        c += __syncthreads_count(t < K && (bm[t] >> 30) != 0);
    }
    // ascending column: the same sort with the column as the key, the list position as the payload
    for (int t = tid; t < P; t += PK_I2I_THREADS) {
        const bool kept = t < c;
        ks[t] = kept ? (uint64_t)(PK_I2I_ITEM_MASK - (bm[t] & PK_I2I_ITEM_MASK)) : 0;
        km[t] = kept ? ((2u << 30) | (uint32_t)t) : PK_I2I_ITEM_MASK;
    }
    __syncthreads();
    i2i_sort<PK_I2I_THREADS>(ks, km, P);
    int32_t oj[KNN_SLOTS];
    double ow[KNN_SLOTS];
#pragma unroll
    for (int q = 0; q < KNN_SLOTS; ++q) {
        const int r = tid + q * PK_I2I_THREADS;
        oj[q] = -1;
        ow[q] = 0.0;
        if (r < c) {
            oj[q] = (int32_t)(PK_I2I_ITEM_MASK - (uint32_t)ks[r]);
            ow[q] = i2i_unkey(bs[km[r] & PK_I2I_ITEM_MASK]);
        }
    }
    if (normalize) {
        __syncthreads();                                // every thread has read its entries of bs
#pragma unroll
        for (int q = 0; q < KNN_SLOTS; ++q) {
            const int r = tid + q * PK_I2I_THREADS;
            if (r < c) bs[r] = (uint64_t)__double_as_longlong(fabs(ow[q]));
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int r = 0; r < c; ++r) s = s + __longlong_as_double((long long)bs[r]);
            s_sum = s;
        }
        __syncthreads();
        const double s = s_sum;
        if (fabs(s) <= DBL_MAX && s != 0.0) {
#pragma unroll
            for (int q = 0; q < KNN_SLOTS; ++q) ow[q] = ow[q] / s;      // pads: 0 / s = 0
        }
    }
#pragma unroll
    for (int q = 0; q < KNN_SLOTS; ++q) {
        const int r = tid + q * PK_I2I_THREADS;
        if (r < K) {
            idx[i * K + r] = oj[q];
            val[i * K + r] = r < c ? ow[q] : 0.0;
        }
    }
    if (tid == 0) count[i] = c;
}

extern "C" int pk_knn_prune_f64(void *stream, int64_t n, const double *G_dev, int64_t ldg, int32_t kind, const double *row_dev,
                                const double *col_dev, double shrink, int32_t K, int32_t normalize, int32_t *count_dev,
                                int32_t *idx_dev, double *val_dev) {
    PK_REQUIRE(n >= 1 && n <= (int64_t)PK_I2I_ITEM_MASK, "pk_knn_prune_f64: n = %lld outside 1 <= n < 2^30", (long long)n);
    PK_REQUIRE(ldg >= n, "pk_knn_prune_f64: ldg = %lld is below n = %lld", (long long)ldg, (long long)n);
    PK_REQUIRE(kind == PK_KNN_SCALE || kind == PK_KNN_COSINE || kind == PK_KNN_TANIMOTO, "pk_knn_prune_f64: unknown kind %d",
               (int)kind);
    PK_REQUIRE(K >= 1 && K <= PK_I2I_MAX_TOPK, "pk_knn_prune_f64: K = %d outside 1..%d (pk_knn_max_neighbours)", (int)K,
               PK_I2I_MAX_TOPK);
    PK_REQUIRE(shrink >= 0.0 && shrink <= DBL_MAX, "pk_knn_prune_f64: shrink must be finite and >= 0, got %g", shrink);
    PK_REQUIRE(G_dev && row_dev && col_dev && count_dev && idx_dev && val_dev, "pk_knn_prune_f64: null pointer");
    const bool vec = ldg % PK_I2I_COLS == 0 && reinterpret_cast<uintptr_t>(G_dev) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(col_dev) % 16 == 0;
    const int P = i2i_pow2(K);
    if (vec)
        hipLaunchKernelGGL(knn_prune_kernel<true>, dim3((unsigned)n), dim3(PK_I2I_THREADS), 0, pk_stream(stream), n, G_dev, ldg,
                           (int)kind, row_dev, col_dev, shrink, (int)K, P, (int)normalize, count_dev, idx_dev, val_dev);
    else
        hipLaunchKernelGGL(knn_prune_kernel<false>, dim3((unsigned)n), dim3(PK_I2I_THREADS), 0, pk_stream(stream), n, G_dev, ldg,
                           (int)kind, row_dev, col_dev, shrink, (int)K, P, (int)normalize, count_dev, idx_dev, val_dev);
    PK_CHECK_LAUNCH("knn_prune_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_knn() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&knn_prune_kernel<true>));
}
