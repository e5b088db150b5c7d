// The total order of the item-to-item family (i2i.hip, simagg.hip): the limits of a scoring window, the key of a column
// (class, score, item), the LDS bitonic sort of a window's keys, and the launch of the kernel that merges the windows of a
// row into its list (the kernel itself lives in i2i.hip).
#pragma once
#include "pk_common.h"

#define PK_I2I_COLS 8                // columns of a scoring lane
#define PK_I2I_THREADS 256
#define PK_I2I_WIN (PK_I2I_COLS * PK_I2I_THREADS)   // 2048 columns per scoring workgroup
#define PK_I2I_MAX_TOPK 1024
#define PK_I2I_CAND_BUDGET (512ll << 20)           // bytes of window candidates per launch (users are chunked under it)
#define PK_I2I_ITEM_MASK 0x3fffffffu

static inline int32_t i2i_pow2(int32_t topk) {
    int32_t p = 1;
    while (p < topk) p <<= 1;
    return p;
}

// ---- keys ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t i2i_key(double s) {
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double i2i_unkey(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}
// a strictly better than b under (class desc, score desc, item asc); m = class << 30 | item
__device__ __forceinline__ bool i2i_better(uint64_t sa, uint32_t ma, uint64_t sb, uint32_t mb) {
    const uint32_t ca = ma >> 30, cb = mb >> 30;
    if (ca != cb) return ca > cb;
    if (sa != sb) return sa > sb;
    return (ma & PK_I2I_ITEM_MASK) < (mb & PK_I2I_ITEM_MASK);
}
__device__ __forceinline__ void i2i_cmpx(uint64_t *s, uint32_t *m, int i, int l) {
    if (i2i_better(s[l], m[l], s[i], m[i])) {
        const uint64_t ts = s[i];
        const uint32_t tm = m[i];
        s[i] = s[l];
        m[i] = m[l];
        s[l] = ts;
        m[l] = tm;
    }
}
// pair t of a compare distance j: (i, i + j) with bit j of i clear
__device__ __forceinline__ int i2i_pair(int t, int j) { return 2 * t - (t & (j - 1)); }

// best-first bitonic sort of n (power of two) keys in LDS by the block's NT threads
template <int NT>
__device__ void i2i_sort(uint64_t *s, uint32_t *m, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += NT) {
                const int i = i2i_pair(t, j);
                if ((i & k) == 0)
                    i2i_cmpx(s, m, i, i + j);
                else
                    i2i_cmpx(s, m, i + j, i);
            }
            __syncthreads();
        }
}

// ---- sparse rows ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double i2i_val(const void *v, int kind, int64_t p) {
    return kind == PK_VAL_F32 ? (double)static_cast<const float *>(v)[p] : static_cast<const double *>(v)[p];
}

// first position in [lo, hi) whose column is >= c
__device__ __forceinline__ int64_t i2i_lower_bound(const int32_t *__restrict__ idx, int64_t lo, int64_t hi, int64_t c) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// one wave per row: the best P keys of each of the n_win windows of rows [u0, u0 + nu) merged into out_idx / out_scores
// (i2i_merge_kernel, i2i.hip); hipGetLastError() tells whether the launch went through
void i2i_launch_merge(hipStream_t s, int64_t nu, int64_t u0, int n_win, int P, int topk, const uint64_t *cand_s,
                      const uint32_t *cand_m, int64_t *out_idx, double *out_scores);
