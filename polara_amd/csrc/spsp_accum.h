// The accumulation of one window of a row-wise sparse x sparse product in LDS, shared by simagg.hip (top-k / dense rows) and
// spgemm.hip (CSR output).  See simagg.hip for the layout (four waves, one 512-column quarter each, no barrier) and the
// numerical contract (ascending order of the left row's entries from +0.0, separately rounded multiply and add).
#pragma once
#include "i2i_keys.h"

#define PK_SPSP_QUARTER (PK_I2I_WIN / 4)     // columns of a wave

// the accumulation `op` is PK_SPGEMM_OP_MUL (acc + v * b, SciPy's product) or PK_SPGEMM_OP_MIN (acc + min(v, b)): polara_hip.h

// acc + v * b as a separately rounded multiply and add.  (HIP's __dmul_rn / __dadd_rn are the plain operators: under the
// compiler's default -ffp-contract=fast they fuse into v_fmac_f64, whose sums differ from SciPy's in the last bit.  With
// contraction switched off for this function the two instructions carry no `contract` flag and stay apart.)
__device__ __forceinline__ double spsp_mul_add(double acc, double v, double b) {
#pragma clang fp contract(off)
    const double prod = v * b;
    return acc + prod;
}

__device__ __forceinline__ double spsp_min_add(double acc, double v, double b) { return acc + (b < v ? b : v); }

__device__ __forceinline__ int64_t spsp_readlane(int64_t x, int lane) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)x, lane), hi = __builtin_amdgcn_readlane((int)(x >> 32), lane);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// The accumulation of window w0 of left row r into acc (2048 doubles kept as their bit patterns) and, under filter_seen, the
// row's own stored columns of the window into the bitmap `seen` (64 words).  Returns whether this wave added anything.
template <int OP = PK_SPGEMM_OP_MUL>
__device__ __forceinline__ bool spsp_accumulate(int64_t r, int64_t w0, int64_t n_inner, const int64_t *__restrict__ l_indptr,
                                                const int32_t *__restrict__ l_indices, const void *__restrict__ l_values,
                                                int l_kind, const int64_t *__restrict__ b_indptr,
                                                const int32_t *__restrict__ b_indices, const double *__restrict__ b_values,
                                                int mark_seen, uint64_t *acc, uint32_t *seen) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint64_t *qacc = acc + wave * PK_SPSP_QUARTER;
    uint32_t *qseen = seen + wave * (PK_SPSP_QUARTER / 32);
    for (int c = lane; c < PK_SPSP_QUARTER; c += 64) qacc[c] = 0;           // the bits of +0.0
    if (lane < PK_SPSP_QUARTER / 32) qseen[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t c0 = w0 + wave * PK_SPSP_QUARTER, c1 = c0 + PK_SPSP_QUARTER;
    const int64_t p1 = l_indptr[r + 1];
    bool touched = false;
    for (int64_t p = l_indptr[r]; p < p1; p += 64) {
        const int64_t q = p + lane;
        int64_t lo = 0, hi = 0;
        double v = 0.0;
        if (q < p1) {
            const int64_t i = l_indices[q];
            if ((uint64_t)i < (uint64_t)n_inner) {
                v = i2i_val(l_values, l_kind, q);
                const int64_t b1 = b_indptr[i + 1];
                lo = i2i_lower_bound(b_indices, b_indptr[i], b1, c0);
                hi = i2i_lower_bound(b_indices, lo, b1, c1);
                const uint32_t d = (uint32_t)(i - c0);
                if (mark_seen && (uint64_t)(i - c0) < PK_SPSP_QUARTER) atomicOr(&qseen[d >> 5], 1u << (d & 31));
            }
        }
        uint64_t todo = __ballot(hi > lo);
        touched |= todo != 0;
        while (todo) {
            const int e = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int64_t slo = spsp_readlane(lo, e), shi = spsp_readlane(hi, e);
            const double sv = __longlong_as_double(spsp_readlane(__double_as_longlong(v), e));
            for (int64_t k = slo + lane; k < shi; k += 64) {
                const uint32_t d = (uint32_t)((int64_t)b_indices[k] - c0);
                if (d < PK_SPSP_QUARTER) {
                    const double a = __longlong_as_double((long long)qacc[d]);
                    if constexpr (OP == PK_SPGEMM_OP_MIN)
                        qacc[d] = (uint64_t)__double_as_longlong(spsp_min_add(a, sv, b_values[k]));
                    else
                        qacc[d] = (uint64_t)__double_as_longlong(spsp_mul_add(a, sv, b_values[k]));
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    return touched;
}
