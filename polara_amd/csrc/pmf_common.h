// What the blocked SGD sweeps of pmf.hip and kpmf.hip share: the arguments of a stratum launch, the halving tree of the dot,
// the gradient adjusters and the launch of the squared error's reduction (defined once, in pmf.hip).
#pragma once
#include "pk_common.h"

#define PMF_MAX_RANK 64
#define PMF_THREADS 64              // one wave per workgroup: a block's sweep is a chain of dependent loads, so the waves of
                                    // a stratum are spread over as many SIMDs as there are

struct PmfArgs {
    int B, rank;
    const int64_t *block_ptr;
    const int32_t *users, *items;
    const double *vals;
    double *P, *Q;
    int64_t ldp, ldq;
    const double *rnnz, *cnnz;
    double eta, lambd;
    double *SP, *SQ;
    int64_t ldsp, ldsq;
    double gamma, one_minus_gamma, smoothing;
    double *block_sse;
};

// the halving tree of polara_hip.h on a xor butterfly: every lane of the group ends with the same bits (a + b == b + a)
template <int W>
__device__ __forceinline__ double pmf_group_sum(double v) {
    if constexpr (W >= 64) v = v + pk_lane_xor<32>(v);
    if constexpr (W >= 32) v = v + pk_lane_xor<16>(v);
    v = v + pk_lane_xor<8>(v);
    v = v + pk_lane_xor<4>(v);
    v = v + pk_lane_xor<2>(v);
    v = v + pk_lane_xor<1>(v);
    return v;
}

// (both sweeps switch contraction off for their whole translation unit before they include this)
template <int ADJ>
__device__ __forceinline__ double pmf_adjust(double g, double &s, const PmfArgs &a) {
    if constexpr (ADJ == PK_PMF_ADJUST_NONE) {
        return g;
    } else {
        double u;
        if constexpr (ADJ == PK_PMF_ADJUST_ADAGRAD)
            u = s + g * g;
        else
            u = a.gamma * s + a.one_minus_gamma * (g * g);
        s = u;
        return g / sqrt(a.smoothing + u);
    }
}

// block sums -> stratum sums (block order) -> the epoch's sum (stratum order): pmf_sse_kernel of pmf.hip on `st`
void pmf_launch_sse(hipStream_t st, int blocks, const double *block_sse_dev, double *sse_dev);
