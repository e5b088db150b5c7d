// The normalised weight of one Gram entry, shared by the pruning pass of the dense image (knn.hip) and the sparse
// neighbour pass (uknn.hip): the three formulas of include/polara_hip.h, every product, sum, difference and quotient
// rounded on its own (contraction is switched off inside the function, so it holds wherever it is inlined).
#pragma once
#include "pk_common.h"

__device__ __forceinline__ double knn_weight(int kind, double g, double ri, double cj, double shrink) {
#pragma clang fp contract(off)
    if (kind == PK_KNN_SCALE) {
        const double a = g * ri;
        return a * cj;
    }
    if (kind == PK_KNN_COSINE) {
        const double p = ri * cj;
        const double d = p + shrink;
        return g / d;
    }
    const double s = ri + cj;
    const double t = s - g;
    const double d = t + shrink;
    return g / d;
}
