// The sigmoid of the pairwise and logistic solvers (bpr.hip, lmf.hip), once: IEEE operations only, the same sequence as
// tests/bpr_reference.py (the specification is the BPR comment of include/polara_hip.h).
//
// Include this AFTER `#pragma clang fp contract(off)`: every product and sum below is rounded on its own.
//
// sigm(x) = 1 / (1 + exp(x)).  With a = -|x| (cut at PK_SIGMOID_EXP_MIN, below which exp(a) is under half the smallest subnormal):
// n = floor(a * log2(e) + 1/2), r = (a - n * LN2_HI) - n * LN2_LO (|r| <= 0.35; n * LN2_HI is exact), e = ldexp(T13(r), n)
// with T13 the Taylor polynomial of degree 13 in Horner form; sigm = 1 / (1 + e) for x <= 0, e / (1 + e) for x > 0.
#pragma once
#include "pk_common.h"

#define PK_SIGMOID_EXP_MIN (-750.0)
#define PK_SIGMOID_LOG2E 0x1.71547652b82fep+0
#define PK_SIGMOID_LN2_HI 0x1.62e42fee00000p-1
#define PK_SIGMOID_LN2_LO 0x1.a39ef35793c76p-33
__device__ __forceinline__ double pk_sigmoid(double x) {
    const bool pos = x > 0.0;
    double a = pos ? -x : x;
    a = a < PK_SIGMOID_EXP_MIN ? PK_SIGMOID_EXP_MIN : a;          // a NaN passes through every comparison
    const double n = floor(a * PK_SIGMOID_LOG2E + 0.5);
    const double r = (a - n * PK_SIGMOID_LN2_HI) - n * PK_SIGMOID_LN2_LO;
    double p = 0x1.6124613a86d09p-33;                             // 1 / 13!
    p = p * r + 0x1.1eed8eff8d898p-29;                            // 1 / 12!
    p = p * r + 0x1.ae64567f544e4p-26;                            // 1 / 11!
    p = p * r + 0x1.27e4fb7789f5cp-22;                            // 1 / 10!
    p = p * r + 0x1.71de3a556c734p-19;                            // 1 / 9!
    p = p * r + 0x1.a01a01a01a01ap-16;                            // 1 / 8!
    p = p * r + 0x1.a01a01a01a01ap-13;                            // 1 / 7!
    p = p * r + 0x1.6c16c16c16c17p-10;                            // 1 / 6!
    p = p * r + 0x1.1111111111111p-7;                             // 1 / 5!
    p = p * r + 0x1.5555555555555p-5;                             // 1 / 4!
    p = p * r + 0x1.5555555555555p-3;                             // 1 / 3!
    p = p * r + 0x1.0000000000000p-1;                             // 1 / 2!
    p = p * r + 1.0;
    p = p * r + 1.0;
    const double e = ldexp(p, n == n ? (int)n : 0);               // |n| <= 1083
    return (pos ? e : 1.0) / (1.0 + e);
}
