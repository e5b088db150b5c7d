// The summation order of every exact fp64 score of the library: shared by the re-scoring and exact-row kernels (rescore.hip)
// and the contextual tier (context.hip), so that a (user, item) score has the same bits wherever it is computed.
#pragma once
#include "pk_common.h"

// ---- the ONE summation order of every exact fp64 score of the library ---------------------------------
// The K products are dealt to four chains by element PAIR: pair p = (2p, 2p+1) goes to chain p & 3, each
// chain is a serial fma chain in increasing p, and the total is (c0 + c2) + (c1 + c3).  A thread working
// alone (LPC = 1, and the exact-row kernel) keeps four accumulators; with LPC = 2 lane q owns chains q and
// q + 2; with LPC = 4 lane q owns chain {0, 2, 1, 3}[q], so that the lane^1 exchange forms (c0 + c2) and
// (c1 + c3) and the lane^2 exchange the total.  Whatever the lane layout — and whether a user goes
// through the re-scoring kernel or the exact-row kernel — a given (user, item) score has the same bits.
template <int LPC>
__device__ __forceinline__ double pk_dot_chains(const double *__restrict__ vr, const double *er, int K, int q,
                                                bool vvec2, bool evec2, double *e_norm2 = nullptr) {
    double n2 = 0.0;   // sum of squares of the e elements this lane touches (any order: only feeds a bound)
    constexpr int NLOC = 4 / LPC;
    double acc[NLOC];
#pragma unroll
    for (int j = 0; j < NLOC; ++j) acc[j] = 0.0;
    const int np = (K + 1) >> 1, nfull = K >> 1;
    const int start = (LPC == 4) ? (((q & 1) << 1) | (q >> 1)) : q;
    int p = start;
    // all NLOC pairs of an iteration are complete: no bounds tests, loads of the iteration issued together
    if (vvec2 && evec2) {
        const double2 *v2 = reinterpret_cast<const double2 *>(vr);
        const double2 *e2 = reinterpret_cast<const double2 *>(er);
#pragma unroll 2
        for (; p + (NLOC - 1) * LPC < nfull; p += 4) {
            double2 a[NLOC], e[NLOC];
#pragma unroll
            for (int j = 0; j < NLOC; ++j) {
                a[j] = v2[p + j * LPC];
                e[j] = e2[p + j * LPC];
            }
#pragma unroll
            for (int j = 0; j < NLOC; ++j) {
                acc[j] = fma(e[j].x, a[j].x, acc[j]);
                acc[j] = fma(e[j].y, a[j].y, acc[j]);
                n2 = fma(e[j].x, e[j].x, fma(e[j].y, e[j].y, n2));
            }
        }
    } else {
        for (; p + (NLOC - 1) * LPC < nfull; p += 4) {
#pragma unroll
            for (int j = 0; j < NLOC; ++j) {
                const int pj = p + j * LPC;
                const double e0 = er[2 * pj], e1 = er[2 * pj + 1];
                acc[j] = fma(e0, vr[2 * pj], acc[j]);
                acc[j] = fma(e1, vr[2 * pj + 1], acc[j]);
                n2 = fma(e0, e0, fma(e1, e1, n2));
            }
        }
    }
    // tail of the row (at most one iteration), incl. the half-filled last pair of an odd K
#pragma unroll
    for (int j = 0; j < NLOC; ++j) {
        const int pj = p + j * LPC;
        if (pj < nfull) {
            const double e0 = er[2 * pj], e1 = er[2 * pj + 1];
            acc[j] = fma(e0, vr[2 * pj], acc[j]);
            acc[j] = fma(e1, vr[2 * pj + 1], acc[j]);
            n2 = fma(e0, e0, fma(e1, e1, n2));
        } else if (pj < np) {
            const double e0 = er[2 * pj];
            acc[j] = fma(e0, vr[2 * pj], acc[j]);
            n2 = fma(e0, e0, n2);
        }
    }
    if (e_norm2) {
        if constexpr (LPC >= 2) n2 += pk_lane_xor<1>(n2);
        if constexpr (LPC >= 4) n2 += pk_lane_xor<2>(n2);
        *e_norm2 = n2;
    }
    double s;
    if constexpr (LPC == 1) s = (acc[0] + acc[2]) + (acc[1] + acc[3]);
    else if constexpr (LPC == 2) s = acc[0] + acc[1];
    else s = acc[0];
    if constexpr (LPC >= 2) s += pk_lane_xor<1>(s);
    if constexpr (LPC >= 4) s += pk_lane_xor<2>(s);
    return s;
}
