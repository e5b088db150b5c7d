// What the candidate sweep (score.hip) and the re-scoring kernel (rescore.hip) share: the error bound of the sweep's
// product, the settle rule's arithmetic, its flag value and the segment sort both run it on — ONE definition each.
#pragma once
#include "pk_common.h"
#include <math.h>

#define PK_IDX_NONE 0x7fffffff

__device__ __forceinline__ bool pk_before64(double ka, int va, double kb, int vb) {
    return (ka > kb) || (ka == kb && va < vb);
}

// bitonic sort (descending by pk_before64) inside aligned segments of SEG lanes, one (key, val) per lane
// LPC: lanes per element (the LPC adjacent lanes of a candidate hold identical copies and perform identical
// exchanges, so the network runs on all lanes with partners LPC * J lanes away)
// pay...: 32-bit values that travel with their element (none: the re-scoring kernel; the item's norm: the sweep's exit)
template <int SEG, int K, int J, int LPC, typename... P>
__device__ __forceinline__ void pk_bitonic_seg_merge(double &key, int &val, int t, P &...pay) {
    const double ok = pk_lane_xor<J * LPC>(key);
    const int ov = pk_lane_xor<J * LPC>(val);
    const bool lower = (t & J) == 0;
    const bool desc = (t & K) == 0;   // t < SEG: the last level (K == SEG) is descending everywhere
    const bool want_first = (lower == desc);
    const bool other_first = pk_before64(ok, ov, key, val);
    const bool take = (want_first == other_first);
    // (the exchange itself runs on ALL lanes, like the key's and the value's above: a lane exchange evaluated only where
    // `take` holds — the lazy arm of a ?: — reads zeros through the lanes that sit the branch out, J = 4 is two DPP steps)
    auto swap_in = [take](auto &p) {
        const auto other = pk_lane_xor<J * LPC>(p);
        p = take ? other : p;
    };
    (swap_in(pay), ...);
    if (take) {
        key = ok;
        val = ov;
    }
    if constexpr (J > 1) pk_bitonic_seg_merge<SEG, K, (J >> 1), LPC>(key, val, t, pay...);
}
template <int SEG, int K, int LPC, typename... P>
__device__ __forceinline__ void pk_bitonic_seg_levels(double &key, int &val, int t, P &...pay) {
    if constexpr (K > 2) pk_bitonic_seg_levels<SEG, (K >> 1), LPC>(key, val, t, pay...);
    pk_bitonic_seg_merge<SEG, K, (K >> 1), LPC>(key, val, t, pay...);
}
template <int SEG, int LPC, typename... P>
__device__ __forceinline__ void pk_bitonic_seg(double &key, int &val, int t, P &...pay) {
    pk_bitonic_seg_levels<SEG, SEG, LPC>(key, val, t, pay...);
}

// The sweep's split-bf16 product (score.hip): |s32 - e.v| <= pk_sweep_err_coeff(K) |e||v| — operands split into two bf16
// each, the lo.lo term dropped, fp32 conversion of the inputs, accumulation roundings.  ONE definition: the certification
// against the sweep's threshold and the settle rule (below) both stand on it.
__device__ __forceinline__ double pk_sweep_err_coeff(int K) {
    return 3.0 * 1.52587890625e-05 + (double)(4 * K + 10) * 1.1920928955078125e-07;
}

// flags[u] of a user the settle rule finished (rescore_topk_kernel's tier, or the sweep's exit): above the mask 7 of the
// lists of users to re-do, so nobody re-does them — the bit only lets a caller COUNT them afterwards
#define PK_FLAG_SETTLED 8

// The settle rule's per-user and per-item error terms: every sweep score of user u is within d_i = c_u n_i of the exact
// score of the same item, c_u = B N_u + 2^-24 w_u (N_u >= ||E'_u||: the users' side of the sweep's pruning bound,
// w_u: the approximate fold-in's error weight), n_i = the item's norm bound capped by the catalogue's largest.
__device__ __forceinline__ double pk_settle_coeff(int K, float user_norm, double w) {
    return pk_sweep_err_coeff(K) * (double)user_norm + w * 5.9604644775390625e-08 * (1.0 + 1e-6);
}
__device__ __forceinline__ double pk_settle_item_err(double c, double vmax, float item_norm) {
    return c * fmin(vmax, (double)item_norm * (1.0 + 1e-6));
}
// the bound on the sweep score of an item the sweep left out: its lists are ordered by keys that drop low bits (2^-15 covers it)
__device__ __forceinline__ double pk_settle_tau_cert(double tau32) { return tau32 + fabs(tau32) * 3.0517578125e-05; }
