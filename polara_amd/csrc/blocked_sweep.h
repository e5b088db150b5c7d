// The skeleton of the blocked SGD sweeps (pmf.hip, kpmf.hip, bpr.hip, warp.hip), once: a lane group's block and the wave's
// longest one, the halving tree of the dot, the 16 / 32 / 64 width rule, the stratum loop of an epoch and the argument checks of
// its entry; what the two PMF sweeps share beyond that: the arguments of a stratum launch, the gradient adjusters, the body of a
// sample (pmf_stratum_kernel, with the kernelized pieces of kpmf.hip behind `if constexpr`) and the launch of the squared
// error's reduction (defined once, in pmf.hip); and what the two pairwise sweeps share: the block counters with the launch of
// their reduction (defined once, in bpr.hip) and the pieces of a draw inside an item part.
//
// Include this AFTER `#pragma clang fp contract(off)`: every sweep switches contraction off for its whole translation unit,
// and what is compiled from here must round every product and sum on its own too.
#pragma once
#include <type_traits>
#include "pk_common.h"

#define PMF_MAX_RANK 64
#define PMF_THREADS 64              // one wave per workgroup: a block's sweep is a chain of dependent loads, so the waves of
                                    // a stratum are spread over as many SIMDs as there are

// ---- the skeleton ---------------------------------------------------------------------------------------------------------
// W lanes per block, 64 / W blocks per wave: lane group g of workgroup x sweeps block b = x * G + g of the stratum (returned),
// lane c of the group holds column c.
template <int W>
__device__ __forceinline__ int64_t pk_sweep_lanes(int &c) {
    constexpr int G = 64 / W;
    const int lane = pk_lane();
    const int g = lane / W;
    c = lane % W;
    return (int64_t)blockIdx.x * G + g;
}

// Block b is positions t0 .. t0 + len of the schedule (none past the last block).  Returns the longest block of the wave,
// wave-uniform: the sweep's loop runs that far with every lane active, for the butterfly reads its neighbours.
template <int W>
__device__ __forceinline__ int64_t pk_sweep_range(int B, const int64_t *block_ptr, int stratum, int64_t b, int64_t &t0, int64_t &len) {
    t0 = 0, len = 0;
    if (b < B) {
        t0 = block_ptr[(int64_t)stratum * B + b];
        len = block_ptr[(int64_t)stratum * B + b + 1] - t0;
    }
    int64_t maxlen = len;
#pragma unroll
    for (int off = 32; off >= W; off >>= 1) {
        const int64_t o = __shfl_xor(maxlen, off, 64);
        maxlen = o > maxlen ? o : maxlen;
    }
    return ((int64_t)__builtin_amdgcn_readfirstlane((int)(maxlen >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(maxlen & 0xffffffffll));
}

// the halving tree of polara_hip.h on a xor butterfly: every lane of the group ends with the same bits (a + b == b + a)
template <int W>
__device__ __forceinline__ double group_sum(double v) {
    if constexpr (W >= 64) v = v + pk_lane_xor<32>(v);
    if constexpr (W >= 32) v = v + pk_lane_xor<16>(v);
    v = v + pk_lane_xor<8>(v);
    v = v + pk_lane_xor<4>(v);
    v = v + pk_lane_xor<2>(v);
    v = v + pk_lane_xor<1>(v);
    return v;
}

// lanes per block for rows of `cols` columns
static inline int pk_sweep_width(int cols) { return cols <= 16 ? 16 : cols <= 32 ? 32 : 64; }

// One epoch in stream order: for every stratum s, stratum(<W>, grid, s), then epilogue().  Both return PK_OK or the code of
// a failed launch (PK_CHECK_LAUNCH), which ends the epoch.
template <class Stratum, class Epilogue>
static int pk_sweep_epoch(int blocks, int cols, Stratum &&stratum, Epilogue &&epilogue) {
    const int w = pk_sweep_width(cols);
    const unsigned grid = (unsigned)pk_ceil_div(blocks, 64 / w);
    for (int s = 0; s < blocks; ++s) {
        const int rc = w == 16   ? stratum(std::integral_constant<int, 16>(), grid, s)
                       : w == 32 ? stratum(std::integral_constant<int, 32>(), grid, s)
                                 : stratum(std::integral_constant<int, 64>(), grid, s);
        if (rc != PK_OK) return rc;
    }
    return epilogue();
}

// The checks every sweep entry starts with, in their order and under the entry's name: the ranges of rank and blocks, `sizes`
// (the entry's own size checks; true where it has none), `pointers` (its own non-NULL pointers), `samples` (the schedule's
// arrays are there when nnz > 0; `what` names them), the leading dimensions of P and Q for `cols` columns, and the adjuster
// with its two state blocks.
static inline int pk_sweep_check(const char *entry, int blocks, int rank, int max_rank, int cols, bool sizes, bool pointers,
                                 bool samples, const char *what, int64_t ldp, int64_t ldq, int adjust = PK_PMF_ADJUST_NONE,
                                 const double *SP = nullptr, const double *SQ = nullptr, int64_t ldsp = 0, int64_t ldsq = 0) {
    PK_REQUIRE(rank >= 1 && rank <= max_rank, "%s: rank %d outside 1..%d", entry, rank, max_rank);
    PK_REQUIRE(blocks >= 1 && blocks <= PK_PMF_MAX_BLOCKS, "%s: %d blocks outside 1..%d", entry, blocks, PK_PMF_MAX_BLOCKS);
    PK_REQUIRE(sizes, "%s: bad sizes", entry);
    PK_REQUIRE(pointers, "%s: bad pointers", entry);
    PK_REQUIRE(samples, "%s: no %s given", entry, what);
    PK_REQUIRE(ldp >= cols && ldq >= cols, "%s: bad leading dimension%s", entry, cols == rank ? "" : " (rank + 1 columns)");
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || adjust == PK_PMF_ADJUST_ADAGRAD || adjust == PK_PMF_ADJUST_RMSPROP,
               "%s: unknown gradient adjustment %d", entry, adjust);
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || (SP && SQ && SP != SQ && ldsp >= rank && ldsq >= rank),
               "%s: the gradient adjustment needs its two state blocks", entry);
    return PK_OK;
}

// ---- the PMF sweeps -------------------------------------------------------------------------------------------------------
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

// one side's kernel matrix without its diagonal (canonical CSR), the diagonal, the parts of the schedule and the snapshot
struct KpmfSide {
    const int64_t *ptr;
    const int32_t *idx;
    const double *val, *diag;
    const int32_t *part;
    const double *snap;
    int64_t ldsnap;
};

struct KpmfArgs {
    PmfArgs pmf;
    KpmfSide u, i;
};

__device__ __forceinline__ const PmfArgs &pmf_args(const PmfArgs &a) { return a; }
__device__ __forceinline__ const PmfArgs &pmf_args(const KpmfArgs &ka) { return ka.pmf; }

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

// The sweep of one stratum, plain (Args = PmfArgs) or kernelized (Args = KpmfArgs: kpmf_neighbours of kpmf.hip).  A group past
// the end of its block computes on zeros and stores nothing.  Sample t + 1's rows are loaded while sample t is computed —
// unless they are sample t's own rows, whose new values then stay in registers.  Kernelized, block b holds user part b and
// item part (b + stratum) mod B; the user's neighbour sum is computed once per run of a user (the block writes no other user
// row meanwhile), the item's per sample.
template <int W, int ADJ, class Args>
__global__ __launch_bounds__(PMF_THREADS) void pmf_stratum_kernel(Args args, int stratum) {
    constexpr bool kernelized = std::is_same_v<Args, KpmfArgs>;
    const PmfArgs &a = pmf_args(args);
    int c;
    const int64_t b = pk_sweep_lanes<W>(c);
    const bool col = c < a.rank;
    int upart = 0, ipart = 0;
    if constexpr (kernelized) upart = (int)b, ipart = (int)((b + stratum) % a.B);
    int64_t t0, len;
    const int64_t maxlen = pk_sweep_range<W>(a.B, a.block_ptr, stratum, b, t0, len);

    auto sample = [&](int64_t t, int &m, int &n, double &v) {
        if (t < len) {
            m = a.users[t0 + t];
            n = a.items[t0 + t];
            v = a.vals[t0 + t];
        } else {
            m = -1;
            n = -1;
            v = 0.0;
        }
    };
    auto row = [&](const double *X, int64_t ld, int r) { return (r >= 0 && col) ? X[(int64_t)r * ld + c] : 0.0; };
    auto count = [&](const double *cnt, int r) { return r >= 0 ? cnt[r] : 1.0; };
    auto diag = [&](const double *d, int r) { return r >= 0 ? d[r] : 0.0; };

    int m0, n0, m1, n1, m2, n2;
    double v0, v1, v2;
    sample(0, m0, n0, v0);
    sample(1, m1, n1, v1);
    double p = row(a.P, a.ldp, m0), q = row(a.Q, a.ldq, n0);
    double sp = ADJ ? row(a.SP, a.ldsp, m0) : 0.0, sq = ADJ ? row(a.SQ, a.ldsq, n0) : 0.0;
    double rc0 = count(a.rnnz, m0), cc0 = count(a.cnnz, n0);
    double du0 = 0.0, di0 = 0.0, du1 = 0.0, di1 = 0.0;
    if constexpr (kernelized) du0 = diag(args.u.diag, m0), di0 = diag(args.i.diag, n0);
    double off_p = 0.0, sse = 0.0;
    bool first_of_run = true;
    for (int64_t t = 0; t < maxlen; ++t) {
        sample(t + 2, m2, n2, v2);
        const bool new_m = m1 != m0, new_n = n1 != n0;
        const double p_next = new_m ? row(a.P, a.ldp, m1) : 0.0, q_next = new_n ? row(a.Q, a.ldq, n1) : 0.0;
        const double sp_next = (ADJ && new_m) ? row(a.SP, a.ldsp, m1) : 0.0, sq_next = (ADJ && new_n) ? row(a.SQ, a.ldsq, n1) : 0.0;
        const double rc1 = count(a.rnnz, m1), cc1 = count(a.cnnz, n1);
        double off_q = 0.0;
        if constexpr (kernelized) {
            du1 = diag(args.u.diag, m1), di1 = diag(args.i.diag, n1);
            if (first_of_run) off_p = kpmf_neighbours(args.u, upart, a.P, a.ldp, m0, c, m0 >= 0 && col);
            off_q = kpmf_neighbours(args.i, ipart, a.Q, a.ldq, n0, c, n0 >= 0 && col);
        }

        const double dot = group_sum<W>(p * q);
        const double err = v0 - dot;
        const double row_lambda = a.lambd / rc0, col_lambda = a.lambd / cc0;
        const double kp = kernelized ? off_p + du0 * (p + p) : p;
        const double kq = kernelized ? off_q + di0 * (q + q) : q;
        const double gp = err * q - kp * row_lambda;
        const double gq = err * p - kq * col_lambda;
        const double ap = pmf_adjust<ADJ>(gp, sp, a);
        const double p_new = p + a.eta * ap;
        const double aq = pmf_adjust<ADJ>(gq, sq, a);
        const double q_new = q + a.eta * aq;
        if (m0 >= 0) {
            if (col) {
                a.P[(int64_t)m0 * a.ldp + c] = p_new;
                a.Q[(int64_t)n0 * a.ldq + c] = q_new;
                if constexpr (ADJ != PK_PMF_ADJUST_NONE) {
                    a.SP[(int64_t)m0 * a.ldsp + c] = sp;
                    a.SQ[(int64_t)n0 * a.ldsq + c] = sq;
                }
            }
            sse = sse + err * err;
        }
        p = new_m ? p_next : p_new;
        q = new_n ? q_next : q_new;
        if constexpr (ADJ != PK_PMF_ADJUST_NONE) {
            sp = new_m ? sp_next : sp;
            sq = new_n ? sq_next : sq;
        }
        first_of_run = new_m;
        m0 = m1, n0 = n1, v0 = v1, rc0 = rc1, cc0 = cc1, du0 = du1, di0 = di1;
        m1 = m2, n1 = n2, v1 = v2;
    }
    if (b < a.B && c == 0) a.block_sse[(int64_t)stratum * a.B + b] = sse;
}

// the instance of pmf_stratum_kernel for the adjuster code, on `st`; `name` is the kernel's name in a launch error
template <int W, class Args>
static int pmf_launch(hipStream_t st, int adjust, unsigned grid, const Args &a, int stratum, const char *name) {
    if (adjust == PK_PMF_ADJUST_NONE)
        hipLaunchKernelGGL((pmf_stratum_kernel<W, PK_PMF_ADJUST_NONE, Args>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else if (adjust == PK_PMF_ADJUST_ADAGRAD)
        hipLaunchKernelGGL((pmf_stratum_kernel<W, PK_PMF_ADJUST_ADAGRAD, Args>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else
        hipLaunchKernelGGL((pmf_stratum_kernel<W, PK_PMF_ADJUST_RMSPROP, Args>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    PK_CHECK_LAUNCH(name);
    return PK_OK;
}

// block sums -> stratum sums (block order) -> the epoch's sum (stratum order): pmf_sse_kernel of pmf.hip on `st`, checked
int pmf_launch_sse(hipStream_t st, int blocks, const double *block_sse_dev, double *sse_dev);

// ---- the pairwise sweeps (bpr.hip, warp.hip) --------------------------------------------------------------------------------
// A sample is a stored positive and items drawn inside the positive's own item part.  Shared: the three counters every block
// keeps and their reduction, and the pieces of a draw.  Each model's draw kernel keeps its own thread mapping, its own counter
// stride per position and its own treatment of the answer.

// bytes of an epoch's work buffer: the [3][B * B] counters of every block
static inline int64_t pair_work_bytes(int32_t blocks) {
    const int64_t b = blocks < 1 ? 1 : blocks;
    return 3 * b * b * (int64_t)sizeof(int64_t);
}

// (A block's three stores into that buffer stay spelled out at the end of each stratum kernel: behind a helper the compiler
// orders them differently, and the kernels' instruction streams are kept equal to what was measured.)

// block counts -> stratum counts (block order) -> the epoch's three counts (stratum order): pair_counts_kernel of bpr.hip on
// `st`, checked
int pair_launch_counts(hipStream_t st, int blocks, const int64_t *block_counts_dev, int64_t *counts_dev);

// the key of an epoch's draw stream: mix64(seed * 2^32 + epoch)
static inline uint64_t pair_stream_key(uint32_t seed, uint32_t epoch) { return pk_mix64(((uint64_t)seed << 32) + (uint64_t)epoch); }

// the item the 32-bit draw w picks among the n_c items of the part that starts at item_order[lo_c]
__device__ __forceinline__ int32_t pair_draw_in_part(const int32_t *item_order, int64_t lo_c, uint64_t n_c, uint64_t w) {
    return item_order[lo_c + (int64_t)((w * n_c) >> 32)];
}

// whether the sorted row indices[r0 .. r1) holds item j: its lower bound
__device__ __forceinline__ bool pair_row_holds(const int32_t *indices, int64_t r0, int64_t r1, int32_t j) {
    int64_t lo = r0, hi = r1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (indices[mid] < j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < r1 && indices[lo] == j;
}

// The checks both draw entries make, in their order and under the entry's name; `draws` per position between the blocks and the
// pointers (BPR's are fixed, WARP's are its max_sampled).  `parts`: the plan's and the matrix's pointers, `samples`: the arrays
// that are there when nnz > 0.
static inline int pair_draw_check(const char *entry, int64_t nnz, int64_t n_users, int64_t n_items, int blocks, int draws,
                                  int max_draws, bool parts, bool samples) {
    PK_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31) && n_users >= 1 && n_items >= 1 && n_items < ((int64_t)1 << 31), "%s: bad sizes",
               entry);
    PK_REQUIRE(blocks >= 1 && blocks <= PK_PMF_MAX_BLOCKS, "%s: %d blocks outside 1..%d", entry, blocks, PK_PMF_MAX_BLOCKS);
    PK_REQUIRE(draws >= 1 && draws <= max_draws, "%s: max_sampled %d outside 1..%d", entry, draws, max_draws);
    PK_REQUIRE(parts, "%s: bad pointers", entry);
    PK_REQUIRE(samples, "%s: no interactions given", entry);
    return PK_OK;
}
