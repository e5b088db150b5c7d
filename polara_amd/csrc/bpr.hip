// Bayesian personalised ranking (LearnBPR, Rendle et al. 2009, in the shape the `implicit` package trains it: rank k plus an
// item bias) on the conflict-free blocked schedule of PMF (polara_amd/bpr.py: block_schedule with the epoch's item order).
// A sample touches one user row and TWO item rows — the positive's and the negative's — so the negative of a positive is drawn
// inside the positive's own item part: the blocks of one stratum then share no row at all, and one launch sweeps them side by
// side, each block sequentially by one lane group.  Negatives do not depend on the factors: one launch draws them for the whole
// epoch ahead of the sweep.  The arithmetic of a sample, the draw stream and the sigmoid are spelled out in polara_hip.h.
// gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "blocked_sweep.h"            // after the pragma: the shared helpers are compiled without contraction too
#include "pk_sigmoid.h"               // the sigmoid (shared with lmf.hip), compiled without contraction as well

#define BPR_MAX_RANK 63             // k + 1 columns (the bias) in one wave
#define BPR_THREADS 64              // one wave per workgroup, as PMF_THREADS: a block's sweep is a chain of dependent loads

__global__ __launch_bounds__(256) void bpr_sigmoid_kernel(int64_t n, const double *__restrict__ x, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) out[t] = pk_sigmoid(x[t]);
}

extern "C" int pk_bpr_sigmoid_f64(void *stream, int64_t n, const double *x_dev, double *out_dev) {
    PK_REQUIRE(n >= 0 && n < ((int64_t)1 << 38) && (n == 0 || (x_dev && out_dev)), "pk_bpr_sigmoid_f64: bad arguments");
    if (n == 0) return PK_OK;
    hipLaunchKernelGGL(bpr_sigmoid_kernel, dim3((unsigned)pk_ceil_div(n, 256)), dim3(256), 0, pk_stream(stream), n, x_dev, out_dev);
    PK_CHECK_LAUNCH("bpr_sigmoid_kernel");
    return PK_OK;
}

// ---- the negatives of an epoch --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bpr_draw_kernel(int64_t nnz, const int32_t *__restrict__ users, const int32_t *__restrict__ items,
                                                       const int64_t *__restrict__ perm, const int32_t *__restrict__ item_order,
                                                       const int32_t *__restrict__ item_part, const int64_t *__restrict__ item_ptr,
                                                       const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                       uint64_t key, int32_t *__restrict__ neg) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const int32_t u = users[p], c = item_part[items[p]];
    const int64_t lo_c = item_ptr[c];
    const uint64_t n_c = (uint64_t)(item_ptr[c + 1] - lo_c);
    const int64_t r0 = indptr[u], r1 = indptr[u + 1];
    const uint64_t base = key + 4ull * (uint64_t)perm[p];
    int32_t found = -1;
    for (int t = 0; t < PK_BPR_DRAWS && found < 0; ++t) {
        const int32_t j = pair_draw_in_part(item_order, lo_c, n_c, pk_mix64(base + (uint64_t)t) >> 32);
        if (!pair_row_holds(indices, r0, r1, j)) found = j;
    }
    neg[p] = found;
}

extern "C" int pk_bpr_draw_negatives(void *stream, int64_t nnz, int64_t n_users, int64_t n_items, int32_t blocks,
                                     const int32_t *users_dev, const int32_t *items_dev, const int64_t *perm_dev,
                                     const int32_t *item_order_dev, const int32_t *item_part_dev, const int64_t *item_ptr_dev,
                                     const int64_t *indptr_dev, const int32_t *indices_dev, uint32_t seed, uint32_t epoch,
                                     int32_t *neg_dev) {
    const int rc = pair_draw_check("pk_bpr_draw_negatives", nnz, n_users, n_items, blocks, PK_BPR_DRAWS, PK_BPR_DRAWS,
                                   item_order_dev && item_part_dev && item_ptr_dev && indptr_dev,
                                   nnz == 0 || (users_dev && items_dev && perm_dev && indices_dev && neg_dev));
    if (rc != PK_OK) return rc;
    if (nnz == 0) return PK_OK;
    hipLaunchKernelGGL(bpr_draw_kernel, dim3((unsigned)pk_ceil_div(nnz, 256)), dim3(256), 0, pk_stream(stream), nnz, users_dev, items_dev,
                       perm_dev, item_order_dev, item_part_dev, item_ptr_dev, indptr_dev, indices_dev, pair_stream_key(seed, epoch),
                       neg_dev);
    PK_CHECK_LAUNCH("bpr_draw_kernel");
    return PK_OK;
}

// ---- the sweep --------------------------------------------------------------------------------------------------------------
struct BprArgs {
    int B, rank;
    const int64_t *block_ptr;
    const int32_t *users, *items, *neg;
    double *P, *Q;
    int64_t ldp, ldq;
    double lr, reg;
    int64_t *counts;                    // [3][B * B]: trained, skipped, correct of every block
};

// W lanes per block, 64 / W blocks per wave; lane c holds column c of the k + 1 (column k: the constant 1 of P, the bias of Q).
// The loop runs to the longest block of the wave with every lane active (the butterfly reads its neighbours); a group past the
// end of its block, or at a skipped sample (negative -1), holds no rows: it computes on zeros, loads nothing and stores nothing.
// Sample t + 1's rows are loaded while sample t is computed — unless one of them is a row of sample t, whose new value is then
// forwarded in registers: the user row, and each of the two item rows from either item row of sample t.
template <int W>
__global__ __launch_bounds__(BPR_THREADS) void bpr_stratum_kernel(BprArgs a, int stratum) {
    int c;
    const int64_t b = pk_sweep_lanes<W>(c);
    const bool qcol = c <= a.rank, pcol = c < a.rank;
    int64_t t0, len;
    const int64_t maxlen = pk_sweep_range<W>(a.B, a.block_ptr, stratum, b, t0, len);

    auto sample = [&](int64_t t, int &u, int &i, int &j) {
        u = i = j = -1;
        if (t < len) {
            j = a.neg[t0 + t];
            if (j >= 0) {
                u = a.users[t0 + t];
                i = a.items[t0 + t];
            }
        }
    };
    auto row = [&](const double *X, int64_t ld, int r) { return (r >= 0 && qcol) ? X[(int64_t)r * ld + c] : 0.0; };

    int u0, i0, j0, u1, i1, j1, u2, i2, j2;
    sample(0, u0, i0, j0);
    sample(1, u1, i1, j1);
    double p = row(a.P, a.ldp, u0), qi = row(a.Q, a.ldq, i0), qj = row(a.Q, a.ldq, j0);
    int64_t trained = 0, correct = 0;
    for (int64_t t = 0; t < maxlen; ++t) {
        sample(t + 2, u2, i2, j2);
        const bool new_u = u1 != u0;
        const bool i_from_i = i1 == i0, i_from_j = i1 == j0, j_from_i = j1 == i0, j_from_j = j1 == j0;
        const double p_next = new_u ? row(a.P, a.ldp, u1) : 0.0;
        const double qi_next = (i_from_i || i_from_j) ? 0.0 : row(a.Q, a.ldq, i1);
        const double qj_next = (j_from_i || j_from_j) ? 0.0 : row(a.Q, a.ldq, j1);

        const double d = qi - qj;
        const double x = group_sum<W>(p * d);
        const double z = pk_sigmoid(x);
        const double p_new = pcol ? p + a.lr * (z * d - a.reg * p) : p;
        const double qi_new = qi + a.lr * (z * p - a.reg * qi);
        const double qj_new = qj - a.lr * (z * p + a.reg * qj);
        if (u0 >= 0) {
            if (pcol) a.P[(int64_t)u0 * a.ldp + c] = p_new;
            if (qcol) {
                a.Q[(int64_t)i0 * a.ldq + c] = qi_new;
                a.Q[(int64_t)j0 * a.ldq + c] = qj_new;
            }
            trained += 1;
            correct += x > 0.0 ? 1 : 0;
        }
        p = new_u ? p_next : p_new;
        qi = i_from_i ? qi_new : i_from_j ? qj_new : qi_next;
        qj = j_from_i ? qi_new : j_from_j ? qj_new : qj_next;
        u0 = u1, i0 = i1, j0 = j1;
        u1 = u2, i1 = i2, j1 = j2;
    }
    if (b < a.B && c == 0) {
        const int64_t BB = (int64_t)a.B * a.B, at = (int64_t)stratum * a.B + b;
        a.counts[at] = trained;
        a.counts[BB + at] = len - trained;
        a.counts[2 * BB + at] = correct;
    }
}

// block counts -> stratum counts (block order) -> the epoch's counts (stratum order): integers, fixed order, no atomics; the
// pairwise sweeps' one reduction (pair_launch_counts of blocked_sweep.h)
__global__ __launch_bounds__(256) void pair_counts_kernel(int B, const int64_t *__restrict__ counts, int64_t *__restrict__ out) {
    __shared__ int64_t stratum_counts[PK_PMF_MAX_BLOCKS];
    const int64_t BB = (int64_t)B * B;
    for (int q = 0; q < 3; ++q) {
        for (int s = threadIdx.x; s < B; s += 256) {
            int64_t acc = 0;
            for (int b = 0; b < B; ++b) acc += counts[q * BB + (int64_t)s * B + b];
            stratum_counts[s] = acc;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t total = 0;
            for (int s = 0; s < B; ++s) total += stratum_counts[s];
            out[q] = total;
        }
        __syncthreads();
    }
}

int pair_launch_counts(hipStream_t st, int blocks, const int64_t *block_counts_dev, int64_t *counts_dev) {
    hipLaunchKernelGGL(pair_counts_kernel, dim3(1), dim3(256), 0, st, blocks, block_counts_dev, counts_dev);
    PK_CHECK_LAUNCH("pair_counts_kernel");
    return PK_OK;
}

extern "C" int32_t pk_bpr_max_rank(void) { return BPR_MAX_RANK; }
extern "C" int64_t pk_bpr_work_bytes(int32_t blocks) { return pair_work_bytes(blocks); }

extern "C" int pk_bpr_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, const int64_t *block_ptr_dev,
                                const int32_t *users_dev, const int32_t *items_dev, const int32_t *neg_dev, double *P_dev, int64_t ldp,
                                double *Q_dev, int64_t ldq, double learning_rate, double regularization, void *work_dev,
                                int64_t *counts_dev) {
    const int rc = pk_sweep_check("pk_bpr_epoch_f64", blocks, rank, BPR_MAX_RANK, rank + 1, true,
                                  nnz >= 0 && block_ptr_dev && P_dev && Q_dev && work_dev && counts_dev && P_dev != Q_dev,
                                  nnz == 0 || (users_dev && items_dev && neg_dev), "samples", ldp, ldq);
    if (rc != PK_OK) return rc;
    BprArgs a;
    a.B = blocks, a.rank = rank;
    a.block_ptr = block_ptr_dev, a.users = users_dev, a.items = items_dev, a.neg = neg_dev;
    a.P = P_dev, a.Q = Q_dev, a.ldp = ldp, a.ldq = ldq;
    a.lr = learning_rate, a.reg = regularization;
    a.counts = (int64_t *)work_dev;
    hipStream_t st = pk_stream(stream);
    return pk_sweep_epoch(
        blocks, rank + 1,
        [&](auto w, unsigned grid, int s) -> int {
            hipLaunchKernelGGL(bpr_stratum_kernel<w()>, dim3(grid), dim3(BPR_THREADS), 0, st, a, s);
            PK_CHECK_LAUNCH("bpr_stratum_kernel");
            return PK_OK;
        },
        [&] { return pair_launch_counts(st, (int)blocks, (const int64_t *)work_dev, counts_dev); });
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_bpr() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&pair_counts_kernel));
}
