// Kernelized probabilistic matrix factorisation (polara/lib/optimize.py:258-301: `generalized_sgd_sweep` with
// `sparse_kernel_update` as its transform): PMF's blocked sweep (pmf.hip) whose regulariser reads the neighbours of the
// sample's user and item in two kernel matrices.  A neighbour row of the block's own user (item) part is read live — the
// block alone writes it during the stratum —, every other one from a snapshot taken when the stratum began, so no block
// reads what another one is writing.  The arithmetic of a sample is spelled out in polara_hip.h.  gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "pmf_common.h"               // after the pragma: the shared helpers are compiled without contraction too

#define KPMF_BATCH 4                // neighbour rows whose loads are issued together

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

// off = (+0.0 + K[e1] * X(j1)) + K[e2] * X(j2) + ... over row r's stored off-diagonal entries in storage order, for column c.
// X(j) is row j of `live` when j lies in the block's own part and row j of the snapshot otherwise.  The loads of a batch are
// independent of each other; they stay behind the stores of the sample before, which may have written a live row.
__device__ __forceinline__ double kpmf_neighbours(const KpmfSide &k, int my_part, const double *live, int64_t ldlive, int r, int c,
                                                  bool on) {
    double acc = 0.0;
    if (!on) return acc;
    int64_t e = k.ptr[r];
    const int64_t end = k.ptr[r + 1];
    for (; e + KPMF_BATCH <= end; e += KPMF_BATCH) {
        int32_t j[KPMF_BATCH];
        double kv[KPMF_BATCH], x[KPMF_BATCH];
        bool own[KPMF_BATCH];
#pragma unroll
        for (int b = 0; b < KPMF_BATCH; ++b) {
            j[b] = k.idx[e + b];
            kv[b] = k.val[e + b];
        }
#pragma unroll
        for (int b = 0; b < KPMF_BATCH; ++b) own[b] = k.part[j[b]] == my_part;
#pragma unroll
        for (int b = 0; b < KPMF_BATCH; ++b)
            x[b] = own[b] ? live[(int64_t)j[b] * ldlive + c] : k.snap[(int64_t)j[b] * k.ldsnap + c];
#pragma unroll
        for (int b = 0; b < KPMF_BATCH; ++b) acc = acc + kv[b] * x[b];
    }
    for (; e < end; ++e) {
        const int32_t j = k.idx[e];
        const double x = k.part[j] == my_part ? live[(int64_t)j * ldlive + c] : k.snap[(int64_t)j * k.ldsnap + c];
        acc = acc + k.val[e] * x;
    }
    return acc;
}

// pmf_stratum_kernel with the two transforms.  Lane group g of workgroup x sweeps block b = x * G + g of the stratum: user
// part b, item part (b + stratum) mod B.  The user's neighbour sum is computed once per run of a user (the block writes no
// other user row meanwhile), the item's per sample.
template <int W, int ADJ>
__global__ __launch_bounds__(PMF_THREADS) void kpmf_stratum_kernel(KpmfArgs ka, int stratum) {
    const PmfArgs &a = ka.pmf;
    constexpr int G = 64 / W;
    const int lane = pk_lane();
    const int g = lane / W, c = lane % W;
    const int64_t b = (int64_t)blockIdx.x * G + g;
    const bool col = c < a.rank;
    const int upart = (int)b, ipart = (int)((b + stratum) % a.B);
    int64_t t0 = 0, len = 0;
    if (b < a.B) {
        t0 = a.block_ptr[(int64_t)stratum * a.B + b];
        len = a.block_ptr[(int64_t)stratum * a.B + b + 1] - t0;
    }
    int64_t maxlen = len;
#pragma unroll
    for (int off = 32; off >= W; off >>= 1) {
        const int64_t o = __shfl_xor(maxlen, off, 64);
        maxlen = o > maxlen ? o : maxlen;
    }
    maxlen = ((int64_t)__builtin_amdgcn_readfirstlane((int)(maxlen >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(maxlen & 0xffffffffll));

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
    double du0 = diag(ka.u.diag, m0), di0 = diag(ka.i.diag, n0);
    double off_p = 0.0, sse = 0.0;
    bool first_of_run = true;
    for (int64_t t = 0; t < maxlen; ++t) {
        sample(t + 2, m2, n2, v2);
        const bool new_m = m1 != m0, new_n = n1 != n0;
        const double p_next = new_m ? row(a.P, a.ldp, m1) : 0.0, q_next = new_n ? row(a.Q, a.ldq, n1) : 0.0;
        const double sp_next = (ADJ && new_m) ? row(a.SP, a.ldsp, m1) : 0.0, sq_next = (ADJ && new_n) ? row(a.SQ, a.ldsq, n1) : 0.0;
        const double rc1 = count(a.rnnz, m1), cc1 = count(a.cnnz, n1);
        const double du1 = diag(ka.u.diag, m1), di1 = diag(ka.i.diag, n1);

        if (first_of_run) off_p = kpmf_neighbours(ka.u, upart, a.P, a.ldp, m0, c, m0 >= 0 && col);
        const double off_q = kpmf_neighbours(ka.i, ipart, a.Q, a.ldq, n0, c, n0 >= 0 && col);

        const double dot = pmf_group_sum<W>(p * q);
        const double err = v0 - dot;
        const double row_lambda = a.lambd / rc0, col_lambda = a.lambd / cc0;
        const double kp = off_p + du0 * (p + p);
        const double kq = off_q + di0 * (q + q);
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

// the snapshots take what the finished stratum left: both factor blocks, whole, in one launch
__global__ __launch_bounds__(256) void kpmf_snapshot_kernel(int rank, int64_t n_users, int64_t n_items, const double *__restrict__ P,
                                                            int64_t ldp, const double *__restrict__ Q, int64_t ldq,
                                                            double *__restrict__ PS, int64_t ldps, double *__restrict__ QS,
                                                            int64_t ldqs) {
    const int64_t total = (n_users + n_items) * rank;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += (int64_t)gridDim.x * 256) {
        const int64_t r = x / rank;
        const int c = (int)(x - r * rank);
        if (r < n_users)
            PS[r * ldps + c] = P[r * ldp + c];
        else
            QS[(r - n_users) * ldqs + c] = Q[(r - n_users) * ldq + c];
    }
}

template <int W>
static void kpmf_launch(hipStream_t st, int adjust, unsigned grid, const KpmfArgs &a, int stratum) {
    if (adjust == PK_PMF_ADJUST_NONE)
        hipLaunchKernelGGL((kpmf_stratum_kernel<W, PK_PMF_ADJUST_NONE>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else if (adjust == PK_PMF_ADJUST_ADAGRAD)
        hipLaunchKernelGGL((kpmf_stratum_kernel<W, PK_PMF_ADJUST_ADAGRAD>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else
        hipLaunchKernelGGL((kpmf_stratum_kernel<W, PK_PMF_ADJUST_RMSPROP>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
}

extern "C" int pk_kpmf_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, int64_t n_users, int64_t n_items,
                                 const int64_t *block_ptr_dev, const int32_t *users_dev, const int32_t *items_dev,
                                 const double *vals_dev, double *P_dev, int64_t ldp, double *Q_dev, int64_t ldq,
                                 const double *row_nnz_dev, const double *col_nnz_dev, const int32_t *user_part_dev,
                                 const int32_t *item_part_dev, const int64_t *ku_ptr_dev, const int32_t *ku_idx_dev,
                                 const double *ku_val_dev, const double *ku_diag_dev, const int64_t *ki_ptr_dev,
                                 const int32_t *ki_idx_dev, const double *ki_val_dev, const double *ki_diag_dev,
                                 double *P_snap_dev, int64_t ldps, double *Q_snap_dev, int64_t ldqs, double eta, double lambd,
                                 int32_t adjust, double *SP_dev, int64_t ldsp, double *SQ_dev, int64_t ldsq, double gamma,
                                 double smoothing, double *work_dev, double *sse_dev) {
    PK_REQUIRE(rank >= 1 && rank <= PMF_MAX_RANK, "pk_kpmf_epoch_f64: rank %d outside 1..%d", (int)rank, PMF_MAX_RANK);
    PK_REQUIRE(blocks >= 1 && blocks <= PK_PMF_MAX_BLOCKS, "pk_kpmf_epoch_f64: %d blocks outside 1..%d", (int)blocks, PK_PMF_MAX_BLOCKS);
    PK_REQUIRE(nnz >= 0 && n_users >= 1 && n_items >= 1 && n_users < (1ll << 31) && n_items < (1ll << 31),
               "pk_kpmf_epoch_f64: bad sizes");
    PK_REQUIRE(block_ptr_dev && P_dev && Q_dev && row_nnz_dev && col_nnz_dev && work_dev && sse_dev && P_dev != Q_dev,
               "pk_kpmf_epoch_f64: bad pointers");
    PK_REQUIRE(nnz == 0 || (users_dev && items_dev && vals_dev), "pk_kpmf_epoch_f64: no interactions given");
    PK_REQUIRE(ldp >= rank && ldq >= rank, "pk_kpmf_epoch_f64: bad leading dimension");
    PK_REQUIRE(user_part_dev && item_part_dev && ku_ptr_dev && ku_diag_dev && ki_ptr_dev && ki_diag_dev,
               "pk_kpmf_epoch_f64: the kernel matrices (row pointers, diagonals) and the parts are needed");
    PK_REQUIRE(P_snap_dev && Q_snap_dev && P_snap_dev != Q_snap_dev && P_snap_dev != P_dev && Q_snap_dev != Q_dev && ldps >= rank &&
                   ldqs >= rank,
               "pk_kpmf_epoch_f64: the two snapshot blocks are needed, apart from P and Q");
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || adjust == PK_PMF_ADJUST_ADAGRAD || adjust == PK_PMF_ADJUST_RMSPROP,
               "pk_kpmf_epoch_f64: unknown gradient adjustment %d", (int)adjust);
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || (SP_dev && SQ_dev && SP_dev != SQ_dev && ldsp >= rank && ldsq >= rank),
               "pk_kpmf_epoch_f64: the gradient adjustment needs its two state blocks");
    KpmfArgs ka;
    PmfArgs &a = ka.pmf;
    a.B = blocks, a.rank = rank;
    a.block_ptr = block_ptr_dev, a.users = users_dev, a.items = items_dev, a.vals = vals_dev;
    a.P = P_dev, a.Q = Q_dev, a.ldp = ldp, a.ldq = ldq;
    a.rnnz = row_nnz_dev, a.cnnz = col_nnz_dev;
    a.eta = eta, a.lambd = lambd;
    a.SP = SP_dev, a.SQ = SQ_dev, a.ldsp = ldsp, a.ldsq = ldsq;
    a.gamma = gamma, a.one_minus_gamma = 1.0 - gamma, a.smoothing = smoothing;
    a.block_sse = work_dev;
    ka.u = KpmfSide{ku_ptr_dev, ku_idx_dev, ku_val_dev, ku_diag_dev, user_part_dev, P_snap_dev, ldps};
    ka.i = KpmfSide{ki_ptr_dev, ki_idx_dev, ki_val_dev, ki_diag_dev, item_part_dev, Q_snap_dev, ldqs};
    const int w = rank <= 16 ? 16 : rank <= 32 ? 32 : 64;
    const unsigned grid = (unsigned)pk_ceil_div(blocks, 64 / w);
    const int64_t cells = (n_users + n_items) * rank;
    const unsigned copy_grid = (unsigned)(pk_ceil_div(cells, (int64_t)256) < 4096 ? pk_ceil_div(cells, (int64_t)256) : 4096);
    hipStream_t st = pk_stream(stream);
    auto snapshot = [&]() {
        hipLaunchKernelGGL(kpmf_snapshot_kernel, dim3(copy_grid), dim3(256), 0, st, (int)rank, n_users, n_items, (const double *)P_dev,
                           ldp, (const double *)Q_dev, ldq, P_snap_dev, ldps, Q_snap_dev, ldqs);
    };
    snapshot();                                     // P and Q as the epoch finds them
    PK_CHECK_LAUNCH("kpmf_snapshot_kernel");
    for (int s = 0; s < blocks; ++s) {
        if (w == 16)
            kpmf_launch<16>(st, adjust, grid, ka, s);
        else if (w == 32)
            kpmf_launch<32>(st, adjust, grid, ka, s);
        else
            kpmf_launch<64>(st, adjust, grid, ka, s);
        PK_CHECK_LAUNCH("kpmf_stratum_kernel");
        snapshot();                                 // what this stratum wrote, for the next one
        PK_CHECK_LAUNCH("kpmf_snapshot_kernel");
    }
    pmf_launch_sse(st, (int)blocks, work_dev, sse_dev);
    PK_CHECK_LAUNCH("pmf_sse_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_kpmf() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&kpmf_snapshot_kernel));
}
