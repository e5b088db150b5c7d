// Kernelized probabilistic matrix factorisation (polara/lib/optimize.py:258-301: `generalized_sgd_sweep` with
// `sparse_kernel_update` as its transform): PMF's blocked sweep (pmf_stratum_kernel of blocked_sweep.h, instantiated here on
// KpmfArgs; this file holds its gather, the snapshot copy and the entry) whose regulariser reads the neighbours of the
// sample's user and item in two kernel matrices.  A neighbour row of the block's own user (item) part is read live — the
// block alone writes it during the stratum —, every other one from a snapshot taken when the stratum began, so no block
// reads what another one is writing.  The arithmetic of a sample is spelled out in polara_hip.h.  gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "blocked_sweep.h"            // after the pragma: the shared sweep (pmf_stratum_kernel) is compiled without contraction too

#define KPMF_BATCH 4                // neighbour rows whose loads are issued together

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
    const int rc = pk_sweep_check("pk_kpmf_epoch_f64", blocks, rank, PMF_MAX_RANK, rank,
                                  nnz >= 0 && n_users >= 1 && n_items >= 1 && n_users < (1ll << 31) && n_items < (1ll << 31),
                                  block_ptr_dev && P_dev && Q_dev && row_nnz_dev && col_nnz_dev && work_dev && sse_dev && P_dev != Q_dev,
                                  nnz == 0 || (users_dev && items_dev && vals_dev), "interactions", ldp, ldq, adjust, SP_dev, SQ_dev,
                                  ldsp, ldsq);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(user_part_dev && item_part_dev && ku_ptr_dev && ku_diag_dev && ki_ptr_dev && ki_diag_dev,
               "pk_kpmf_epoch_f64: the kernel matrices (row pointers, diagonals) and the parts are needed");
    PK_REQUIRE(P_snap_dev && Q_snap_dev && P_snap_dev != Q_snap_dev && P_snap_dev != P_dev && Q_snap_dev != Q_dev && ldps >= rank &&
                   ldqs >= rank,
               "pk_kpmf_epoch_f64: the two snapshot blocks are needed, apart from P and Q");
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
    const int64_t cells = (n_users + n_items) * rank;
    const unsigned copy_grid = (unsigned)(pk_ceil_div(cells, (int64_t)256) < 4096 ? pk_ceil_div(cells, (int64_t)256) : 4096);
    hipStream_t st = pk_stream(stream);
    auto snapshot = [&]() -> int {
        hipLaunchKernelGGL(kpmf_snapshot_kernel, dim3(copy_grid), dim3(256), 0, st, (int)rank, n_users, n_items, (const double *)P_dev,
                           ldp, (const double *)Q_dev, ldq, P_snap_dev, ldps, Q_snap_dev, ldqs);
        PK_CHECK_LAUNCH("kpmf_snapshot_kernel");
        return PK_OK;
    };
    if (snapshot() != PK_OK) return PK_E_LAUNCH;                    // P and Q as the epoch finds them
    return pk_sweep_epoch(
        blocks, rank,
        [&](auto w, unsigned grid, int s) -> int {
            const int launched = pmf_launch<w()>(st, adjust, grid, ka, s, "kpmf_stratum_kernel");
            return launched != PK_OK ? launched : snapshot();       // what this stratum wrote, for the next one
        },
        [&] { return pmf_launch_sse(st, (int)blocks, work_dev, sse_dev); });
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_kpmf() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&kpmf_snapshot_kernel));
}
