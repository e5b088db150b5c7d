// Probabilistic matrix factorisation (polara/lib/optimize.py:123-154 as simple_pmf_sgd drives it): one SGD sweep over the
// interactions per epoch, on a conflict-free blocked schedule (polara_amd/pmf.py: block_schedule).  The blocks of one
// stratum share no user and no item: one launch sweeps them side by side, each block sequentially by one lane group, and the
// launches of an epoch follow each other in stream order.  The arithmetic of a sample is spelled out in polara_hip.h; the
// sweep kernel itself is pmf_stratum_kernel of blocked_sweep.h (shared with kpmf.hip), this file holds the squared error's
// reduction and the entry.
// gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "blocked_sweep.h"            // after the pragma: the shared sweep (pmf_stratum_kernel) is compiled without contraction too

// block sums -> stratum sums (block order) -> the epoch's sum (stratum order)
__global__ __launch_bounds__(256) void pmf_sse_kernel(int B, const double *__restrict__ block_sse, double *__restrict__ out) {
    __shared__ double stratum_sse[PK_PMF_MAX_BLOCKS];
    for (int s = threadIdx.x; s < B; s += 256) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc = acc + block_sse[(int64_t)s * B + b];
        stratum_sse[s] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int s = 0; s < B; ++s) total = total + stratum_sse[s];
        out[0] = total;
    }
}

int pmf_launch_sse(hipStream_t st, int blocks, const double *block_sse_dev, double *sse_dev) {
    hipLaunchKernelGGL(pmf_sse_kernel, dim3(1), dim3(256), 0, st, blocks, block_sse_dev, sse_dev);
    PK_CHECK_LAUNCH("pmf_sse_kernel");
    return PK_OK;
}

extern "C" int32_t pk_pmf_max_rank(void) { return PMF_MAX_RANK; }
extern "C" int64_t pk_pmf_work_doubles(int32_t blocks) { return (int64_t)(blocks < 1 ? 1 : blocks) * (blocks < 1 ? 1 : blocks); }

extern "C" int pk_pmf_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, const int64_t *block_ptr_dev,
                                const int32_t *users_dev, const int32_t *items_dev, const double *vals_dev, double *P_dev, int64_t ldp,
                                double *Q_dev, int64_t ldq, const double *row_nnz_dev, const double *col_nnz_dev, double eta,
                                double lambd, int32_t adjust, double *SP_dev, int64_t ldsp, double *SQ_dev, int64_t ldsq, double gamma,
                                double smoothing, double *work_dev, double *sse_dev) {
    const int rc = pk_sweep_check("pk_pmf_epoch_f64", blocks, rank, PMF_MAX_RANK, rank, true,
                                  nnz >= 0 && block_ptr_dev && P_dev && Q_dev && row_nnz_dev && col_nnz_dev && work_dev && sse_dev &&
                                      P_dev != Q_dev,
                                  nnz == 0 || (users_dev && items_dev && vals_dev), "interactions", ldp, ldq, adjust, SP_dev, SQ_dev,
                                  ldsp, ldsq);
    if (rc != PK_OK) return rc;
    PmfArgs a;
    a.B = blocks, a.rank = rank;
    a.block_ptr = block_ptr_dev, a.users = users_dev, a.items = items_dev, a.vals = vals_dev;
    a.P = P_dev, a.Q = Q_dev, a.ldp = ldp, a.ldq = ldq;
    a.rnnz = row_nnz_dev, a.cnnz = col_nnz_dev;
    a.eta = eta, a.lambd = lambd;
    a.SP = SP_dev, a.SQ = SQ_dev, a.ldsp = ldsp, a.ldsq = ldsq;
    a.gamma = gamma, a.one_minus_gamma = 1.0 - gamma, a.smoothing = smoothing;
    a.block_sse = work_dev;
    hipStream_t st = pk_stream(stream);
    return pk_sweep_epoch(
        blocks, rank,
        [&](auto w, unsigned grid, int s) { return pmf_launch<w()>(st, adjust, grid, a, s, "pmf_stratum_kernel"); },
        [&] { return pmf_launch_sse(st, (int)blocks, work_dev, sse_dev); });
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_pmf() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&pmf_sse_kernel));
}
