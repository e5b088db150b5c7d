// SLIM (Ning & Karypis, ICDM 2011): the sparse item-to-item weights W by elastic-net coordinate descent over the dense
// Gram image G = X^T X, one independent problem per target item (include/polara_hip.h has the contract).
//
//   * One workgroup of 1024 threads per target column.  Thread t owns the coordinates t, t + 1024, ... of the residual
//     image r and of the weight row w for the whole solve: it is the only thread that ever reads or writes them, so
//     neither needs a barrier or a fence.  w is the output row itself.  r lives in LDS while n <= SLIM_LDS_ITEMS, else
//     in one scratch row per workgroup in HBM (pk_set_option("slim_r_global", 1) forces that residence at any n).
//   * The contract's loop visits the coordinates in ascending order, and between two changes r is constant.  So the
//     workgroup evaluates a chunk of 1024 coordinates at once, finds the lowest one whose value changes (ballot per wave,
//     16 candidates through LDS), applies that single update (one row of the Gram image streamed against r) and goes on
//     behind it: the changing coordinates are visited in ascending order with the r the plain loop would have, hence
//     the same bits.  Both maxima of the stopping rule are order-free.
//   * No contraction: every product, sum and quotient is rounded on its own.
#include "pk_common.h"
#include <limits.h>

#pragma clang fp contract(off)

#define SLIM_THREADS 1024
#define SLIM_WAVES (SLIM_THREADS / PK_WAVE)
#define SLIM_LDS_ITEMS 19456           // r in LDS: 152 KiB of the CU's 160 KiB, the rest for the candidate and maxima slots
#define SLIM_MAX_ITEMS 65536           // the r row in HBM has no limit of its own: this one is the stated one
#define SLIM_BATCH_COLUMNS 1024        // four workgroups per CU of a launch; two are resident with r in HBM, one with r in LDS
#define SLIM_CSR_THREADS 256

extern "C" int64_t pk_slim_max_items(void) { return SLIM_MAX_ITEMS; }
extern "C" int64_t pk_slim_lds_items(void) { return SLIM_LDS_ITEMS; }
extern "C" int64_t pk_slim_batch_columns(int64_t n) { return n < 1 ? 1 : (n < SLIM_BATCH_COLUMNS ? n : SLIM_BATCH_COLUMNS); }

static bool slim_r_global(int64_t n) { return n > SLIM_LDS_ITEMS || pk_option("slim_r_global", 0) != 0; }

// the diagonal of the Gram image [n doubles, rounded up to 256 bytes], then one r row per column of the batch when r lives
// in HBM
static int64_t slim_diag_bytes(int64_t n) { return ((n < 1 ? 1 : n) * 8 + 255) / 256 * 256; }
extern "C" int64_t pk_slim_work_bytes(int64_t n, int64_t nc) {
    if (n < 1 || nc < 1) return slim_diag_bytes(n);
    return slim_diag_bytes(n) + (slim_r_global(n) ? nc * n * 8 : 0);
}

__global__ __launch_bounds__(256) void slim_diag_kernel(int64_t n, const double *__restrict__ G, int64_t ldg, double *__restrict__ diag) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) diag[k] = G[k * ldg + k];
}

template <bool R_GLOBAL>
__global__ __launch_bounds__(SLIM_THREADS) void slim_solve_kernel(int n, const double *__restrict__ G, int64_t ldg,
                                                                 const double *__restrict__ diag, int64_t j0, double l1, double l2,
                                                                 double tol, int max_sweeps, int positive, double *__restrict__ Wt,
                                                                 int64_t ldw, int32_t *__restrict__ sweeps, double *__restrict__ r_rows) {
    extern __shared__ double s_r[];
    __shared__ int s_cand[2][SLIM_WAVES];
    __shared__ double s_d;
    __shared__ double s_dmax[SLIM_WAVES], s_wmax[SLIM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = (int)(j0 + blockIdx.x);
    double *__restrict__ w = Wt + (int64_t)blockIdx.x * ldw;
    double *__restrict__ r = R_GLOBAL ? r_rows + (int64_t)blockIdx.x * n : s_r;
    const double *__restrict__ gj = G + (int64_t)j * ldg;
    for (int64_t i = tid; i < ldw; i += SLIM_THREADS) w[i] = 0.0;         // the pad columns stay exactly 0
    for (int i = tid; i < n; i += SLIM_THREADS) r[i] = gj[i];
    int parity = 0, sweep = 0;
    while (sweep < max_sweeps) {
        ++sweep;
        double dmax = 0.0, wmax = 0.0;
        int k0 = 0;
        while (k0 < n) {
            const int cb = k0 & ~(SLIM_THREADS - 1), k = cb + tid;
            double d = 0.0, nw = 0.0;
            bool counted = false;
            if (k >= k0 && k < n && k != j) {
                const double gkk = diag[k], den = gkk + l2;
                if (den > 0.0) {
                    const double old = w[k], rho = r[k] + gkk * old;
                    if (positive) {
                        const double t = rho - l1;
                        nw = t > 0.0 ? t / den : 0.0;
                    } else {
                        const double t = fabs(rho) - l1;
                        nw = t > 0.0 ? copysign(t / den, rho) : 0.0;
                    }
                    d = nw - old;
                    counted = true;
                }
            }
            const unsigned long long changed = __ballot(d != 0.0);
            if (lane == 0) s_cand[parity][wave] = changed ? cb + wave * PK_WAVE + (__ffsll((long long)changed) - 1) : INT_MAX;
            __syncthreads();
            int kmin = INT_MAX;
#pragma unroll
            for (int v = 0; v < SLIM_WAVES; ++v) kmin = min(kmin, s_cand[parity][v]);
            parity ^= 1;
            // everything in front of the first change keeps its value and is done for this sweep; what lies behind it is
            // evaluated again with the updated r
            if (counted && k <= kmin) {
                wmax = fmax(wmax, fabs(nw));
                if (k == kmin) {
                    dmax = fmax(dmax, fabs(d));
                    w[k] = nw;
                    s_d = d;
                }
            }
            if (kmin == INT_MAX) {
                k0 = cb + SLIM_THREADS;
                continue;
            }
            __syncthreads();
            const double dk = s_d;
            const double *__restrict__ gk = G + (int64_t)kmin * ldg;
            for (int i = tid; i < n; i += SLIM_THREADS) r[i] = r[i] - dk * gk[i];
            k0 = kmin + 1;
        }
        // the stopping rule: two maxima over the workgroup, the same value in every thread
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            dmax = fmax(dmax, __shfl_xor(dmax, off, 64));
            wmax = fmax(wmax, __shfl_xor(wmax, off, 64));
        }
        if (lane == 0) {
            s_dmax[wave] = dmax;
            s_wmax[wave] = wmax;
        }
        __syncthreads();
        dmax = 0.0;
        wmax = 0.0;
#pragma unroll
        for (int v = 0; v < SLIM_WAVES; ++v) {
            dmax = fmax(dmax, s_dmax[v]);
            wmax = fmax(wmax, s_wmax[v]);
        }
        __syncthreads();
        if (wmax == 0.0 || dmax <= tol * wmax) break;
    }
    if (tid == 0) sweeps[blockIdx.x] = sweep;
}

extern "C" int pk_slim_solve_f64(void *stream, int64_t n, const double *G_dev, int64_t ldg, int64_t j0, int64_t nc, double l1,
                                 double l2, double tol, int32_t max_sweeps, int32_t positive, double *Wt_block_dev, int64_t ldw,
                                 int32_t *sweeps_dev, void *work_dev) {
    PK_REQUIRE(n >= 1 && n <= SLIM_MAX_ITEMS, "pk_slim_solve_f64: %lld items outside 1..%d (pk_slim_max_items)", (long long)n,
               SLIM_MAX_ITEMS);
    PK_REQUIRE(j0 >= 0 && nc >= 0 && j0 + nc <= n, "pk_slim_solve_f64: columns [%lld, %lld) outside the %lld items", (long long)j0,
               (long long)(j0 + nc), (long long)n);
    PK_REQUIRE(ldg >= n && ldw >= n, "pk_slim_solve_f64: bad leading dimension");
    PK_REQUIRE(l1 >= 0.0 && l2 >= 0.0 && l1 <= 1.79e308 && l2 <= 1.79e308 && tol > 0.0 && max_sweeps >= 1,
               "pk_slim_solve_f64: l1 = %g, l2 = %g (finite, >= 0), tol = %g (> 0), max_sweeps = %d (>= 1)", l1, l2, tol,
               (int)max_sweeps);
    PK_REQUIRE(G_dev && work_dev && (nc == 0 || (Wt_block_dev && sweeps_dev)), "pk_slim_solve_f64: bad pointers");
    if (nc == 0) return PK_OK;
    hipStream_t st = pk_stream(stream);
    double *diag = (double *)work_dev;
    hipLaunchKernelGGL(slim_diag_kernel, dim3((unsigned)pk_ceil_div(n, 256)), dim3(256), 0, st, n, G_dev, ldg, diag);
    PK_CHECK_LAUNCH("slim_diag_kernel");
    if (slim_r_global(n)) {
        double *r_rows = (double *)((char *)work_dev + slim_diag_bytes(n));
        hipLaunchKernelGGL(slim_solve_kernel<true>, dim3((unsigned)nc), dim3(SLIM_THREADS), 0, st, (int)n, G_dev, ldg, (const double *)diag,
                           j0, l1, l2, tol, (int)max_sweeps, (int)positive, Wt_block_dev, ldw, sweeps_dev, r_rows);
    } else {
        const size_t lds = (size_t)n * sizeof(double);
        // per call: the attribute is per device and setting it is cheap (ials.hip and lce.hip do the same)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&slim_solve_kernel<false>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SLIM_LDS_ITEMS * sizeof(double)));
        if (e != hipSuccess) {
            pk_set_error("pk_slim_solve_f64: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
            return PK_E_LAUNCH;
        }
        hipLaunchKernelGGL(slim_solve_kernel<false>, dim3((unsigned)nc), dim3(SLIM_THREADS), lds, st, (int)n, G_dev, ldg,
                           (const double *)diag, j0, l1, l2, tol, (int)max_sweeps, (int)positive, Wt_block_dev, ldw, sweeps_dev,
                           (double *)nullptr);
    }
    PK_CHECK_LAUNCH("slim_solve_kernel");
    return PK_OK;
}

// ---- a batch block [nc x ldw] of rows of W^T as CSR rows: count, scan, fill -----------------------------------------------------
// An entry is stored when it is != 0; the entries of a row keep their ascending index order.
__global__ __launch_bounds__(SLIM_CSR_THREADS) void slim_csr_count_kernel(int n, const double *__restrict__ Wt, int64_t ldw,
                                                                         int64_t *__restrict__ counts) {
    __shared__ int s_cnt[SLIM_CSR_THREADS / PK_WAVE];
    const double *__restrict__ w = Wt + (int64_t)blockIdx.x * ldw;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += SLIM_CSR_THREADS) cnt += w[i] != 0.0 ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (pk_lane() == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int v = 0; v < SLIM_CSR_THREADS / PK_WAVE; ++v) total += s_cnt[v];
        counts[blockIdx.x] = total;
    }
}

// indptr[0] = 0, indptr[c + 1] = counts[0] + ... + counts[c]; one workgroup, chunks of 1024 rows (integers: any order is exact)
__global__ __launch_bounds__(SLIM_THREADS) void slim_csr_scan_kernel(int64_t nc, const int64_t *__restrict__ counts,
                                                                    int64_t *__restrict__ indptr) {
    __shared__ int64_t s[SLIM_THREADS];
    __shared__ int64_t s_base;
    if (threadIdx.x == 0) {
        s_base = 0;
        indptr[0] = 0;
    }
    __syncthreads();
    for (int64_t c0 = 0; c0 < nc; c0 += SLIM_THREADS) {
        const int64_t c = c0 + threadIdx.x;
        s[threadIdx.x] = c < nc ? counts[c] : 0;
        __syncthreads();
        for (int h = 1; h < SLIM_THREADS; h <<= 1) {
            const int64_t add = (int)threadIdx.x >= h ? s[threadIdx.x - h] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        const int64_t base = s_base;
        if (c < nc) indptr[c + 1] = base + s[threadIdx.x];
        __syncthreads();
        if (threadIdx.x == SLIM_THREADS - 1) s_base = base + s[threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(SLIM_CSR_THREADS) void slim_csr_fill_kernel(int n, const double *__restrict__ Wt, int64_t ldw,
                                                                        const int64_t *__restrict__ indptr, int64_t nnz,
                                                                        int32_t *__restrict__ indices, double *__restrict__ values) {
    __shared__ int s_cnt[SLIM_CSR_THREADS / PK_WAVE];
    const double *__restrict__ w = Wt + (int64_t)blockIdx.x * ldw;
    const int lane = pk_lane(), wave = threadIdx.x >> 6;
    int64_t pos = indptr[blockIdx.x];
    const int64_t end = indptr[blockIdx.x + 1];
    for (int i0 = 0; i0 < n; i0 += SLIM_CSR_THREADS) {
        const int i = i0 + threadIdx.x;
        const double v = i < n ? w[i] : 0.0;
        const unsigned long long keep = __ballot(v != 0.0);
        if (lane == 0) s_cnt[wave] = __popcll(keep);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int u = 0; u < SLIM_CSR_THREADS / PK_WAVE; ++u) {
            before += u < wave ? s_cnt[u] : 0;
            total += s_cnt[u];
        }
        if (v != 0.0) {
            const int64_t p = pos + before + __popcll(keep & ((1ull << lane) - 1ull));
            if (p < end && p < nnz) {          // a block that changed between the count and the fill must not write past its row
                indices[p] = i;
                values[p] = v;
            }
        }
        pos += total;
        __syncthreads();
    }
}

extern "C" int pk_slim_csr_count(void *stream, int64_t nc, int64_t n, const double *Wt_block_dev, int64_t ldw, int64_t *indptr_dev,
                                 void *work_dev) {
    PK_REQUIRE(nc >= 0 && n >= 1 && n <= SLIM_MAX_ITEMS && ldw >= n, "pk_slim_csr_count: %lld rows of %lld items, ldw %lld",
               (long long)nc, (long long)n, (long long)ldw);
    PK_REQUIRE(indptr_dev && work_dev && (nc == 0 || Wt_block_dev), "pk_slim_csr_count: bad pointers");
    hipStream_t st = pk_stream(stream);
    if (nc > 0) {
        hipLaunchKernelGGL(slim_csr_count_kernel, dim3((unsigned)nc), dim3(SLIM_CSR_THREADS), 0, st, (int)n, Wt_block_dev, ldw,
                           (int64_t *)work_dev);
        PK_CHECK_LAUNCH("slim_csr_count_kernel");
    }
    hipLaunchKernelGGL(slim_csr_scan_kernel, dim3(1), dim3(SLIM_THREADS), 0, st, nc, (const int64_t *)work_dev, indptr_dev);
    PK_CHECK_LAUNCH("slim_csr_scan_kernel");
    return PK_OK;
}

extern "C" int pk_slim_csr_fill(void *stream, int64_t nc, int64_t n, const double *Wt_block_dev, int64_t ldw,
                                const int64_t *indptr_dev, int64_t nnz, int32_t *indices_dev, double *values_dev) {
    PK_REQUIRE(nc >= 0 && n >= 1 && n <= SLIM_MAX_ITEMS && ldw >= n && nnz >= 0, "pk_slim_csr_fill: %lld rows of %lld items, ldw %lld",
               (long long)nc, (long long)n, (long long)ldw);
    PK_REQUIRE(indptr_dev && (nc == 0 || Wt_block_dev) && (nnz == 0 || (indices_dev && values_dev)), "pk_slim_csr_fill: bad pointers");
    if (nc == 0 || nnz == 0) return PK_OK;
    hipLaunchKernelGGL(slim_csr_fill_kernel, dim3((unsigned)nc), dim3(SLIM_CSR_THREADS), 0, pk_stream(stream), (int)n, Wt_block_dev, ldw,
                       indptr_dev, nnz, indices_dev, values_dev);
    PK_CHECK_LAUNCH("slim_csr_fill_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_slim() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&slim_diag_kernel));
}
