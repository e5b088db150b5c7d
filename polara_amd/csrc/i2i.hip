// Item-to-item (CooccurrenceModel, models.py:699-725) and most-popular (PopularityModel, models.py:649-666) baselines on the
// device: the build of the co-occurrence matrix C = A^T A (diagonal 0), its certified fp32 image, the scoring pass
// s_u = sum_i t_ui C[i, :] with the seen-item masking and the per-user top-k fused into it, and the popularity top-k.
//
//   * build (row-owner Gustavson, no global atomics): workgroup (i, w) owns columns [w * WIN, (w + 1) * WIN) of row i of C
//     and accumulates them in an fp64 LDS array.  Its four waves take different users of item i (the CSC image), the lanes
//     of a wave the entries of that user's row that fall into the window (two binary searches in the sorted columns);
//     `atomicAdd` on a __shared__ double is ds_add_f64 on gfx950.  Every product and partial sum of integer or
//     half-integer data is exact, so C is bit-exact whatever the order of the adds;
//   * image: one pass converts C to fp32 and raises a flag where (double)(float)c != c — C is kept as fp32 only when the
//     flag stays down (scoring always accumulates in fp64: the image only halves the bytes it reads);
//   * scoring: workgroup (u, w) sums the rows C[i, w * 2048 : (w + 1) * 2048) of the user's test items into fp64
//     registers (8 fixed columns per lane, 16-byte loads), marks the user's seen columns of the window in a register
//     mask, forms the key (class, score, item) of every column and bitonic-sorts the 2048 keys in LDS; the best P of
//     every window go to a candidate buffer, and a second kernel merges the windows of a user (one bitonic merge per
//     window) into the final list.  The grid runs window-major (users fastest), so the workgroups in flight read one
//     column slab of C (n_items x 2048 x 4 B = 219 MB at the ML-20M shape: it fits the 256 MiB Infinity Cache), and a
//     heavy user is split over all its windows instead of forming a tail;
//   * popularity: one wave per user walks the global item order (score desc, item asc; one device radix sort at build
//     time), tests each item against the user's seen bitmap in LDS and keeps the first topk unseen items (ballot +
//     prefix count); when a user has fewer than topk unseen items, its seen items follow in the same order.
//
// The key of a column, best first: class descending (2 = candidate, 1 = seen item of the dense branch under
// filter_seen, 0 = not a candidate: pad), then score descending, then item ascending — one total order, so the lists
// are a function of the scores alone.
#include "i2i_keys.h"

#define PK_I2I_BUILD_WIN 8192        // fp64 columns of C per build workgroup (64 KiB of LDS)
#define PK_POP_MAX_ITEMS (1 << 19)   // the popularity kernel's seen bitmap: 64 KiB of LDS

// ---- planning (host functions, no device needed) -------------------------------------------------------------
extern "C" int32_t pk_i2i_max_topk(void) { return PK_I2I_MAX_TOPK; }
extern "C" int32_t pk_i2i_window(void) { return PK_I2I_WIN; }
extern "C" int32_t pk_i2i_build_window(void) { return PK_I2I_BUILD_WIN; }

extern "C" int64_t pk_i2i_ld(int64_t n_items) { return pk_ceil_div(n_items, PK_I2I_COLS) * PK_I2I_COLS; }

extern "C" int64_t pk_i2i_chunk_users(int64_t n_users, int64_t n_items, int32_t topk) {
    if (n_users <= 0 || n_items <= 0 || topk < 1 || topk > PK_I2I_MAX_TOPK) return 0;
    const int64_t per_user = pk_ceil_div(pk_i2i_ld(n_items), PK_I2I_WIN) * i2i_pow2(topk) * 12;
    const int64_t c = PK_I2I_CAND_BUDGET / per_user;
    return c < 1 ? 1 : (c < n_users ? c : n_users);
}

extern "C" int64_t pk_i2i_topk_work_bytes(int64_t n_users, int64_t n_items, int32_t topk) {
    const int64_t chunk = pk_i2i_chunk_users(n_users, n_items, topk);
    const int64_t n = chunk * pk_ceil_div(pk_i2i_ld(n_items), PK_I2I_WIN) * i2i_pow2(topk);
    return n * 8 + n * 4 + 256;
}

// ---- build -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void i2i_build_kernel(int64_t n_items, const int64_t *__restrict__ indptr,
                                                        const int32_t *__restrict__ indices, const void *__restrict__ values,
                                                        int val_kind, const int64_t *__restrict__ t_indptr,
                                                        const int32_t *__restrict__ t_indices,
                                                        const void *__restrict__ t_values, double *__restrict__ C, int64_t ldc) {
    __shared__ double acc[PK_I2I_BUILD_WIN];
    const int64_t i = blockIdx.x;
    const int64_t w0 = (int64_t)blockIdx.y * PK_I2I_BUILD_WIN;
    const int64_t wn = ldc - w0 < PK_I2I_BUILD_WIN ? ldc - w0 : PK_I2I_BUILD_WIN;
    for (int c = threadIdx.x; c < wn; c += 256) acc[c] = 0.0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c_hi = w0 + wn < n_items ? w0 + wn : n_items;
    for (int64_t p = t_indptr[i] + wave; p < t_indptr[i + 1]; p += 4) {
        const int64_t u = t_indices[p];
        const double a = i2i_val(t_values, val_kind, p);
        const int64_t lo = i2i_lower_bound(indices, indptr[u], indptr[u + 1], w0);
        const int64_t hi = i2i_lower_bound(indices, lo, indptr[u + 1], c_hi);
        for (int64_t q = lo + lane; q < hi; q += 64) atomicAdd(&acc[indices[q] - w0], a * i2i_val(values, val_kind, q));
    }
    __syncthreads();
    double *row = C + i * ldc + w0;
    for (int c = threadIdx.x; c < wn; c += 256) row[c] = (w0 + c == i) ? 0.0 : acc[c];
}

extern "C" int pk_i2i_build_f64(void *stream, int64_t n_users, int64_t n_items, const int64_t *indptr_dev,
                                const int32_t *indices_dev, const void *values_dev, int val_kind,
                                const int64_t *t_indptr_dev, const int32_t *t_indices_dev, const void *t_values_dev,
                                double *C_dev, int64_t ldc) {
    PK_REQUIRE(n_users >= 0 && n_items >= 1 && n_items <= (int64_t)PK_I2I_ITEM_MASK && ldc >= n_items && ldc % PK_I2I_COLS == 0,
               "pk_i2i_build_f64: bad shape (n_items %lld, ldc %lld: 1 <= n_items < 2^30, ldc >= n_items, ldc %% %d == 0)",
               (long long)n_items, (long long)ldc, PK_I2I_COLS);
    PK_REQUIRE(indptr_dev && t_indptr_dev && C_dev && (val_kind == PK_VAL_F32 || val_kind == PK_VAL_F64),
               "pk_i2i_build_f64: null pointer or bad val_kind");
    const int64_t n_win = pk_ceil_div(ldc, PK_I2I_BUILD_WIN);
    PK_REQUIRE(n_win <= 65535 && n_items <= 0x7fffffff, "pk_i2i_build_f64: catalogue too large for the grid");
    hipLaunchKernelGGL(i2i_build_kernel, dim3((unsigned)n_items, (unsigned)n_win), dim3(256), 0, pk_stream(stream), n_items,
                       indptr_dev, indices_dev, values_dev, val_kind, t_indptr_dev, t_indices_dev, t_values_dev, C_dev, ldc);
    PK_CHECK_LAUNCH("i2i_build_kernel");
    return PK_OK;
}

// ---- certified fp32 image ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void i2i_image_kernel(int64_t n, const double *__restrict__ C64, float *__restrict__ C32,
                                                        int32_t *__restrict__ inexact) {
    bool bad = false;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const double c = C64[e];
        const float f = (float)c;
        C32[e] = f;
        bad |= ((double)f != c);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(inexact, 1);
}

extern "C" int pk_i2i_image_f32(void *stream, int64_t n, const double *C64_dev, float *C32_dev, int32_t *inexact_dev) {
    PK_REQUIRE(n >= 0 && C64_dev && C32_dev && inexact_dev, "pk_i2i_image_f32: bad arguments");
    if (n == 0) return PK_OK;
    const int64_t blocks = pk_ceil_div(n, 256 * 8);
    hipLaunchKernelGGL(i2i_image_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, pk_stream(stream), n,
                       C64_dev, C32_dev, inexact_dev);
    PK_CHECK_LAUNCH("i2i_image_kernel");
    return PK_OK;
}

// ---- scoring -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void i2i_load8(const float *__restrict__ p, double *c) {
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
}
__device__ __forceinline__ void i2i_load8(const double *__restrict__ p, double *c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double2 a = reinterpret_cast<const double2 *>(p)[k];
        c[2 * k] = a.x, c[2 * k + 1] = a.y;
    }
}

template <typename CT>
__global__ __launch_bounds__(PK_I2I_THREADS) void i2i_window_kernel(
    int64_t u0, int64_t n_items, const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices,
    const void *__restrict__ t_values, int t_kind, const CT *__restrict__ C, int64_t ldc, int P, int filter_seen, int sparse,
    uint64_t *__restrict__ cand_s, uint32_t *__restrict__ cand_m) {
    __shared__ uint64_t ks[PK_I2I_WIN];
    __shared__ uint32_t km[PK_I2I_WIN];
    const int64_t u = u0 + blockIdx.x;
    const int64_t col0 = (int64_t)blockIdx.y * PK_I2I_WIN + threadIdx.x * PK_I2I_COLS;
    const bool live = col0 < ldc;            // ldc is a multiple of PK_I2I_COLS: a lane's 8 columns are all in or all out
    double acc[PK_I2I_COLS];
#pragma unroll
    for (int j = 0; j < PK_I2I_COLS; ++j) acc[j] = 0.0;
    uint32_t seen = 0;
    const int64_t p0 = t_indptr[u], p1 = t_indptr[u + 1];
    int64_t p = p0;
    // entries with zero feedback add fma(0, c, acc) = acc: no branch, they are only marked seen
    for (; p + 4 <= p1; p += 4) {
        int64_t it[4];
        double tv[4], c[4][PK_I2I_COLS];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            it[e] = t_indices[p + e];
            tv[e] = i2i_val(t_values, t_kind, p + e);
            const uint64_t d = (uint64_t)(it[e] - col0);
            if (d < PK_I2I_COLS) seen |= 1u << d;
        }
        if (live) {
#pragma unroll
            for (int e = 0; e < 4; ++e) i2i_load8(C + it[e] * ldc + col0, c[e]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < PK_I2I_COLS; ++j) acc[j] = fma(tv[e], c[e][j], acc[j]);
        }
    }
    for (; p < p1; ++p) {
        const int64_t it = t_indices[p];
        const double tv = i2i_val(t_values, t_kind, p);
        const uint64_t d = (uint64_t)(it - col0);
        if (d < PK_I2I_COLS) seen |= 1u << d;
        if (live) {
            double c[PK_I2I_COLS];
            i2i_load8(C + it * ldc + col0, c);
#pragma unroll
            for (int j = 0; j < PK_I2I_COLS; ++j) acc[j] = fma(tv, c[j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < PK_I2I_COLS; ++j) {
        const int64_t col = col0 + j;
        const double s = acc[j] == 0.0 ? 0.0 : acc[j];          // -0 -> +0
        const bool sn = filter_seen && ((seen >> j) & 1u);
        uint32_t cls;
        if (col >= n_items)
            cls = 0;
        else if (sparse)
            cls = (s != 0.0 && !sn) ? 2 : 0;
        else
            cls = sn ? 1 : 2;
        const int slot = threadIdx.x * PK_I2I_COLS + j;
        ks[slot] = cls ? i2i_key(s) : 0;
        km[slot] = cls ? ((cls << 30) | (uint32_t)col) : PK_I2I_ITEM_MASK;
    }
    __syncthreads();
    i2i_sort<PK_I2I_THREADS>(ks, km, PK_I2I_WIN);
    const int64_t base = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * P;
    for (int k = threadIdx.x; k < P; k += PK_I2I_THREADS) {
        cand_s[base + k] = ks[k];
        cand_m[base + k] = km[k];
    }
}

// one wave per user: the best P of every window merged into the user's list
__global__ __launch_bounds__(64) void i2i_merge_kernel(int64_t u0, int n_win, int P, int topk, const uint64_t *__restrict__ cand_s,
                                                       const uint32_t *__restrict__ cand_m, int64_t *__restrict__ out_idx,
                                                       double *__restrict__ out_scores) {
    __shared__ uint64_t bs[2 * PK_I2I_MAX_TOPK];
    __shared__ uint32_t bm[2 * PK_I2I_MAX_TOPK];
    const int64_t base = (int64_t)blockIdx.x * n_win * P;
    for (int k = threadIdx.x; k < P; k += 64) {
        bs[k] = cand_s[base + k];
        bm[k] = cand_m[base + k];
    }
    for (int w = 1; w < n_win; ++w) {
        // window w's list reversed behind the running best P: a bitonic sequence of 2P keys
        for (int k = threadIdx.x; k < P; k += 64) {
            bs[2 * P - 1 - k] = cand_s[base + (int64_t)w * P + k];
            bm[2 * P - 1 - k] = cand_m[base + (int64_t)w * P + k];
        }
        __syncthreads();
        for (int j = P; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P; t += 64) {
                const int i = i2i_pair(t, j);
                i2i_cmpx(bs, bm, i, i + j);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int64_t u = u0 + blockIdx.x;
    for (int k = threadIdx.x; k < topk; k += 64) {
        const bool pad = (bm[k] >> 30) == 0;
        out_idx[u * topk + k] = pad ? -1 : (int64_t)(bm[k] & PK_I2I_ITEM_MASK);
        if (out_scores) out_scores[u * topk + k] = pad ? 0.0 : i2i_unkey(bs[k]);
    }
}

void i2i_launch_merge(hipStream_t s, int64_t nu, int64_t u0, int n_win, int P, int topk, const uint64_t *cand_s,
                      const uint32_t *cand_m, int64_t *out_idx, double *out_scores) {
    hipLaunchKernelGGL(i2i_merge_kernel, dim3((unsigned)nu), dim3(64), 0, s, u0, n_win, P, topk, cand_s, cand_m, out_idx,
                       out_scores);
}

extern "C" int pk_i2i_topk(void *stream, int64_t n_users, int64_t n_items, const int64_t *t_indptr_dev,
                           const int32_t *t_indices_dev, const void *t_values_dev, int t_val_kind, const void *C_dev,
                           int c_kind, int64_t ldc, int32_t topk, int32_t filter_seen, int32_t sparse, int64_t *out_idx_dev,
                           double *out_scores_dev, void *work_dev) {
    PK_REQUIRE(topk >= 1 && topk <= PK_I2I_MAX_TOPK, "pk_i2i_topk: topk %d outside 1..%d", (int)topk, PK_I2I_MAX_TOPK);
    PK_REQUIRE(n_users >= 0 && n_items >= 1 && n_items <= (int64_t)PK_I2I_ITEM_MASK && ldc == pk_i2i_ld(n_items),
               "pk_i2i_topk: bad shape (n_items %lld, ldc %lld != pk_i2i_ld)", (long long)n_items, (long long)ldc);
    PK_REQUIRE((c_kind == PK_VAL_F32 || c_kind == PK_VAL_F64) && (t_val_kind == PK_VAL_F32 || t_val_kind == PK_VAL_F64),
               "pk_i2i_topk: bad value kind");
    PK_REQUIRE(t_indptr_dev && C_dev && out_idx_dev && work_dev, "pk_i2i_topk: null pointer");
    if (n_users == 0) return PK_OK;
    const int64_t n_win = pk_ceil_div(ldc, PK_I2I_WIN);
    PK_REQUIRE(n_win <= 65535, "pk_i2i_topk: catalogue too large for the grid");
    const int P = i2i_pow2(topk);
    const int64_t chunk = pk_i2i_chunk_users(n_users, n_items, topk);
    uint64_t *cand_s = static_cast<uint64_t *>(work_dev);
    uint32_t *cand_m = reinterpret_cast<uint32_t *>(cand_s + chunk * n_win * P);
    hipStream_t s = pk_stream(stream);
    for (int64_t u0 = 0; u0 < n_users; u0 += chunk) {
        const int64_t nu = n_users - u0 < chunk ? n_users - u0 : chunk;
        if (c_kind == PK_VAL_F32)
            hipLaunchKernelGGL(i2i_window_kernel<float>, dim3((unsigned)nu, (unsigned)n_win), dim3(PK_I2I_THREADS), 0, s, u0,
                               n_items, t_indptr_dev, t_indices_dev, t_values_dev, t_val_kind,
                               static_cast<const float *>(C_dev), ldc, P, filter_seen, sparse, cand_s, cand_m);
        else
            hipLaunchKernelGGL(i2i_window_kernel<double>, dim3((unsigned)nu, (unsigned)n_win), dim3(PK_I2I_THREADS), 0, s, u0,
                               n_items, t_indptr_dev, t_indices_dev, t_values_dev, t_val_kind,
                               static_cast<const double *>(C_dev), ldc, P, filter_seen, sparse, cand_s, cand_m);
        PK_CHECK_LAUNCH("i2i_window_kernel");
        i2i_launch_merge(s, nu, u0, (int)n_win, P, (int)topk, cand_s, cand_m, out_idx_dev, out_scores_dev);
        PK_CHECK_LAUNCH("i2i_merge_kernel");
    }
    return PK_OK;
}

// ---- popularity --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void popular_keys_kernel(int64_t n, const double *__restrict__ scores,
                                                           uint64_t *__restrict__ keys, uint32_t *__restrict__ ids) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double s = scores[e] == 0.0 ? 0.0 : scores[e];
    keys[e] = ~i2i_key(s);      // ascending keys = descending scores; the stable sort keeps ids ascending within ties
    ids[e] = (uint32_t)e;
}

extern "C" int64_t pk_popular_order_work_bytes(int64_t n_items) {
    return 2 * n_items * 8 + n_items * 4 + 256 + pk_radix_work_bytes(n_items);
}

extern "C" int pk_popular_order(void *stream, int64_t n_items, const double *scores_dev, int32_t *order_dev, void *work_dev) {
    PK_REQUIRE(n_items >= 1 && n_items <= PK_POP_MAX_ITEMS && scores_dev && order_dev && work_dev,
               "pk_popular_order: bad arguments (1 <= n_items <= %d)", PK_POP_MAX_ITEMS);
    uint64_t *keys = static_cast<uint64_t *>(work_dev);
    uint64_t *keys_tmp = keys + n_items;
    uint32_t *ids_tmp = reinterpret_cast<uint32_t *>(keys_tmp + n_items);
    void *rwork = reinterpret_cast<char *>(work_dev) + pk_ceil_div(2 * n_items * 8 + n_items * 4, 256) * 256;
    uint32_t *ids = reinterpret_cast<uint32_t *>(order_dev);
    hipLaunchKernelGGL(popular_keys_kernel, dim3((unsigned)pk_ceil_div(n_items, 256)), dim3(256), 0, pk_stream(stream), n_items,
                       scores_dev, keys, ids);
    PK_CHECK_LAUNCH("popular_keys_kernel");
    int32_t in_tmp = 0;
    const int rc = pk_radix_sort_pairs(stream, n_items, 8, keys, ids, keys_tmp, ids_tmp, 64, rwork, &in_tmp);
    if (rc != PK_OK) return rc;
    if (in_tmp && hipMemcpyAsync(ids, ids_tmp, n_items * 4, hipMemcpyDeviceToDevice, pk_stream(stream)) != hipSuccess) {
        pk_set_error("pk_popular_order: copy failed");
        return PK_E_LAUNCH;
    }
    return PK_OK;
}

__global__ __launch_bounds__(64) void popular_topk_kernel(int64_t n_items, const int64_t *__restrict__ t_indptr,
                                                          const int32_t *__restrict__ t_indices,
                                                          const int32_t *__restrict__ order, int topk, int filter_seen,
                                                          int64_t *__restrict__ out_idx) {
    extern __shared__ uint32_t bitmap[];
    const int64_t u = blockIdx.x;
    const int lane = threadIdx.x;
    const int n_words = (int)((n_items + 31) >> 5);
    int64_t *out = out_idx + u * topk;
    if (filter_seen) {
        for (int w = lane; w < n_words; w += 64) bitmap[w] = 0;
        __syncthreads();
        for (int64_t p = t_indptr[u] + lane; p < t_indptr[u + 1]; p += 64) {
            const int32_t c = t_indices[p];
            atomicOr(&bitmap[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
    }
    const uint64_t below = (1ull << lane) - 1;
    int found = 0;
    // pass 0: unseen items in the global order; pass 1 (only when they run out): the seen ones, same order
    for (int pass = 0; pass < (filter_seen ? 2 : 1) && found < topk; ++pass)
        for (int64_t b = 0; b < n_items && found < topk; b += 64) {
            const int64_t e = b + lane;
            const int32_t item = e < n_items ? order[e] : -1;
            bool take = false;
            if (item >= 0) {
                const bool sn = filter_seen && ((bitmap[item >> 5] >> (item & 31)) & 1u);
                take = (pass == 0) ? !sn : sn;
            }
            const uint64_t mask = __ballot(take);
            const int pos = found + __popcll(mask & below);
            if (take && pos < topk) out[pos] = item;
            found += __popcll(mask);
        }
}

extern "C" int pk_popular_topk(void *stream, int64_t n_users, int64_t n_items, const int64_t *t_indptr_dev,
                               const int32_t *t_indices_dev, const int32_t *order_dev, int32_t topk, int32_t filter_seen,
                               int64_t *out_idx_dev) {
    PK_REQUIRE(n_users >= 0 && n_items >= 1 && n_items <= PK_POP_MAX_ITEMS && topk >= 1 && topk <= n_items,
               "pk_popular_topk: bad shape (1 <= topk <= n_items <= %d)", PK_POP_MAX_ITEMS);
    PK_REQUIRE(t_indptr_dev && order_dev && out_idx_dev, "pk_popular_topk: null pointer");
    if (n_users == 0) return PK_OK;
    PK_REQUIRE(n_users <= 0x7fffffff, "pk_popular_topk: too many users for the grid");
    const size_t lds = filter_seen ? (size_t)pk_ceil_div(n_items, 32) * 4 : 0;
    hipLaunchKernelGGL(popular_topk_kernel, dim3((unsigned)n_users), dim3(64), lds, pk_stream(stream), n_items, t_indptr_dev,
                       t_indices_dev, order_dev, (int)topk, (int)filter_seen, out_idx_dev);
    PK_CHECK_LAUNCH("popular_topk_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_i2i() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&i2i_merge_kernel));
}
