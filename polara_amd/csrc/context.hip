// Contextual post-filtering (the reference's ItemPostFilteringMixin, contextual/models.py:5-32) as a short exact tier on top
// of the lists of the scoring pass.  The reference up-votes the items of a user's context values on the dense score chunk
// (s <- max + s + 1, context by context); wherever that arithmetic means anything (every score > -1) it is the order
//     class descending, score descending, item ascending,     class = sum_j 2^j [item in the list of the user's value of context j]
// over the unseen items.  The scoring pass already gives the class-0 part of that order (its lists); this kernel adds the rest.
//
// pk_context_merge_f64: one workgroup per user.
//   * tier: the workgroup walks the list of the user's value of context 0, then of context 1, ...  An item that an earlier
//     context's list also holds is skipped (it was emitted there), its class bits come from binary searches in the other
//     lists, a seen item is dropped (binary search in the sorted seen row).  Four lanes per item compute E_u . V_i in fp64
//     with pk_dot_chains<4>: the bits of the re-scoring and exact-row kernels, so both tiers share one within-class order.
//   * selection: keys (score, class << 28 | item) in LDS, sorted best first by a bitonic sort (the sort of i2i_keys.h with a
//     4-bit class field).  A list longer than the window is taken in rounds: the first round takes a whole window, after it
//     the best topk stay in the first slots and `window - topk` new entries follow.  The host bounds the rounds per context
//     from the longest list, so every loop is bounded.
//   * output: the m = min(topk, emitted) tier entries, then the entries of the base list that the tier did not emit (an entry
//     is skipped iff it is in some list of the user and not filtered as seen), in their order, up to topk.  If m < topk at
//     most m base entries are tier entries, so the plain top-k base list always holds the topk - m plain ones needed.
// List entries are NOT range-checked here (the host layer does that).
#include "i2i_keys.h"   // i2i_key, i2i_pair, i2i_pow2, i2i_lower_bound
#include "pk_dot.h"

#define PK_CTX_MAX 4
#define PK_CTX_WIN 4096              // keys of one workgroup: 12 bytes each, 48 KB
#define PK_CTX_THREADS 256
#define PK_CTX_MAX_TOPK 1024
#define PK_CTX_MAX_RANK 1024         // the user's row sits in LDS next to the keys
#define PK_CTX_ITEM_MASK 0x0fffffffu
#define PK_CTX_NONE PK_CTX_ITEM_MASK   // class 0: behind every tier entry (their class is >= 1)

extern "C" int32_t pk_context_window(void) { return PK_CTX_WIN; }
extern "C" int32_t pk_context_max(void) { return PK_CTX_MAX; }

struct CtxLists {
    const int32_t *user_value[PK_CTX_MAX];
    const int64_t *value_ptr[PK_CTX_MAX];
    const int32_t *value_items[PK_CTX_MAX];
};

// a strictly better than b under (class desc, score desc, item asc); m = class << 28 | item
__device__ __forceinline__ bool ctx_better(uint64_t sa, uint32_t ma, uint64_t sb, uint32_t mb) {
    const uint32_t ca = ma >> 28, cb = mb >> 28;
    if (ca != cb) return ca > cb;
    if (sa != sb) return sa > sb;
    return (ma & PK_CTX_ITEM_MASK) < (mb & PK_CTX_ITEM_MASK);
}
__device__ __forceinline__ void ctx_cmpx(uint64_t *s, uint32_t *m, int i, int l) {
    if (ctx_better(s[l], m[l], s[i], m[i])) {
        const uint64_t ts = s[i];
        const uint32_t tm = m[i];
        s[i] = s[l];
        m[i] = m[l];
        s[l] = ts;
        m[l] = tm;
    }
}
// best-first bitonic sort of n (power of two) keys in LDS by the block's threads
__device__ void ctx_sort(uint64_t *s, uint32_t *m, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += PK_CTX_THREADS) {
                const int i = i2i_pair(t, j);
                if ((i & k) == 0)
                    ctx_cmpx(s, m, i, i + j);
                else
                    ctx_cmpx(s, m, i + j, i);
            }
            __syncthreads();
        }
}

__device__ __forceinline__ int ctx_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

__device__ __forceinline__ bool ctx_member(const int32_t *__restrict__ idx, int64_t lo, int64_t hi, int32_t x) {
    const int64_t p = i2i_lower_bound(idx, lo, hi, x);
    return p < hi && idx[p] == x;
}

// the key of a score: -0 counts as +0 (the exact path compares the doubles), NaN last
__device__ __forceinline__ uint64_t ctx_key(double s) {
    return i2i_key((s != s) ? -INFINITY : (s == 0.0 ? 0.0 : s));
}

// dynamic LDS: the user's row [K rounded up to even] | keys [win] (8 B) | class and item [win] (4 B)
__global__ __launch_bounds__(PK_CTX_THREADS) void context_merge_kernel(
    int K, const double *__restrict__ V, int64_t ldv, const double *__restrict__ E, int64_t lde,
    const int64_t *__restrict__ seen_ptr, const int32_t *__restrict__ seen_idx, int n_ctx, CtxLists cx, int win, int rounds,
    const int64_t *__restrict__ base_idx, int topk, int64_t *__restrict__ out_idx, int32_t *__restrict__ out_class,
    const int32_t *__restrict__ order) {
    extern __shared__ __align__(16) unsigned char ctx_lds[];
    __shared__ int64_t s_lo[PK_CTX_MAX], s_hi[PK_CTX_MAX];
    __shared__ int s_cnt[PK_CTX_THREADS / 64];
    double *s_e = reinterpret_cast<double *>(ctx_lds);
    uint64_t *ks = reinterpret_cast<uint64_t *>(s_e + ((K + 1) & ~1));
    uint32_t *km = reinterpret_cast<uint32_t *>(ks + win);
    const int tid = threadIdx.x, q = tid & 3;
    const int64_t u = order ? (int64_t)order[blockIdx.x] : (int64_t)blockIdx.x;
    const int64_t t0 = seen_ptr ? seen_ptr[u] : 0, t1 = seen_ptr ? seen_ptr[u + 1] : 0;
    const bool vvec2 = ((ldv & 1) == 0) && ((reinterpret_cast<uintptr_t>(V) & 15) == 0);

    if (tid < PK_CTX_MAX) {
        int64_t lo = 0, hi = 0;
        if (tid < n_ctx) {
            const int32_t v = cx.user_value[tid][u];
            if (v >= 0) {
                lo = cx.value_ptr[tid][v];
                hi = cx.value_ptr[tid][v + 1];
            }
        }
        s_lo[tid] = lo;
        s_hi[tid] = hi;
    }
    for (int c = tid; c < K; c += PK_CTX_THREADS) s_e[c] = E[u * lde + c];
    __syncthreads();

    // ---- the tier: the best topk of the user's context items in the first slots ----
    int carried = 0;          // slots at the front that hold the best so far: 0 before the first sort, topk after it
    for (int j = 0; j < n_ctx; ++j) {
        const int64_t lo = s_lo[j], len = s_hi[j] - lo;
        const int32_t *__restrict__ items = cx.value_items[j];
        int64_t p0 = 0;
        for (int r = 0; r < rounds && p0 < len; ++r) {
            const int room = win - carried;
            const int take = (int)((len - p0 < (int64_t)room) ? (len - p0) : (int64_t)room);
            const int n = ctx_pow2(carried + take);
            for (int l0 = 0; l0 < n - carried; l0 += PK_CTX_THREADS / 4) {
                const int li = l0 + (tid >> 2);
                bool valid = li < take;             // the same for the four lanes of an item
                int32_t item = 0;
                uint32_t cls = 1u << j;
                if (valid) {
                    item = items[lo + p0 + li];
                    for (int jj = 0; jj < n_ctx; ++jj) {
                        if (jj == j || s_hi[jj] == s_lo[jj]) continue;
                        if (ctx_member(cx.value_items[jj], s_lo[jj], s_hi[jj], item)) {
                            if (jj < j) valid = false;        // emitted with context jj's list
                            cls |= 1u << jj;
                        }
                    }
                    if (valid && seen_ptr) valid = !ctx_member(seen_idx, t0, t1, item);
                }
                double sc = 0.0;
                if (valid) sc = pk_dot_chains<4>(V + (int64_t)item * ldv, s_e, K, q, vvec2, true);
                if (q == 0 && li < n - carried) {
                    ks[carried + li] = valid ? ctx_key(sc) : 0ull;
                    km[carried + li] = valid ? ((cls << 28) | (uint32_t)item) : PK_CTX_NONE;
                }
            }
            __syncthreads();
            ctx_sort(ks, km, n);
            if (carried == 0) {
                for (int k = n + tid; k < topk; k += PK_CTX_THREADS) {      // a first window shorter than the list
                    ks[k] = 0ull;
                    km[k] = PK_CTX_NONE;
                }
                carried = topk;
                __syncthreads();
            }
            p0 += take;
        }
    }

    // ---- output: tier entries, then the base entries the tier did not emit ----
    int m = 0;                // tier entries among the first topk slots (they come first: class >= 1)
    if (carried) {
        // (sorted: the tier entries are a prefix, so the count is the first slot of class 0)
        int lo_k = 0, hi_k = topk;
        while (lo_k < hi_k) {
            const int mid = (lo_k + hi_k) >> 1;
            if ((km[mid] >> 28) != 0)
                lo_k = mid + 1;
            else
                hi_k = mid;
        }
        m = lo_k;
    }
    int64_t *orow = out_idx + u * topk;
    int32_t *crow = out_class ? out_class + u * topk : nullptr;
    for (int k = tid; k < m; k += PK_CTX_THREADS) {
        orow[k] = (int64_t)(km[k] & PK_CTX_ITEM_MASK);
        if (crow) crow[k] = (int32_t)(km[k] >> 28);
    }
    int written = m;
    const int lane = tid & 63, wave = tid >> 6;
    for (int b0 = 0; b0 < topk && written < topk; b0 += PK_CTX_THREADS) {
        const int t = b0 + tid;
        int64_t b = -1;
        bool keep = false;
        if (t < topk) {
            b = base_idx[u * topk + t];
            keep = true;                              // pads (-1) stay, behind everything kept before them
            if (b >= 0 && m > 0) {
                bool in_list = false;
                for (int jj = 0; jj < n_ctx; ++jj)
                    if (s_hi[jj] > s_lo[jj] && ctx_member(cx.value_items[jj], s_lo[jj], s_hi[jj], (int32_t)b)) in_list = true;
                if (in_list && !(seen_ptr && ctx_member(seen_idx, t0, t1, (int32_t)b))) keep = false;   // it is in the tier
            }
        }
        const uint64_t bal = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = written, total = 0;
        for (int w = 0; w < PK_CTX_THREADS / 64; ++w) {
            if (w < wave) before += s_cnt[w];
            total += s_cnt[w];
        }
        const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && pos < topk) {
            orow[pos] = b;
            if (crow) crow[pos] = 0;
        }
        written += total;
        __syncthreads();
    }
    for (int k = written + tid; k < topk; k += PK_CTX_THREADS) {
        orow[k] = -1;
        if (crow) crow[k] = 0;
    }
}

extern "C" int pk_context_merge_f64(void *stream, int64_t n_users, int64_t n_items, int32_t K, const double *V_dev, int64_t ldv,
                                    const double *E_dev, int64_t lde, const int64_t *seen_indptr_dev,
                                    const int32_t *seen_indices_dev, int32_t n_ctx, const int32_t *const *user_value_dev,
                                    const int64_t *const *value_ptr_dev, const int32_t *const *value_items_dev, int64_t max_list,
                                    const int64_t *base_idx_dev, int32_t topk, int64_t *out_idx_dev, int32_t *out_class_dev,
                                    const int32_t *order_dev) {
    PK_REQUIRE(n_ctx >= 1 && n_ctx <= PK_CTX_MAX, "pk_context_merge_f64: %d contexts outside 1..%d", (int)n_ctx, PK_CTX_MAX);
    PK_REQUIRE(K >= 1 && K <= PK_CTX_MAX_RANK, "pk_context_merge_f64: rank %d outside 1..%d", (int)K, PK_CTX_MAX_RANK);
    PK_REQUIRE(topk >= 1 && topk <= PK_CTX_MAX_TOPK, "pk_context_merge_f64: topk %d outside 1..%d", (int)topk, PK_CTX_MAX_TOPK);
    PK_REQUIRE(n_users >= 0 && n_users <= 0x7fffffff && n_items >= 1 && n_items <= (int64_t)PK_CTX_ITEM_MASK,
               "pk_context_merge_f64: bad shape (n_users %lld, n_items %lld; items < 2^28)", (long long)n_users, (long long)n_items);
    PK_REQUIRE(V_dev && E_dev && base_idx_dev && out_idx_dev && user_value_dev && value_ptr_dev && value_items_dev,
               "pk_context_merge_f64: null pointer");
    PK_REQUIRE(base_idx_dev != out_idx_dev, "pk_context_merge_f64: the lists are not merged in place");
    PK_REQUIRE(seen_indptr_dev || !seen_indices_dev, "pk_context_merge_f64: seen indices without their row pointers");
    PK_REQUIRE(ldv >= K && lde >= K, "pk_context_merge_f64: bad strides (ldv %lld, lde %lld, rank %d)", (long long)ldv,
               (long long)lde, (int)K);
    PK_REQUIRE(max_list >= 0 && max_list <= n_items, "pk_context_merge_f64: longest list %lld of %lld items", (long long)max_list,
               (long long)n_items);
    CtxLists cx;
    for (int j = 0; j < PK_CTX_MAX; ++j) {
        cx.user_value[j] = j < n_ctx ? user_value_dev[j] : nullptr;
        cx.value_ptr[j] = j < n_ctx ? value_ptr_dev[j] : nullptr;
        cx.value_items[j] = j < n_ctx ? value_items_dev[j] : nullptr;
        // (an empty context — no value has items — may come without an item array)
        PK_REQUIRE(j >= n_ctx || (cx.user_value[j] && cx.value_ptr[j] && (cx.value_items[j] || max_list == 0)),
                   "pk_context_merge_f64: null pointer in context %d", j);
    }
    if (n_users == 0) return PK_OK;
    // the window: as short as the longest list allows (less LDS: more workgroups per CU); always room for one new entry
    int64_t want = max_list + topk;
    if (want < 64) want = 64;
    const int win = want >= PK_CTX_WIN ? PK_CTX_WIN : i2i_pow2((int32_t)want);
    // rounds of one context: its first may take a whole window, every other one takes win - topk >= 1 new entries
    const int rounds = max_list == 0 ? 1 : (int)pk_ceil_div(max_list, win - topk);
    const size_t lds = (size_t)win * 12 + (size_t)((K + 1) & ~1) * 8;
    hipLaunchKernelGGL(context_merge_kernel, dim3((unsigned)n_users), dim3(PK_CTX_THREADS), lds, pk_stream(stream), (int)K, V_dev, ldv,
                       E_dev, lde, seen_indptr_dev, seen_indices_dev, (int)n_ctx, cx, win, rounds, base_idx_dev, (int)topk,
                       out_idx_dev, out_class_dev, order_dev);
    PK_CHECK_LAUNCH("context_merge_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_context() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&context_merge_kernel));
}
