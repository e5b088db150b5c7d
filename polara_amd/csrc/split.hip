// Splitting raw interactions on the device: the two kernels behind RecommenderArrayData.prepare() that are
// not plain sorting / scanning / compaction (those are csrc/ingest.hip and torch plumbing):
//
//   * pk_split_keys: the two-word key (key_hi, key_lo) of every candidate row.  key_hi orders by the order value (the
//     feedback or a custom column) — an order-preserving map of the fp64 bits to u64, by integer operations only, so the
//     NumPy twin is bit-equal; key_lo breaks ties by the row's position or by a counter-based draw
//     mix64(mix64(seed) + position).  Smaller key = selected first.
//   * pk_segment_select: flags[q] = 1 for the min(k, len) entries of every segment (= user) with the smallest
//     (key_hi, key_lo), lexicographic, unsigned.  Keys are distinct inside a segment (key_lo is a bijection of the
//     position), so the result is unique: no atomics touch the flags and the launch geometry cannot change it.
//
// Three paths by segment length (wave64 throughout, no inline assembly):
//   len <= 256   one wave per segment (4 segments per workgroup): the keys go to LDS once and every lane counts, for its
//                <= 4 entries, the entries with a smaller key — an entry is selected when fewer than k are.  len^2 / 64
//                compares per lane, broadcast LDS reads.  LDS: 4 waves x 256 x 16 B = 16 KB per workgroup.
//   len <= 32768 one 256-thread workgroup per segment: most-significant-digit-first radix select on the 128-bit key, 8 bits
//                per pass: a 256-bin LDS histogram of the entries that share the prefix found so far, a workgroup scan, the
//                bin in which the k-th smallest lies extends the prefix; it stops as soon as that bin is taken whole
//                (at the latest after 16 passes, when the bin holds one key).  The keys are re-read from L2 every pass
//                (<= 512 KB per segment).  LDS: 256 x 4 B histogram + 4 wave sums + 4 words = ~1.1 KB per workgroup.
//   longer       the same radix select with the whole grid on the segment and one launch pair per pass: per-workgroup LDS
//                histograms are added into a 256-bin table in HBM scratch (integer atomics on COUNTS, which do not depend
//                on arrival order), a one-workgroup kernel picks the bin and writes the state of the next pass.  Kernel
//                boundaries order the passes; nothing waits inside a kernel.
// The cost is len x passes (<= 16) whatever k is: it never grows like k x len.
#include "pk_common.h"

#define PK_SEL_WAVE_MAX 256
#define PK_SEL_WG_MAX 32768
#define PK_SEL_HUGE_GRID 1024
#define PK_SEL_WG_GRID 2048

__global__ __launch_bounds__(256) void split_keys_kernel(int64_t n, const double *__restrict__ order_vals,
                                                         const int64_t *__restrict__ pos, int mode, uint64_t seed_mixed,
                                                         uint64_t *__restrict__ key_hi, uint64_t *__restrict__ key_lo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t h = 0;
    if (!(mode & PK_SPLIT_NO_ORDER)) {
        uint64_t b = (uint64_t)__double_as_longlong(order_vals[i]);
        if ((b << 1) == 0) b = 0;                                              // -0.0 orders as +0.0
        const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);     // ascending in the value
        h = (mode & PK_SPLIT_ASCENDING) ? asc : ~asc;
    }
    const uint64_t p = (uint64_t)pos[i];
    uint64_t l;
    if (mode & PK_SPLIT_RANDOM_LO)
        l = pk_mix64(seed_mixed + p);
    else
        l = (mode & PK_SPLIT_POS_ASCENDING) ? p : ~p;
    key_hi[i] = h;
    key_lo[i] = l;
}

extern "C" int pk_split_keys(void *stream, int64_t n, const double *order_vals_dev, const int64_t *pos_dev, int32_t mode,
                             uint64_t seed, uint64_t *key_hi_dev, uint64_t *key_lo_dev) {
    PK_REQUIRE(n >= 0 && mode >= 0 && mode < 16, "pk_split_keys: bad arguments (n=%lld mode=%d)", (long long)n, mode);
    PK_REQUIRE((mode & PK_SPLIT_NO_ORDER) || order_vals_dev || n == 0, "pk_split_keys: order values needed in mode %d", mode);
    if (n == 0) return PK_OK;
    PK_REQUIRE(pos_dev && key_hi_dev && key_lo_dev, "pk_split_keys: null buffer");
    PK_REQUIRE(pk_ceil_div(n, 256) < (1ll << 31), "pk_split_keys: n too large");
    hipLaunchKernelGGL(split_keys_kernel, dim3((unsigned)pk_ceil_div(n, 256)), dim3(256), 0, pk_stream(stream), n, order_vals_dev,
                       pos_dev, mode, pk_mix64(seed), key_hi_dev, key_lo_dev);
    PK_CHECK_LAUNCH("split_keys_kernel");
    return PK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// segmented selection
// ------------------------------------------------------------------------------------------------------------
struct PkSelState {          // one segment of the whole-grid path (64 bytes)
    int64_t begin, len;
    uint64_t pre_hi, pre_lo, mask_hi, mask_lo;     // the digits found so far and the bits they occupy
    uint32_t krem, done;                           // how many of the entries sharing the prefix are still to be taken
    uint64_t pad;
};

__device__ __forceinline__ bool sel_less(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl) {
    return ah < bh || (ah == bh && al < bl);
}

// a valid segment lies inside [0, n); anything else is skipped (its flags stay 0)
__device__ __forceinline__ bool sel_segment(const int64_t *__restrict__ seg_ptr, int64_t s, int64_t n, int64_t *b, int64_t *len) {
    const int64_t lo = seg_ptr[s], hi = seg_ptr[s + 1];
    *b = lo;
    *len = hi - lo;
    return lo >= 0 && hi <= n && hi > lo;
}

template <int NT>
__device__ __forceinline__ void sel_rank_wave(const uint64_t *s_hi, const uint64_t *s_lo, int len, int lane, uint32_t k,
                                              uint8_t *__restrict__ flags_seg) {
    uint64_t mh[NT], ml[NT];
    uint32_t cnt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int i = lane + 64 * t;
        mh[t] = i < len ? s_hi[i] : 0;
        ml[t] = i < len ? s_lo[i] : 0;
        cnt[t] = 0;
    }
    for (int j = 0; j < len; ++j) {
        const uint64_t hj = s_hi[j], lj = s_lo[j];          // the same address in every lane: a broadcast read
#pragma unroll
        for (int t = 0; t < NT; ++t) cnt[t] += sel_less(hj, lj, mh[t], ml[t]) ? 1u : 0u;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int i = lane + 64 * t;
        if (i < len && cnt[t] < k) flags_seg[i] = 1;
    }
}

__global__ __launch_bounds__(256) void select_wave_kernel(int64_t n_seg, int64_t n, const int64_t *__restrict__ seg_ptr,
                                                          const uint64_t *__restrict__ key_hi, const uint64_t *__restrict__ key_lo,
                                                          uint32_t k, uint8_t *__restrict__ flags, int64_t *__restrict__ long_list,
                                                          uint32_t *__restrict__ n_long, uint32_t long_cap) {
    __shared__ uint64_t s_hi[4][PK_SEL_WAVE_MAX];
    __shared__ uint64_t s_lo[4][PK_SEL_WAVE_MAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * 4 + w;
    int len = 0;
    int64_t b = 0, L = 0;
    if (s < n_seg && sel_segment(seg_ptr, s, n, &b, &L)) {
        if (L > PK_SEL_WAVE_MAX) {
            if (lane == 0) {                                         // the ORDER of the list does not reach the result
                const uint32_t at = atomicAdd(n_long, 1u);
                if (at < long_cap) long_list[at] = s;                // (more than n / 257 such segments: they overlap; dropped)
            }
        } else if ((int64_t)k >= L) {
            for (int i = lane; i < (int)L; i += 64) flags[b + i] = 1;
        } else {
            len = (int)L;
            for (int i = lane; i < len; i += 64) {
                s_hi[w][i] = key_hi[b + i];
                s_lo[w][i] = key_lo[b + i];
            }
        }
    }
    __syncthreads();
    if (len == 0) return;
    if (len <= 64)
        sel_rank_wave<1>(s_hi[w], s_lo[w], len, lane, k, flags + b);
    else if (len <= 128)
        sel_rank_wave<2>(s_hi[w], s_lo[w], len, lane, k, flags + b);
    else
        sel_rank_wave<4>(s_hi[w], s_lo[w], len, lane, k, flags + b);
}

// exclusive prefix of c over the 256 threads of the workgroup (s_wsum: 4 words of LDS); every thread calls it
__device__ __forceinline__ uint32_t sel_block_excl(uint32_t c, uint32_t *s_wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    uint32_t excl = incl - c;
    for (int v = 0; v < w; ++v) excl += s_wsum[v];
    return excl;
}

__device__ __forceinline__ bool sel_match(uint64_t h, uint64_t l, uint64_t pre_hi, uint64_t pre_lo, uint64_t mask_hi,
                                          uint64_t mask_lo) {
    return (((h ^ pre_hi) & mask_hi) | ((l ^ pre_lo) & mask_lo)) == 0;
}

__device__ __forceinline__ bool sel_taken(uint64_t h, uint64_t l, uint64_t pre_hi, uint64_t pre_lo, uint64_t mask_hi,
                                          uint64_t mask_lo) {
    const uint64_t mh = h & mask_hi, ml = l & mask_lo;
    return mh < pre_hi || (mh == pre_hi && ml <= pre_lo);
}

__global__ __launch_bounds__(256) void select_wg_kernel(int64_t n, const int64_t *__restrict__ seg_ptr,
                                                        const uint64_t *__restrict__ key_hi, const uint64_t *__restrict__ key_lo,
                                                        uint32_t k, uint8_t *__restrict__ flags, const int64_t *__restrict__ long_list,
                                                        const uint32_t *__restrict__ n_long, PkSelState *__restrict__ huge,
                                                        uint32_t *__restrict__ n_huge, uint32_t long_cap, uint32_t huge_cap) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_digit, s_krem, s_done;
    const int tid = threadIdx.x;
    const uint32_t count = *n_long < long_cap ? *n_long : long_cap;
    for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
        int64_t b, L;
        if (!sel_segment(seg_ptr, long_list[li], n, &b, &L)) continue;        // (checked when it was listed)
        if (L > PK_SEL_WG_MAX) {
            if (tid == 0) {
                PkSelState st;
                st.begin = b;
                st.len = L;
                st.pre_hi = st.pre_lo = st.mask_hi = st.mask_lo = 0;
                st.done = (int64_t)k >= L ? 1u : 0u;           // no bit fixed: every entry counts as taken
                st.krem = k;
                st.pad = 0;
                const uint32_t at = atomicAdd(n_huge, 1u);
                if (at < huge_cap) huge[at] = st;
            }
            continue;
        }
        if ((int64_t)k >= L) {
            for (int64_t i = tid; i < L; i += 256) flags[b + i] = 1;
            continue;
        }
        uint64_t pre_hi = 0, pre_lo = 0, mask_hi = 0, mask_lo = 0;
        uint32_t krem = k;
        for (int pass = 0; pass < 16; ++pass) {
            const int shift = 56 - 8 * (pass & 7);
            s_hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < L; i += 256) {
                const uint64_t h = key_hi[b + i], l = key_lo[b + i];
                if (sel_match(h, l, pre_hi, pre_lo, mask_hi, mask_lo))
                    atomicAdd(&s_hist[(int)(((pass < 8 ? h : l) >> shift) & 255)], 1u);
            }
            __syncthreads();
            const uint32_t c = s_hist[tid];
            const uint32_t excl = sel_block_excl(c, s_wsum);
            if (excl < krem && krem <= excl + c) {             // exactly one thread: the bin of the k-th smallest
                s_digit = (uint32_t)tid;
                s_krem = krem - excl;
                s_done = (krem - excl == c) ? 1u : 0u;
            }
            __syncthreads();
            const uint64_t d = s_digit;
            krem = s_krem;
            if (pass < 8) {
                pre_hi |= d << shift;
                mask_hi |= 255ull << shift;
            } else {
                pre_lo |= d << shift;
                mask_lo |= 255ull << shift;
            }
            if (s_done) break;                                 // uniform: read from LDS after the barrier
        }
        for (int64_t i = tid; i < L; i += 256)
            if (sel_taken(key_hi[b + i], key_lo[b + i], pre_hi, pre_lo, mask_hi, mask_lo)) flags[b + i] = 1;
        __syncthreads();                                       // s_digit / s_done are rewritten for the next segment
    }
}

__global__ __launch_bounds__(256) void select_huge_hist_kernel(int pass, const uint64_t *__restrict__ key_hi,
                                                               const uint64_t *__restrict__ key_lo,
                                                               const PkSelState *__restrict__ huge,
                                                               const uint32_t *__restrict__ n_huge, uint32_t huge_cap,
                                                               uint32_t *__restrict__ ghist) {
    __shared__ uint32_t s_hist[256];
    const int tid = threadIdx.x;
    const int shift = 56 - 8 * (pass & 7);
    const uint32_t count = *n_huge < huge_cap ? *n_huge : huge_cap;
    for (uint32_t hs = 0; hs < count; ++hs) {
        const PkSelState st = huge[hs];
        if (st.done) continue;
        s_hist[tid] = 0;
        __syncthreads();
        for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < st.len; i += (int64_t)gridDim.x * 256) {
            const uint64_t h = key_hi[st.begin + i], l = key_lo[st.begin + i];
            if (sel_match(h, l, st.pre_hi, st.pre_lo, st.mask_hi, st.mask_lo))
                atomicAdd(&s_hist[(int)(((pass < 8 ? h : l) >> shift) & 255)], 1u);
        }
        __syncthreads();
        const uint32_t c = s_hist[tid];
        if (c) atomicAdd(&ghist[(int64_t)hs * 256 + tid], c);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void select_huge_pick_kernel(int pass, PkSelState *__restrict__ huge,
                                                               const uint32_t *__restrict__ n_huge, uint32_t huge_cap,
                                                               uint32_t *__restrict__ ghist) {
    __shared__ uint32_t s_wsum[4];
    const int tid = threadIdx.x;
    const int shift = 56 - 8 * (pass & 7);
    const uint32_t count = *n_huge < huge_cap ? *n_huge : huge_cap;
    for (uint32_t hs = blockIdx.x; hs < count; hs += gridDim.x) {
        const uint32_t krem = huge[hs].krem;
        const uint32_t done = huge[hs].done;
        __syncthreads();                                       // every thread has read the state before one rewrites it
        if (done) continue;
        const uint32_t c = ghist[(int64_t)hs * 256 + tid];
        ghist[(int64_t)hs * 256 + tid] = 0;                    // clean for the next pass
        const uint32_t excl = sel_block_excl(c, s_wsum);
        if (excl < krem && krem <= excl + c) {
            PkSelState *st = huge + hs;
            if (pass < 8) {
                st->pre_hi |= (uint64_t)tid << shift;
                st->mask_hi |= 255ull << shift;
            } else {
                st->pre_lo |= (uint64_t)tid << shift;
                st->mask_lo |= 255ull << shift;
            }
            st->krem = krem - excl;
            st->done = (krem - excl == c) ? 1u : 0u;
        }
        __syncthreads();                                       // s_wsum is reused
    }
}

__global__ __launch_bounds__(256) void select_huge_flag_kernel(const uint64_t *__restrict__ key_hi,
                                                               const uint64_t *__restrict__ key_lo,
                                                               const PkSelState *__restrict__ huge,
                                                               const uint32_t *__restrict__ n_huge, uint32_t huge_cap,
                                                               uint8_t *__restrict__ flags) {
    const uint32_t count = *n_huge < huge_cap ? *n_huge : huge_cap;
    for (uint32_t hs = 0; hs < count; ++hs) {
        const PkSelState st = huge[hs];
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < st.len; i += (int64_t)gridDim.x * 256)
            if (sel_taken(key_hi[st.begin + i], key_lo[st.begin + i], st.pre_hi, st.pre_lo, st.mask_hi, st.mask_lo))
                flags[st.begin + i] = 1;
    }
}

static inline int64_t sel_align(int64_t bytes) { return ((bytes + 255) / 256) * 256; }
static inline int64_t sel_long_cap(int64_t n) { return n / (PK_SEL_WAVE_MAX + 1) + 1; }
static inline int64_t sel_huge_cap(int64_t n) { return n / (PK_SEL_WG_MAX + 1) + 1; }

extern "C" int64_t pk_segment_select_work_bytes(int64_t n_seg, int64_t n) {
    (void)n_seg;
    const int64_t m = n > 0 ? n : 1;
    // counters, the list of segments beyond one wave, the states and the histograms of those beyond one workgroup
    return 256 + sel_align(sel_long_cap(m) * 8) + sel_align(sel_huge_cap(m) * (int64_t)sizeof(PkSelState)) +
           sel_align(sel_huge_cap(m) * 256 * 4);
}

extern "C" int pk_segment_select(void *stream, int64_t n_seg, int64_t n, const int64_t *seg_ptr_dev, const uint64_t *key_hi_dev,
                                 const uint64_t *key_lo_dev, int64_t k, uint8_t *flags_dev, void *work_dev) {
    PK_REQUIRE(n_seg >= 0 && n >= 0 && k >= 1 && k < (1ll << 31), "pk_segment_select: bad arguments (n_seg=%lld n=%lld k=%lld)",
               (long long)n_seg, (long long)n, (long long)k);
    PK_REQUIRE(n < 0xffffffffll && pk_ceil_div(n_seg, 4) < (1ll << 31), "pk_segment_select: sizes beyond 32-bit counts");
    if (n == 0) return PK_OK;
    PK_REQUIRE(flags_dev, "pk_segment_select: null flags");
    hipStream_t st = pk_stream(stream);
    (void)hipMemsetAsync(flags_dev, 0, (size_t)n, st);
    if (n_seg == 0) return PK_OK;
    PK_REQUIRE(seg_ptr_dev && key_hi_dev && key_lo_dev && work_dev, "pk_segment_select: null buffer");
    static_assert(sizeof(PkSelState) == 64, "PkSelState layout");
    char *w = static_cast<char *>(work_dev);
    uint32_t *n_long = reinterpret_cast<uint32_t *>(w);
    uint32_t *n_huge = n_long + 1;
    w += 256;
    int64_t *long_list = reinterpret_cast<int64_t *>(w);
    w += sel_align(sel_long_cap(n) * 8);
    PkSelState *huge = reinterpret_cast<PkSelState *>(w);
    w += sel_align(sel_huge_cap(n) * (int64_t)sizeof(PkSelState));
    uint32_t *ghist = reinterpret_cast<uint32_t *>(w);
    (void)hipMemsetAsync(n_long, 0, 256, st);
    const uint32_t k32 = (uint32_t)k;
    hipLaunchKernelGGL(select_wave_kernel, dim3((unsigned)pk_ceil_div(n_seg, 4)), dim3(256), 0, st, n_seg, n, seg_ptr_dev,
                       key_hi_dev, key_lo_dev, k32, flags_dev, long_list, n_long, (uint32_t)sel_long_cap(n));
    if (n > PK_SEL_WAVE_MAX) {            // otherwise no segment can be longer than a wave's
        const int64_t cap = sel_long_cap(n);
        hipLaunchKernelGGL(select_wg_kernel, dim3((unsigned)(cap < PK_SEL_WG_GRID ? cap : PK_SEL_WG_GRID)), dim3(256), 0, st, n,
                           seg_ptr_dev, key_hi_dev, key_lo_dev, k32, flags_dev, long_list, n_long, huge, n_huge, (uint32_t)cap,
                           (uint32_t)sel_huge_cap(n));
    }
    if (n > PK_SEL_WG_MAX) {
        const int64_t cap = sel_huge_cap(n);
        (void)hipMemsetAsync(ghist, 0, (size_t)(cap * 256 * 4), st);
        const unsigned pick_grid = (unsigned)(cap < 64 ? cap : 64);
        for (int pass = 0; pass < 16; ++pass) {
            hipLaunchKernelGGL(select_huge_hist_kernel, dim3(PK_SEL_HUGE_GRID), dim3(256), 0, st, pass, key_hi_dev, key_lo_dev,
                               huge, n_huge, (uint32_t)cap, ghist);
            hipLaunchKernelGGL(select_huge_pick_kernel, dim3(pick_grid), dim3(256), 0, st, pass, huge, n_huge, (uint32_t)cap, ghist);
        }
        hipLaunchKernelGGL(select_huge_flag_kernel, dim3(PK_SEL_HUGE_GRID), dim3(256), 0, st, key_hi_dev, key_lo_dev, huge,
                           n_huge, (uint32_t)cap, flags_dev);
    }
    PK_CHECK_LAUNCH("segment_select kernels");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_split() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&split_keys_kernel));
}
