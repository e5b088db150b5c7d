// The sampled-negatives evaluation protocol (RandomSampleEvaluationSVDMixin, models.py:1095-1183; lib/sparse.py::inner_product_at
// and lib/sampler.py::mf_random_item_scoring under it): every test user ranks a short list of candidate items — its holdout
// items followed by items it has not seen — instead of the whole catalogue.
//
// pk_candidates_topk_f64: s[u, c] = sum_f P[u, f] * V[cand[u, c], f] and the top-k COLUMN POSITIONS of every row.
//   Numerical contract: the sum starts from +0.0 and runs over f ascending, every term a separately rounded fp64 multiply
//   and add (cand_mul_add: contraction switched off) — the loop of inner_product_at and of mf_random_item_scoring, so for
//   the same P and V the scores are bit-equal to theirs.  Selection: score descending, position ascending — the total order
//   of pk_topk_rows_f64 (-0 equals +0, NaN last).
//   * one workgroup per user (64 threads up to 256 candidates, else 256); the user's row of P sits in LDS and every lane
//     reads it at the same address (a broadcast); lane t owns the candidates t, t + NT, ... and walks each one's row of V
//     with 16-byte loads where the layout allows (unit column stride, even leading dimension, aligned base), else with
//     strided 8-byte loads — the sums are the same;
//   * the scores never leave LDS (unless the caller asks for them): they become the keys of i2i_keys.h, sorted in place by
//     its bitonic sort, and the first topk positions are the list;
//   * more than PK_CAND_FUSED_MAX candidates per user do not fit: the scores are written out (cand_scores_kernel) and
//     pk_topk_rows_f64 selects.
//   Candidate ids are NOT range-checked here (the host layer does that).
//
// pk_sample_unseen: n distinct items per user, uniform over the items outside the user's row of a CSR and outside its row of a
//   second CSR, in draw order.  The stream is defined so that NumPy can restate it draw by draw (tests/sampled_reference.py):
//     draw t = 0, 1, 2, ...:  z = mix64(seed_u * 2^32 + t)  (the splitmix64 finaliser, pk_mix64), w = z >> 32,
//                             m = w * n_items (64-bit), the draw is REJECTED when (m mod 2^32) < (2^32 mod n_items), else x = m >> 32;
//     x is ACCEPTED when it is in neither row and was not accepted before; the output is the first n accepted x in order of t.
//   * one wave per user evaluates 64 consecutive t per round: exclusion by binary search in the sorted row and a scan of the
//     (short) second row, membership by a scan of the accepted list in LDS, duplicates inside the round resolved in lane
//     order, then one append;
//   * every loop is bounded: the number of rounds comes from the host (pk_sample_round_limit, at most PK_SAMPLE_MAX_ROUNDS:
//     a launch that would need more is refused); a user that is not done by then sets *err_dev and the wave returns.
#include <math.h>
#include "i2i_keys.h"

#define PK_CAND_MAX_RANK 256
#define PK_CAND_FUSED_MAX 4096       // candidates of one user the fused launch keeps in LDS (12 bytes each)
#define PK_SAMPLE_MAX_N 8192         // accepted items of one user kept in LDS (4 bytes each)

extern "C" int32_t pk_candidates_fused_max(void) { return PK_CAND_FUSED_MAX; }
extern "C" int32_t pk_candidates_max_rank(void) { return PK_CAND_MAX_RANK; }
extern "C" int32_t pk_sample_max_n(void) { return PK_SAMPLE_MAX_N; }

// acc + a * b as a separately rounded multiply and add (see spsp_mul_add, simagg.hip: without the pragma the two fuse into
// v_fmac_f64, whose sums differ from the reference's in the last bit)
__device__ __forceinline__ double cand_mul_add(double acc, double a, double b) {
#pragma clang fp contract(off)
    const double prod = a * b;
    return acc + prod;
}

// sum_f prow[f] * v[f * sv], f ascending from +0.0; vec: v is 16-byte aligned with unit stride (prow always is)
__device__ __forceinline__ double cand_dot(const double *prow, const double *__restrict__ v, int r, int64_t sv, bool vec) {
    double acc = 0.0;
    if (vec) {
        const double2 *p2 = reinterpret_cast<const double2 *>(prow);
        const double2 *v2 = reinterpret_cast<const double2 *>(v);
        int f = 0;
        for (; f + 1 < r; f += 2) {
            const double2 a = p2[f >> 1], b = v2[f >> 1];
            acc = cand_mul_add(acc, a.x, b.x);
            acc = cand_mul_add(acc, a.y, b.y);
        }
        if (f < r) acc = cand_mul_add(acc, prow[f], v[f]);
    } else {
        for (int f = 0; f < r; ++f) acc = cand_mul_add(acc, prow[f], v[(int64_t)f * sv]);
    }
    return acc;
}

// the key of a score under pk_topk_rows_f64's order: -0 counts as +0, NaN as -inf
__device__ __forceinline__ uint64_t cand_key(double s) {
    const double t = (s != s) ? -INFINITY : (s == 0.0 ? 0.0 : s);
    return i2i_key(t);
}

// dynamic LDS: the user's row [r rounded up to even: a multiple of 16 bytes, read as double2] | keys [n] (8 B) | positions [n] (4 B)
template <int NT>
__global__ __launch_bounds__(NT) void cand_topk_kernel(int r, const double *__restrict__ P, int64_t ldp,
                                                       const double *__restrict__ V, int64_t ldv, int64_t sv, int vec,
                                                       const int32_t *__restrict__ cand, int C, int n, int topk,
                                                       int64_t *__restrict__ out_idx, double *__restrict__ out_scores) {
    extern __shared__ __align__(16) unsigned char cand_lds[];
    double *prow = reinterpret_cast<double *>(cand_lds);
    uint64_t *ks = reinterpret_cast<uint64_t *>(prow + ((r + 1) & ~1));
    uint32_t *km = reinterpret_cast<uint32_t *>(ks + n);
    const int64_t u = blockIdx.x;
    for (int f = threadIdx.x; f < r; f += NT) prow[f] = P[u * ldp + f];
    __syncthreads();
    const int32_t *crow = cand + u * C;
    for (int c = threadIdx.x; c < n; c += NT) {
        if (c < C) {
            const double s = cand_dot(prow, V + (int64_t)crow[c] * ldv, r, sv, vec != 0);
            if (out_scores) out_scores[u * C + c] = s;
            ks[c] = cand_key(s);
            km[c] = (2u << 30) | (uint32_t)c;
        } else {                              // padding up to the power of two: sorts behind every candidate
            ks[c] = 0;
            km[c] = PK_I2I_ITEM_MASK;
        }
    }
    __syncthreads();
    i2i_sort<NT>(ks, km, n);
    for (int k = threadIdx.x; k < topk; k += NT) out_idx[u * topk + k] = (int64_t)(km[k] & PK_I2I_ITEM_MASK);
}

// scores only (C above the fused limit): block (u, j) computes candidates [256 j, 256 j + 256) of user u
__global__ __launch_bounds__(256) void cand_scores_kernel(int r, const double *__restrict__ P, int64_t ldp,
                                                          const double *__restrict__ V, int64_t ldv, int64_t sv, int vec,
                                                          const int32_t *__restrict__ cand, int64_t C,
                                                          double *__restrict__ out_scores) {
    __shared__ __align__(16) double prow[PK_CAND_MAX_RANK];
    const int64_t u = blockIdx.x;
    for (int f = threadIdx.x; f < r; f += 256) prow[f] = P[u * ldp + f];
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (c < C) out_scores[u * C + c] = cand_dot(prow, V + (int64_t)cand[u * C + c] * ldv, r, sv, vec != 0);
}

extern "C" int pk_candidates_topk_f64(void *stream, int64_t n_users, int64_t n_items, int32_t r, const double *P_dev, int64_t ldp,
                                      const double *V_dev, int64_t ldv, int64_t v_col_stride, const int32_t *cand_dev, int64_t C,
                                      int32_t topk, int64_t *out_idx_dev, double *out_scores_dev) {
    PK_REQUIRE(r >= 1 && r <= PK_CAND_MAX_RANK, "pk_candidates_topk_f64: rank %d outside 1..%d", (int)r, PK_CAND_MAX_RANK);
    PK_REQUIRE(C >= 1 && C <= (int64_t)PK_I2I_ITEM_MASK && topk >= 1 && topk <= C,
               "pk_candidates_topk_f64: topk %d and %lld candidates per user (1 <= topk <= candidates < 2^30)", (int)topk, (long long)C);
    PK_REQUIRE(n_users >= 0 && n_users <= 0x7fffffff && n_items >= 1, "pk_candidates_topk_f64: bad shape (n_users %lld, n_items %lld)",
               (long long)n_users, (long long)n_items);
    PK_REQUIRE(P_dev && V_dev && cand_dev && out_idx_dev, "pk_candidates_topk_f64: null pointer");
    PK_REQUIRE(ldp >= r && ldv >= 1 && v_col_stride >= 1 && (v_col_stride == 1 ? ldv >= r : v_col_stride >= n_items),
               "pk_candidates_topk_f64: bad strides (ldp %lld, ldv %lld, column stride %lld)", (long long)ldp, (long long)ldv,
               (long long)v_col_stride);
    PK_REQUIRE(C <= PK_CAND_FUSED_MAX || out_scores_dev,
               "pk_candidates_topk_f64: more than %d candidates per user need the score buffer", PK_CAND_FUSED_MAX);
    if (n_users == 0) return PK_OK;
    hipStream_t s = pk_stream(stream);
    const int vec = v_col_stride == 1 && (ldv & 1) == 0 && (reinterpret_cast<uintptr_t>(V_dev) & 15) == 0;
    if (C > PK_CAND_FUSED_MAX) {
        PK_REQUIRE(pk_ceil_div(C, 256) <= 65535, "pk_candidates_topk_f64: too many candidates for the grid");
        hipLaunchKernelGGL(cand_scores_kernel, dim3((unsigned)n_users, (unsigned)pk_ceil_div(C, 256)), dim3(256), 0, s, (int)r, P_dev,
                           ldp, V_dev, ldv, v_col_stride, vec, cand_dev, C, out_scores_dev);
        PK_CHECK_LAUNCH("cand_scores_kernel");
        return pk_topk_rows_f64(stream, n_users, C, out_scores_dev, C, topk, out_idx_dev);
    }
    const int n = i2i_pow2((int32_t)C);
    const size_t lds = (size_t)n * 12 + (size_t)((r + 1) & ~1) * 8;
    if (n <= 256)
        hipLaunchKernelGGL(cand_topk_kernel<64>, dim3((unsigned)n_users), dim3(64), lds, s, (int)r, P_dev, ldp, V_dev, ldv, v_col_stride,
                           vec, cand_dev, (int)C, n, (int)topk, out_idx_dev, out_scores_dev);
    else
        hipLaunchKernelGGL(cand_topk_kernel<256>, dim3((unsigned)n_users), dim3(256), lds, s, (int)r, P_dev, ldp, V_dev, ldv,
                           v_col_stride, vec, cand_dev, (int)C, n, (int)topk, out_idx_dev, out_scores_dev);
    PK_CHECK_LAUNCH("cand_topk_kernel");
    return PK_OK;
}

// ---- sampling without replacement --------------------------------------------------------------------------------------
// Rounds of 64 draws after which every user must be done, given that each has at least min_eligible >= n items outside its
// rows.  A user is NOT done after t accepted-or-repeated draws iff m = e - n + 1 of its e eligible items are still unseen:
//   P <= C(e, n - 1) (1 - m / N)^t <= exp((n - 1) ln(e E / (n - 1)) - t m / N)       (union over the sets of m items)
//   P <= n exp(-t / N)                                                                (union over the last of n items, e = n)
// so t = min(N / m ((n - 1) ln(e E / (n - 1)) + 32), N (ln n + 32)) leaves less than exp(-32) per user; the draws the unbiased
// mapping rejects (a share below N / 2^32) stretch it by 2^32 / (2^32 - N).  With most of the catalogue eligible this is a
// few times n draws; it reaches N (ln n + 32) only for a user with hardly more than n eligible items.
extern "C" int64_t pk_sample_round_limit(int64_t n_items, int32_t n, int64_t min_eligible) {
    if (n < 1 || n_items < n || n_items > 0x7fffffff || min_eligible < n || min_eligible > n_items) return -1;
    const double N = (double)n_items, e = (double)min_eligible, m = e - n + 1.0;
    const double by_sets = N / m * ((n > 1 ? (n - 1.0) * log(e * 2.718281828459045 / (n - 1.0)) : 0.0) + 32.0);
    const double by_last = N * (log((double)n) + 32.0);
    const double draws = (by_sets < by_last ? by_sets : by_last) * (4294967296.0 / (4294967296.0 - N));
    return (int64_t)ceil(draws / 64.0) + 1;
}
// A launch is refused when its limit exceeds this: one wave would otherwise run up to that many rounds, each with a scan of its
// accepted list, on a machine it shares.
#define PK_SAMPLE_MAX_ROUNDS (1 << 16)
extern "C" int32_t pk_sample_max_rounds(void) { return PK_SAMPLE_MAX_ROUNDS; }

__device__ __forceinline__ bool sample_in_sorted(const int32_t *__restrict__ idx, int64_t lo, int64_t hi, int32_t x) {
    const int64_t p = i2i_lower_bound(idx, lo, hi, x);
    return p < hi && idx[p] == x;
}

__global__ __launch_bounds__(64) void sample_unseen_kernel(int64_t n_items, const int64_t *__restrict__ t_indptr,
                                                           const int32_t *__restrict__ t_indices,
                                                           const int64_t *__restrict__ h_indptr,
                                                           const int32_t *__restrict__ h_indices, int n,
                                                           const uint32_t *__restrict__ seeds, int64_t max_rounds,
                                                           int32_t *__restrict__ out, int32_t *__restrict__ err) {
    extern __shared__ int32_t sample_acc[];          // [n] the accepted items
    const int64_t u = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t hi_seed = (uint64_t)seeds[u] << 32;
    const uint32_t thresh = (uint32_t)((1ull << 32) % (uint64_t)n_items);
    const int64_t t0 = t_indptr[u], t1 = t_indptr[u + 1];
    const int64_t h0 = h_indptr ? h_indptr[u] : 0, h1 = h_indptr ? h_indptr[u + 1] : 0;
    int count = 0;
    for (int64_t round = 0; round < max_rounds && count < n; ++round) {
        const uint64_t t = (uint64_t)round * 64 + lane;           // < 2^32 (checked on the host)
        const uint64_t m = (pk_mix64(hi_seed | t) >> 32) * (uint64_t)n_items;
        const int32_t x = (int32_t)(m >> 32);
        bool ok = (uint32_t)m >= thresh;
        if (ok) ok = !sample_in_sorted(t_indices, t0, t1, x);
        if (ok)
            for (int64_t p = h0; p < h1; ++p)
                if (h_indices[p] == x) {
                    ok = false;
                    break;
                }
        if (ok)
            for (int j = 0; j < count; ++j)
                if (sample_acc[j] == x) {
                    ok = false;
                    break;
                }
        // duplicates inside the round: the lowest surviving lane stands, every later lane with its value falls
        uint64_t todo = __ballot(ok);
        while (todo) {
            const int e = __builtin_ctzll(todo);
            const int32_t xe = __builtin_amdgcn_readlane(x, e);
            if (lane > e && x == xe) ok = false;
            todo = __ballot(ok) & ~((2ull << e) - 1ull);
        }
        const uint64_t mask = __ballot(ok);
        const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (ok && pos < n) {
            sample_acc[pos] = x;
            out[u * n + pos] = x;
        }
        count += __popcll(mask);
        __syncthreads();                                          // one wave: orders the LDS appends before the next scan
    }
    if (count < n && lane == 0) atomicOr(err, 1);
}

extern "C" int pk_sample_unseen(void *stream, int64_t n_users, int64_t n_items, const int64_t *t_indptr_dev,
                                const int32_t *t_indices_dev, const int64_t *h_indptr_dev, const int32_t *h_indices_dev, int32_t n,
                                int64_t min_eligible, const uint32_t *seeds_dev, int32_t *out_dev, int32_t *err_dev) {
    PK_REQUIRE(n >= 1 && n <= PK_SAMPLE_MAX_N, "pk_sample_unseen: %d items per user outside 1..%d", (int)n, PK_SAMPLE_MAX_N);
    PK_REQUIRE(n_users >= 0 && n_users <= 0x7fffffff && n_items >= n && n_items <= 0x7fffffff,
               "pk_sample_unseen: bad shape (n_users %lld, n_items %lld, n %d)", (long long)n_users, (long long)n_items, (int)n);
    PK_REQUIRE(t_indptr_dev && seeds_dev && out_dev && err_dev && (!h_indptr_dev || h_indices_dev),
               "pk_sample_unseen: null pointer");
    PK_REQUIRE(min_eligible >= n && min_eligible <= n_items, "pk_sample_unseen: %lld eligible items for %d wanted of %lld",
               (long long)min_eligible, (int)n, (long long)n_items);
    const int64_t max_rounds = pk_sample_round_limit(n_items, n, min_eligible);
    PK_REQUIRE(max_rounds >= 1 && max_rounds <= PK_SAMPLE_MAX_ROUNDS,
               "pk_sample_unseen: refused — a user with only %lld items to draw %d from (of %lld) may need %lld rounds of 64 draws, "
               "the limit is %d", (long long)min_eligible, (int)n, (long long)n_items, (long long)max_rounds, PK_SAMPLE_MAX_ROUNDS);
    if (n_users == 0) return PK_OK;
    hipLaunchKernelGGL(sample_unseen_kernel, dim3((unsigned)n_users), dim3(64), (size_t)n * 4, pk_stream(stream), n_items,
                       t_indptr_dev, t_indices_dev, h_indptr_dev, h_indices_dev, (int)n, seeds_dev, max_rounds, out_dev, err_dev);
    PK_CHECK_LAUNCH("sample_unseen_kernel");
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_sampled() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sample_unseen_kernel));
}
